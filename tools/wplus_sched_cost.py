"""What the projector schedule costs per W+ step: the same inversion (1024², B=8, 100 steps, two streams, precision
'f16s-g2', launch plans) with every option on against all off, alternated in one process after a warm-up inversion of each; wall time per
inversion between device synchronisations.  profiles/wplus_sched_cost.txt.
    python tools/wplus_sched_cost.py [--batch 8] [--size 1024] [--wsteps 100] [--streams 2] [--reps 3]"""
import argparse, os, sys, time
R_ = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(R_, 'ood-gan-inversion_amd'))
import torch
from oodgan import synth
from oodgan.engine import GeneratorEngine, WPlusInverter

ap = argparse.ArgumentParser()
ap.add_argument('--batch', type=int, default=8)
ap.add_argument('--size', type=int, default=1024)
ap.add_argument('--wsteps', type=int, default=100)
ap.add_argument('--streams', type=int, default=2)
ap.add_argument('--reps', type=int, default=3)
a = ap.parse_args()
B, size, dev = a.batch, a.size, torch.device('cuda:0')
eng = GeneratorEngine({k: v.to(dev) for k, v in synth.generator_state(size, seed=0).items()}, size, precision='f16s-g2')
target = torch.cat([synth.make_images(size, 1, seed=1000 + i) for i in range(B)]).to(dev)
noises = [n.to(dev) for n in synth.make_noises(size, B, seed=7)]
w0 = synth.make_latents(size, B, seed=14, std=0.3).to(dev)
ON = dict(lr_rampup=0.05, lr_rampdown=0.25, latent_noise=0.05, noise_ramp=0.75, latent_reg=0.1)
res, info = {'off': [], 'on': []}, {}
for rep in range(a.reps + 1):          # the first round warms both up
    for name, kw in (('off', {}), ('on', ON)):
        inv = WPlusInverter(eng, **kw)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        _, losses = inv.invert(target, w0, noises, steps=a.wsteps, streams=a.streams, latent_anchor=w0 if kw else None)
        torch.cuda.synchronize()
        info[name] = (inv.last_plan, inv.last_stats, losses[-1].mean().item())
        if rep:
            res[name].append((time.perf_counter() - t0) * 1e3 / a.wsteps)
for name, v in res.items():
    plan, stats, last = info[name]
    print(f'W+ step, B={B} {size}², {a.streams} streams, schedule {name}: {min(v):.3f} ms per step (best of {len(v)}: {", ".join(f"{x:.3f}" for x in v)}; '
          f'{a.wsteps} steps per inversion, set-up steps included); launches per recorded step {plan["launches"]}, rollbacks {stats["rollbacks"]}, '
          f'final mean loss {last:.5f}')
print(f'the schedule costs {min(res["on"]) - min(res["off"]):.3f} ms per step: ratio {min(res["on"]) / min(res["off"]):.4f}')
