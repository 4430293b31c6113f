"""What the latent controls cost per W+ step: the same inversion (1024², B=8, 100 steps, precision 'f16s-g2', launch plans)
with the defaults, with latent_space='w' and with delta_reg + layer_lr, alternated in one process after a warm-up inversion of each; wall
time per inversion between device synchronisations.  profiles/latent_controls_cost.txt.
    python tools/latent_controls_cost.py [--batch 8] [--size 1024] [--wsteps 100] [--streams 1] [--reps 3]"""
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
ap.add_argument('--streams', type=int, default=1)
ap.add_argument('--reps', type=int, default=3)
a = ap.parse_args()
B, size, dev = a.batch, a.size, torch.device('cuda:0')
eng = GeneratorEngine({k: v.to(dev) for k, v in synth.generator_state(size, seed=0).items()}, size, precision='f16s-g2')
target = torch.cat([synth.make_images(size, 1, seed=1000 + i) for i in range(B)]).to(dev)
noises = [n.to(dev) for n in synth.make_noises(size, B, seed=7)]
w0 = synth.make_latents(size, B, seed=14, std=0.3).to(dev)
L = w0.shape[1]
LEGS = (('defaults', {}), ("latent_space='w'", dict(latent_space='w')),
        ('delta_reg + layer_lr', dict(delta_reg=0.5, layer_lr=[1.0] * 8 + [0.0] * (L - 8))))
res, info = {name: [] for name, _ in LEGS}, {}
for rep in range(a.reps + 1):          # the first round warms every leg up
    for name, kw in LEGS:
        inv = WPlusInverter(eng, **kw)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        _, losses = inv.invert(target, w0, noises, steps=a.wsteps, streams=a.streams)
        torch.cuda.synchronize()
        info[name] = (inv.last_plan, inv.last_stats, losses[-1].mean().item())
        if rep:
            res[name].append((time.perf_counter() - t0) * 1e3 / a.wsteps)
for name, v in res.items():
    plan, stats, last = info[name]
    print(f'W+ step, B={B} {size}², {a.streams} stream(s), {name}: {min(v):.3f} ms per step (best of {len(v)}: {", ".join(f"{x:.3f}" for x in v)}; '
          f'{a.wsteps} steps per inversion, set-up steps included); launches per recorded step {plan["launches"]}, rollbacks {stats["rollbacks"]}, '
          f'final mean loss {last:.5f}')
base = min(res['defaults'])
for name, _ in LEGS[1:]:
    print(f'{name} costs {min(res[name]) - base:+.3f} ms per step: ratio {min(res[name]) / base:.4f}')
