"""What the P_N+ prior costs per W+ step: the same inversion (1024², B=8, 100 steps, two streams, precision 'f16s-g2',
launch plans) with pn_reg on against off, the legs interleaved in one process after a warm-up inversion of each, best of --reps; wall time
per inversion between device synchronisations.  Then the kernel pair alone (oodgan_pn_prior_fwd_bwd_row: the row kernel and the finish
kernel) at the loop's shapes, from HIP events around --calls back-to-back calls.  The statistics are synthetic (tests/pn_ref.py's maker
restated: a seeded orthogonal basis, variances log-spaced over 1e-7 ... 1e2): their values do not change what the kernels do.
profiles/pn_prior_cost.txt.
    python tools/pn_prior_cost.py [--batch 8] [--size 1024] [--wsteps 100] [--streams 2] [--reps 3] [--calls 200]"""
import argparse, os, sys, time
R_ = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(R_, 'ood-gan-inversion_amd'))
import torch
from oodgan import ops, synth
from oodgan.engine import GeneratorEngine, WPlusInverter
from oodgan.pn import PNStats

ap = argparse.ArgumentParser()
ap.add_argument('--batch', type=int, default=8)
ap.add_argument('--size', type=int, default=1024)
ap.add_argument('--wsteps', type=int, default=100)
ap.add_argument('--streams', type=int, default=2)
ap.add_argument('--reps', type=int, default=3)
ap.add_argument('--calls', type=int, default=200)
a = ap.parse_args()
B, size, dev, D = a.batch, a.size, torch.device('cuda:0'), 512
eng = GeneratorEngine({k: v.to(dev) for k, v in synth.generator_state(size, seed=0).items()}, size, precision='f16s-g2')
target = torch.cat([synth.make_images(size, 1, seed=1000 + i) for i in range(B)]).to(dev)
noises = [n.to(dev) for n in synth.make_noises(size, B, seed=7)]
w0 = synth.make_latents(size, B, seed=14, std=0.3).to(dev)
gen = torch.Generator().manual_seed(0)
comp, _ = torch.linalg.qr(torch.randn(D, D, generator=gen, dtype=torch.float64))
st = PNStats(torch.randn(D, generator=gen, dtype=torch.float64), comp, torch.logspace(-7, 2, D, dtype=torch.float64), 0, 0, 0.0, dev)
res, info = {'off': [], 'on': []}, {}
for rep in range(a.reps + 1):          # the first round warms both up
    for name, kw in (('off', {}), ('on', dict(pn_reg=1e-6))):
        inv = WPlusInverter(eng, **kw)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        _, losses = inv.invert(target, w0, noises, steps=a.wsteps, streams=a.streams, pn_stats=st if kw else None)
        torch.cuda.synchronize()
        info[name] = (inv.last_plan, inv.last_stats, losses[-1].mean().item())
        if rep:
            res[name].append((time.perf_counter() - t0) * 1e3 / a.wsteps)
for name, v in res.items():
    plan, stats, last = info[name]
    print(f'W+ step, B={B} {size}², {a.streams} streams, pn_reg {name}: {min(v):.3f} ms per step (best of {len(v)}: {", ".join(f"{x:.3f}" for x in v)}; '
          f'{a.wsteps} steps per inversion, set-up steps included); launches per recorded step {plan["launches"]}, rollbacks {stats["rollbacks"]}, '
          f'final mean loss {last:.5f}')
spread = max(max(v) - min(v) for v in res.values())
print(f'the prior costs {min(res["on"]) - min(res["off"]):.3f} ms per step: ratio {min(res["on"]) / min(res["off"]):.4f} (largest spread of the repeats of one leg: {spread:.3f} ms)')
# the kernel pair alone: one sub-batch of the loop (B / streams images) and the whole batch, alone on the GPU
for b in sorted({max(1, B // a.streams), B}):
    w, g = w0[:b].contiguous(), torch.zeros_like(w0[:b])
    table, row, part = torch.zeros(4, b, device=dev), torch.zeros(1, dtype=torch.int32, device=dev), ops.pn_prior_parts(b, w.shape[1], dev)
    best = float('inf')
    for rep in range(a.reps + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.calls):
            ops.pn_prior_loss_grad(w, st.mean, st.matrix, g, 1e-6, table=table, row_dev=row, part=part)
        e1.record()
        torch.cuda.synchronize()
        if rep:
            best = min(best, e0.elapsed_time(e1) * 1e3 / a.calls)
    print(f'kernel pair alone, ({b}, {w.shape[1]}, {D}): {best:.1f} us per call (HIP events around {a.calls} back-to-back calls, best of {a.reps}); '
          f'{100 * best * 1e-3 * (B // b) / min(res["off"]):.3f} % of the step with pn_reg off for the batch of {B}')
