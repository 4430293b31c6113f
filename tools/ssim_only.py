"""The SSIM loss term alone (B=8, 1024²): ms per call of the fused forward + backward kernel (device events; forward-only as well) and
the achieved share of its byte model, then a W+ step with and without the term (plain MSE loop, launch plans, one stream; the two
alternated in one process).  profiles/ssim_term.txt; under rocprofv3 --kernel-trace the per-kernel split.
    python tools/ssim_only.py [--batch 8] [--size 1024] [--wsteps 40] [--reps 3] [--no-step]"""
import argparse, os, sys, time
R_ = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(R_, 'ood-gan-inversion_amd'))
import torch
from oodgan import ops, synth
from oodgan.engine import GeneratorEngine, WPlusInverter

ap = argparse.ArgumentParser()
ap.add_argument('--batch', type=int, default=8)
ap.add_argument('--size', type=int, default=1024)
ap.add_argument('--wsteps', type=int, default=40)
ap.add_argument('--reps', type=int, default=3)
ap.add_argument('--ssim-weight', type=float, default=0.5)
ap.add_argument('--no-step', action='store_true', help='kernels only')
a = ap.parse_args()
if not a.ssim_weight > 0:
    ap.error('--ssim-weight must be > 0: the step is timed with the term against without it')
B, size, dev = a.batch, a.size, torch.device('cuda:0')
target = torch.cat([synth.make_images(size, 1, seed=1000 + i) for i in range(B)]).to(dev)
pred = torch.cat([synth.make_images(size, 1, seed=5000 + i) for i in range(B)]).to(dev)
gimg = torch.zeros_like(pred)


def timed(fn, n=50):
    for _ in range(5):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


ms = timed(lambda: ops.ssim_loss_grad(pred, target, gimg, 4.0))
ms_f = timed(lambda: ops.ssim_loss_grad(pred, target))
nbytes = 4 * pred.numel() * 4           # G and x read, gimg read and written
print(f'SSIM forward + backward to the image, B={B} {size}²: {ms:.3f} ms per call ({nbytes / 1e6:.0f} MB by the fused byte model = '
      f'{nbytes / ms / 1e9:.2f} TB/s); forward only {ms_f:.3f} ms; 1 - SSIM = {ops.ssim_loss_grad(pred, target).tolist()}')
if not a.no_step:
    eng = GeneratorEngine({k: v.to(dev) for k, v in synth.generator_state(size, seed=0).items()}, size, precision='f16s-g2')
    noises = [n.to(dev) for n in synth.make_noises(size, B, seed=7)]
    w0 = synth.make_latents(size, B, seed=14, std=0.3).to(dev)
    res, launches = {0.0: [], a.ssim_weight: []}, {}
    for rep in range(a.reps + 1):          # the first round warms both up
        for lam in res:
            inv = WPlusInverter(eng, ssim_weight=lam)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            inv.invert(target, w0, noises, steps=a.wsteps)
            torch.cuda.synchronize()
            launches[lam] = inv.last_plan['launches']
            if rep:
                res[lam].append((time.perf_counter() - t0) * 1e3 / a.wsteps)
    for lam, v in res.items():
        print(f'W+ step, B={B} {size}², ssim_weight {lam:g}: {min(v):.3f} ms per step (best of {len(v)}: {", ".join(f"{x:.3f}" for x in v)}; '
              f'{a.wsteps} steps per inversion, set-up steps included); launches per recorded step {launches[lam]}')
    print(f'the term costs {min(res[a.ssim_weight]) - min(res[0.0]):.3f} ms per step')
