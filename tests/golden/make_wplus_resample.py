#!/usr/bin/env python3
"""Generate tests/golden/wplus_resample_256.npz by RUNNING THE REAL REFERENCE (the way make_golden.py does: imported, never copied).

The W+ loop with the pixel term on an antialiased resampled view (``WPlusInverter(pixel_size=64, pixel_filter='bicubic')`` at 256², factor
4), B = 2: the reference ``Generator`` on seeded weights (``synth.generator_state(256, seed=0)``) runs 20 steps of autograd
+ ``torch.optim.Adam`` (lr 0.01) on the per-image mean of (D(G(w)) - y)^2, D = ``F.interpolate(., size=64, mode='bicubic',
antialias=True)`` — torch's own resize, not this project's tables — once with the derived target y = D(x) ('derived') and once with a
seeded 64² image given at its own size ('given': ``invert(pixel_target=)``), in float32 and, as the yardstick for how far two correct
implementations drift apart, in float64 (``G.double()``).

Stored per run: the per-image loss of every step (both precisions) and the latents after step 20 (float32 run).

    python tests/golden/make_wplus_resample.py
"""
import os
import sys

import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import make_golden as MG  # noqa: E402
from oodgan import synth  # noqa: E402

SIZE, B, STEPS, FACTOR, FILTER = 256, 2, 20, 4, 'bicubic'
RUNS = ('derived', 'given')
SEEDS = dict(weights=0, x=101, noise=102, w0=103, y=104)


def main():
    MG.install_stubs()
    torch.set_num_threads(8)
    from src.ops.StyleGAN.model import Generator
    x = synth.make_images(SIZE, B, seed=SEEDS['x'])
    noises = synth.make_noises(SIZE, B, seed=SEEDS['noise'])
    w0 = synth.make_latents(SIZE, B, seed=SEEDS['w0'], std=0.3)
    y = synth.make_images(SIZE // FACTOR, B, seed=SEEDS['y'])
    view = lambda t: F.interpolate(t, size=(SIZE // FACTOR, SIZE // FACTOR), mode=FILTER, antialias=True, align_corners=False)  # noqa: E731
    g = dict(seeds=torch.tensor([SEEDS[k] for k in ('weights', 'x', 'noise', 'w0', 'y')]), steps=torch.tensor(STEPS), factor=torch.tensor(FACTOR))
    for tag, dt in (('f32', torch.float32), ('f64', torch.float64)):
        G = Generator(SIZE, 512, 8).eval()
        G.load_state_dict(synth.generator_state(SIZE, seed=SEEDS['weights']), strict=True)
        for p in G.parameters():
            p.requires_grad_(False)
        G = G.to(dt)
        nd = [n.to(dt) for n in noises]
        for kind in RUNS:
            ys = view(x.to(dt)) if kind == 'derived' else y.to(dt)
            w = w0.to(dt).clone().requires_grad_(True)
            opt = torch.optim.Adam([w], lr=0.01, betas=(0.9, 0.999), eps=1e-8)
            losses = []
            for t in range(1, STEPS + 1):
                opt.zero_grad()
                img, _ = G(w, input_is_tensor=True, input_is_latent=True, noise=nd)
                r = view(img) - ys
                per = (r * r).mean(dim=(1, 2, 3))
                per.sum().backward()
                losses.append(per.detach().double().clone())
                opt.step()
            if tag == 'f32':
                g[f'{kind}_w_step{STEPS}'] = w.detach().float().clone()
            g[f'{kind}_losses_{tag}'] = torch.stack(losses)
            print(f'{kind} {tag}: loss step 1 {losses[0].tolist()} -> step {STEPS} {losses[-1].tolist()}', flush=True)
    for kind in RUNS:
        rel = ((g[f'{kind}_losses_f32'] - g[f'{kind}_losses_f64']).abs() / g[f'{kind}_losses_f64'].abs()).max().item()
        print(f'{kind}: reference fp32 vs float64 loss curve: max rel {rel:.2e}')
    MG.save('wplus_resample_256.npz', **g)


if __name__ == '__main__':
    main()
