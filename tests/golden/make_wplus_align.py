#!/usr/bin/env python3
"""Generate tests/golden/wplus_align_64.npz by RUNNING THE REAL REFERENCE (the way make_golden.py does: imported, never copied).

The W+ loop with a similarity alignment of the target fitted beside the latents (``WPlusInverter(align='similarity')`` at 64², B = 2;
DESIGN.md §25): the reference ``Generator`` on seeded weights (``synth.generator_state(64, seed=SEEDS['weights'])``) runs 20 steps of autograd +
``torch.optim.Adam`` on [w, theta] (two groups: lr 0.01 and ALIGN_LR, betas (0.9, 0.999), eps 1e-8) on the per-image mean of
(G(w) - x_theta)^2, x_theta = ``F.grid_sample(x, F.affine_grid([[a, -s, tx], [s, a, ty]], align_corners=False), mode='bicubic',
padding_mode='border', align_corners=False)`` — torch's own resampler, not this project's formula —, from theta = 0, in float32 and, as
the yardstick for how far two correct implementations drift apart, in float64 (``G.double()``).  The photograph x is the image of seeded
latents w*, warped by THETA_STAR with the same call (float64, stored as float32): the run has a registration error to remove.

Stored: x; per step the per-image loss and theta after the step (both precisions); the latents after step 20 (both).

    python tests/golden/make_wplus_align.py
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

SIZE, B, STEPS, LR, ALIGN_LR = 64, 2, 20, 0.01, 0.002
SEEDS = dict(weights=3, noise=112, w_star=113, start=114)
THETA_STAR = [[0.03, 0.05, 0.04, -0.03], [-0.04, -0.03, -0.05, 0.02]]


def warp(x, theta):
    e = torch.exp(theta[:, 0])
    a, s = e * torch.cos(theta[:, 1]), e * torch.sin(theta[:, 1])
    mat = torch.stack([torch.stack([a, -s, theta[:, 2]], 1), torch.stack([s, a, theta[:, 3]], 1)], 1)
    return F.grid_sample(x, F.affine_grid(mat, list(x.shape), align_corners=False), mode='bicubic', padding_mode='border', align_corners=False)


def main():
    MG.install_stubs()
    torch.set_num_threads(8)
    from src.ops.StyleGAN.model import Generator
    noises = synth.make_noises(SIZE, B, seed=SEEDS['noise'])
    w_star = synth.make_latents(SIZE, B, seed=SEEDS['w_star'], std=0.3)
    w0 = w_star + 0.1 * synth.normal('align.start', tuple(w_star.shape), SEEDS['start'])
    g = dict(meta=torch.tensor([SIZE, B, STEPS]), seeds=torch.tensor([SEEDS[k] for k in ('weights', 'noise', 'w_star', 'start')]),
             settings=torch.tensor([LR, ALIGN_LR], dtype=torch.float64), theta_star=torch.tensor(THETA_STAR, dtype=torch.float64))
    x = None
    for tag, dt in (('f64', torch.float64), ('f32', torch.float32)):
        G = Generator(SIZE, 512, 8).eval()
        G.load_state_dict(synth.generator_state(SIZE, seed=SEEDS['weights']), strict=True)
        for p in G.parameters():
            p.requires_grad_(False)
        G = G.to(dt)
        nd = [n.to(dt) for n in noises]
        if x is None:       # the photograph, once, in float64
            with torch.no_grad():
                img, _ = G(w_star.to(dt), input_is_tensor=True, input_is_latent=True, noise=nd)
                x = warp(img, torch.tensor(THETA_STAR, dtype=dt)).float()
            g['target'] = x.clone()
        w = w0.to(dt).clone().requires_grad_(True)
        th = torch.zeros(B, 4, dtype=dt, requires_grad=True)
        opt = torch.optim.Adam([dict(params=[w], lr=LR), dict(params=[th], lr=ALIGN_LR)], betas=(0.9, 0.999), eps=1e-8)
        losses, thetas = [], []
        for t in range(1, STEPS + 1):
            opt.zero_grad()
            img, _ = G(w, input_is_tensor=True, input_is_latent=True, noise=nd)
            r = img - warp(x.to(dt), th)
            per = (r * r).mean(dim=(1, 2, 3))
            per.sum().backward()
            losses.append(per.detach().double().clone())
            opt.step()
            thetas.append(th.detach().double().clone())
        g[f'losses_{tag}'], g[f'theta_{tag}'] = torch.stack(losses), torch.stack(thetas)
        g[f'w_T_{tag}'] = w.detach().clone() if tag == 'f64' else w.detach().float().clone()
        print(f'{tag}: loss step 1 {losses[0].tolist()} -> step {STEPS} {losses[-1].tolist()}; theta_T {thetas[-1].tolist()}', flush=True)
    rel = ((g['losses_f32'] - g['losses_f64']).abs() / g['losses_f64'].abs()).max().item()
    gap = (g['theta_f32'] - g['theta_f64']).abs().max().item()
    print(f'reference fp32 vs float64: loss curve max rel {rel:.2e} (a quarter of the bar 1e-3: 2.5e-4), theta max |diff| {gap:.2e}')
    MG.save('wplus_align_64.npz', **g)


if __name__ == '__main__':
    main()
