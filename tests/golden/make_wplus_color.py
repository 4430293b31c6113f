#!/usr/bin/env python3
"""Generate tests/golden/wplus_color_64.npz by RUNNING THE REAL REFERENCE (the way make_golden.py does: imported, never copied).

The W+ loop with a colour map of the generator image fitted beside the latents (``WPlusInverter(color='affine' | 'gain')`` at 64², B = 2;
DESIGN.md §26): the reference ``Generator`` on seeded weights (``synth.generator_state(64, seed=SEEDS['weights'])``) runs 10 steps of autograd +
``torch.optim.Adam`` on [w, theta] (two groups: lr 0.01 and COLOR_LR, betas (0.9, 0.999), eps 1e-8) on the per-image mean of
(C_theta(G(w)) - x)^2, C_theta(G)_i = sum_j M_ij G_j + b_i written as an einsum, from the identity, in float32 and, as the yardstick for
how far two correct implementations drift apart, in float64 (``G.double()``); once with all 12 numbers free ('affine') and once with the
gradient of the off-diagonal numbers of M masked ('gain').  The photograph x is the image of seeded latents w*, mapped by THETA_STAR
(float64, stored as float32): the run has a colour cast to remove.

10 steps, not 20: at 20 steps (and from a start closer than 0.1) the float32 run of the reference itself drifts up to 1e-3 from its
float64 run, the bar the loop is held to; at 10 it stays under a quarter of it.  The script prints both drifts and refuses to save when
the loss drift exceeds 2.5e-4.

Stored: x; per kind and step the per-image loss and theta after the step (both precisions); the latents after the last step (both).

    python tests/golden/make_wplus_color.py
"""
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import make_golden as MG  # noqa: E402
from oodgan import synth  # noqa: E402

SIZE, B, STEPS, LR, COLOR_LR = 64, 2, 10, 0.01, 0.005
SEEDS = dict(weights=3, noise=112, w_star=113, start=114)
THETA_STAR = [[1.15, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.85, 0.05, 0.0, -0.05],
              [0.80, 0.15, 0.05, 0.10, 0.75, 0.05, 0.05, 0.10, 0.60, -0.04, 0.02, 0.06]]
IDENTITY = [1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0]
FREE = dict(affine=[1.0] * 12, gain=[1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0, 1.0, 1.0, 1.0])
DRIFT_MAX = 2.5e-4


def color_map(img, theta):
    return torch.einsum('bij,bjhw->bihw', theta[:, :9].reshape(-1, 3, 3), img) + theta[:, 9:].reshape(-1, 3, 1, 1)


def main():
    MG.install_stubs()
    torch.set_num_threads(8)
    from src.ops.StyleGAN.model import Generator
    noises = synth.make_noises(SIZE, B, seed=SEEDS['noise'])
    w_star = synth.make_latents(SIZE, B, seed=SEEDS['w_star'], std=0.3)
    w0 = w_star + 0.1 * synth.normal('color.start', tuple(w_star.shape), SEEDS['start'])
    g = dict(meta=torch.tensor([SIZE, B, STEPS]), seeds=torch.tensor([SEEDS[k] for k in ('weights', 'noise', 'w_star', 'start')]),
             settings=torch.tensor([LR, COLOR_LR], dtype=torch.float64), theta_star=torch.tensor(THETA_STAR, dtype=torch.float64))
    x, worst = None, 0.0
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
                x = color_map(img, torch.tensor(THETA_STAR, dtype=dt)).float()
            g['target'] = x.clone()
        for kind, free in FREE.items():
            w = w0.to(dt).clone().requires_grad_(True)
            th = torch.tensor([IDENTITY] * B, dtype=dt, requires_grad=True)
            mask = torch.tensor(free, dtype=dt)
            opt = torch.optim.Adam([dict(params=[w], lr=LR), dict(params=[th], lr=COLOR_LR)], betas=(0.9, 0.999), eps=1e-8)
            losses, thetas = [], []
            for t in range(1, STEPS + 1):
                opt.zero_grad()
                img, _ = G(w, input_is_tensor=True, input_is_latent=True, noise=nd)
                r = color_map(img, th) - x.to(dt)
                per = (r * r).mean(dim=(1, 2, 3))
                per.sum().backward()
                th.grad.mul_(mask)          # a number that is not free has gradient 0: Adam leaves it where it is
                losses.append(per.detach().double().clone())
                opt.step()
                thetas.append(th.detach().double().clone())
            g[f'{kind}_losses_{tag}'], g[f'{kind}_theta_{tag}'] = torch.stack(losses), torch.stack(thetas)
            g[f'{kind}_w_T_{tag}'] = w.detach().clone() if tag == 'f64' else w.detach().float().clone()
            print(f'{tag} {kind}: loss step 1 {losses[0].tolist()} -> step {STEPS} {losses[-1].tolist()}; theta_T {thetas[-1].tolist()}', flush=True)
    for kind in FREE:
        rel = ((g[f'{kind}_losses_f32'] - g[f'{kind}_losses_f64']).abs() / g[f'{kind}_losses_f64'].abs()).max().item()
        gap = (g[f'{kind}_theta_f32'] - g[f'{kind}_theta_f64']).abs().max().item()
        worst = max(worst, rel)
        print(f'{kind}: reference fp32 vs float64: loss curve max rel {rel:.2e} (a quarter of the bar 1e-3: {DRIFT_MAX:.1e}), theta max |diff| {gap:.2e}')
    if worst > DRIFT_MAX:
        sys.exit(f'the loss drift {worst:.2e} exceeds {DRIFT_MAX:.1e}: not saved')
    MG.save('wplus_color_64.npz', **g)


if __name__ == '__main__':
    main()
