#!/usr/bin/env python3
"""Generate tests/golden/wplus_sspace_256.npz by RUNNING THE REAL REFERENCE (the way make_golden.py does: imported, never copied).

The StyleSpace loop (``WPlusInverter(latent_space='s')``) at 256², two images, one at a time: the reference ``Generator`` on
seeded weights (``synth.generator_state(256, seed=0)``) at fixed W+ latents w0, with an offset delta (R,) added to its
``<layer>.conv.modulation.bias`` parameters — ModulatedConv2d computes its style as modulation(w) = scale * W w + bias, so the offset on a
bias IS the offset on that layer's style, for the one image of the batch.  20 steps of autograd + ``torch.optim.Adam`` (lr 0.01) on delta,
from 0, on the per-image MSE, in float32 and, as the yardstick for how far two correct implementations drift apart, in float64
(``G.double()``).  The rows of delta follow the generator's execution order (conv1, to_rgb1, convs.0, convs.1, to_rgbs.0, ...).

Stored: the per-image loss of every step (both precisions) and delta after steps 1, 5 and 20 as float32 (both precisions).

    python tests/golden/make_wplus_sspace.py
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

SIZE, B, STEPS, KEEP = 256, 2, 20, (1, 5, 20)
SEEDS = dict(weights=0, x=81, noise=82, w0=83)


def layer_names(size):
    n = ['conv1', 'to_rgb1']
    for j in range(size.bit_length() - 3):
        n += [f'convs.{2 * j}', f'convs.{2 * j + 1}', f'to_rgbs.{j}']
    return n


def main():
    MG.install_stubs()
    torch.set_num_threads(8)
    from torch.func import functional_call
    from src.ops.StyleGAN.model import Generator
    x = synth.make_images(SIZE, B, seed=SEEDS['x'])
    noises = synth.make_noises(SIZE, B, seed=SEEDS['noise'])
    w0 = synth.make_latents(SIZE, B, seed=SEEDS['w0'], std=0.3)
    g = dict(seeds=torch.tensor([SEEDS[k] for k in ('weights', 'x', 'noise', 'w0')]), steps=torch.tensor(STEPS), keep=torch.tensor(KEEP))
    for tag, dt in (('f32', torch.float32), ('f64', torch.float64)):
        G = Generator(SIZE, 512, 8).eval()
        G.load_state_dict(synth.generator_state(SIZE, seed=SEEDS['weights']), strict=True)
        for p in G.parameters():
            p.requires_grad_(False)
        G = G.to(dt)
        sd = dict(G.named_parameters())
        keys = [f'{n}.conv.modulation.bias' for n in layer_names(SIZE)]
        rows, r = [], 0
        for k in keys:
            rows.append((k, r, sd[k].numel()))
            r += sd[k].numel()
        losses = torch.zeros(STEPS, B, dtype=torch.float64)
        kept = {t: torch.zeros(B, r) for t in KEEP}
        for b in range(B):
            xd, nd, wd = x[b:b + 1].to(dt), [n[b:b + 1].to(dt) for n in noises], w0[b:b + 1].to(dt)
            delta = torch.zeros(r, dtype=dt, requires_grad=True)
            opt = torch.optim.Adam([delta], lr=0.01, betas=(0.9, 0.999), eps=1e-8)
            for t in range(1, STEPS + 1):
                opt.zero_grad()
                over = {k: sd[k] + delta[r0:r0 + n] for k, r0, n in rows}
                img, _ = functional_call(G, over, (wd,), dict(input_is_tensor=True, input_is_latent=True, noise=nd))
                per = ((img - xd) ** 2).mean(dim=(1, 2, 3))
                per.sum().backward()
                losses[t - 1, b] = per.detach().double()[0]
                opt.step()
                if t in kept:
                    kept[t][b] = delta.detach().float()
            print(f'image {b} {tag}: loss step 1 {losses[0, b].item():.6f} -> step {STEPS} {losses[-1, b].item():.6f}, max |delta| {delta.detach().abs().max().item():.3e}', flush=True)
        g[f'losses_{tag}'] = losses
        for t in KEEP:
            g[f'delta_step{t}_{tag}'] = kept[t]
    rel = ((g['losses_f32'] - g['losses_f64']).abs() / g['losses_f64'].abs()).max().item()
    print(f'reference fp32 vs float64 loss curve: max rel {rel:.2e}')
    MG.save('wplus_sspace_256.npz', **g)


if __name__ == '__main__':
    main()
