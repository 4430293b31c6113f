#!/usr/bin/env python3
"""Generate tests/golden/wplus_maskfit_64.npz by RUNNING THE REAL REFERENCE (the way make_golden.py does: imported, never copied).

The W+ loop with a fitted mask (``loss_region='fit'``), one image at a time at 64² with m = 16: the reference ``Generator`` on
seeded weights and the reference ``MaskLoss`` (src/losses/mask_loss.py), fed

    aligns = {m: cat(zeros(1,2,m,m), 1 - a)},  loss_func = {binary: [m], area: {str(m): A}, target: 1, binary_weight: lambda_b / lambda_a},
    loss_weight = lambda_a,

with a = sigmoid(l), beta = F.interpolate(a, size=(S,S), mode='bilinear', align_corners=False), c = x + beta*(G(w) - x) and the loss
mean (c - x)^2 + MaskLoss' two values; ``torch.optim.Adam`` with two parameter groups (w: lr 0.01; l: lr 0.1), 30 steps, in float32 and, as
the yardstick for how far two correct implementations drift apart, in float64.  Defaults of the shipped YAML: A = 0.30, lambda_a = 5.0,
lambda_b = 0.2; the start of a is 0.88.

The case: w* seeded, the start w* + 0.1 N(0,1), the target G(w*) (float64, stored as float32) with the rectangle rows 4-23, columns 20-43
(11.7 % of the area) set to the image's maximum — an occluder the generator cannot express from near w*.

Stored: the target; per precision the terms of every step (total, pixel, MaskLoss' area and binary values, mean(1 - a), mean(min(a, 1 - a))),
w_T, a_T, the means of beta_T inside and outside the rectangle, and a before the steps in ``KEEP`` (what tests/test_mask_fit_cpu.py
evaluates the yardstick's regulariser on).

    python tests/golden/make_wplus_maskfit.py
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

SIZE, M, B, STEPS = 64, 16, 2, 30
AREA, AREA_WEIGHT, BINARY_WEIGHT, LR, MASK_LR, MASK_INIT = 0.30, 5.0, 0.2, 0.01, 0.1, 0.88
RECT = (4, 24, 20, 44)        # rows [4, 24), columns [20, 44)
SEEDS = dict(weights=0, noise=112, w=113, start=114)
KEEP = (1, 10, 20, 30)


def start_latents():
    """(w*, the start w* + 0.1 N(0,1)) — what the GPU test rebuilds from the same seeds."""
    w_star = synth.make_latents(SIZE, B, seed=SEEDS['w'], std=0.3)
    return w_star, w_star + 0.1 * synth.normal('maskfit.start', tuple(w_star.shape), SEEDS['start'])


def main():
    MG.install_stubs()
    torch.set_num_threads(8)
    from src.ops.StyleGAN.model import Generator
    MaskLoss = MG._load_real('ref_mask_loss', 'src/losses/mask_loss.py').MaskLoss
    mask_loss = MaskLoss(loss_weight=AREA_WEIGHT, loss_func=dict(binary=[M], area={str(M): AREA}, target=1, binary_weight=BINARY_WEIGHT / AREA_WEIGHT))
    noises = synth.make_noises(SIZE, B, seed=SEEDS['noise'])
    w_star, w0 = start_latents()
    r0, r1, c0, c1 = RECT
    inside = torch.zeros(SIZE, SIZE, dtype=torch.bool)
    inside[r0:r1, c0:c1] = True
    g = dict(meta=torch.tensor([SIZE, M, B, STEPS]), rect=torch.tensor(RECT), keep=torch.tensor(KEEP),
             seeds=torch.tensor([SEEDS[k] for k in ('weights', 'noise', 'w', 'start')]),
             settings=torch.tensor([AREA, AREA_WEIGHT, BINARY_WEIGHT, LR, MASK_LR, MASK_INIT], dtype=torch.float64))
    x = None
    for tag, dt in (('f64', torch.float64), ('f32', torch.float32)):
        G = Generator(SIZE, 512, 8).eval()
        G.load_state_dict(synth.generator_state(SIZE, seed=SEEDS['weights']), strict=True)
        for p in G.parameters():
            p.requires_grad_(False)
        G = G.to(dt)
        if x is None:       # the target once, from the float64 generator
            with torch.no_grad():
                clean, _ = G(w_star.to(dt), input_is_tensor=True, input_is_latent=True, noise=[n.to(dt) for n in noises])
            x = clean.float().clone()
            for b in range(B):
                x[b, :, r0:r1, c0:c1] = clean[b].max().float()
            g['target'], g['clean'] = x, clean.float()
        terms = {k: torch.zeros(STEPS, B, dtype=torch.float64) for k in ('total', 'pixel', 'ml_area', 'ml_binary', 'mean_1ma', 'mean_min')}
        w_T, a_T = torch.zeros(w0.shape, dtype=torch.float64), torch.zeros(B, 1, M, M, dtype=torch.float64)
        a_kept = torch.zeros(len(KEEP), B, 1, M, M, dtype=torch.float64)
        beta_in, beta_out = torch.zeros(B, dtype=torch.float64), torch.zeros(B, dtype=torch.float64)
        for b in range(B):
            xd, nd = x[b:b + 1].to(dt), [n[b:b + 1].to(dt) for n in noises]
            w = w0[b:b + 1].to(dt).clone().requires_grad_(True)
            a0 = torch.full((1, 1, M, M), MASK_INIT, dtype=dt).clamp(1e-3, 1 - 1e-3)
            l = torch.log(a0 / (1 - a0)).requires_grad_(True)
            opt = torch.optim.Adam([dict(params=[w], lr=LR), dict(params=[l], lr=MASK_LR)], betas=(0.9, 0.999), eps=1e-8)
            for t in range(1, STEPS + 1):
                opt.zero_grad()
                a = torch.sigmoid(l)
                if t in KEEP:
                    a_kept[KEEP.index(t), b] = a.detach().double()[0]
                beta = F.interpolate(a, size=(SIZE, SIZE), mode='bilinear', align_corners=False)
                img, _ = G(w, input_is_tensor=True, input_is_latent=True, noise=nd)
                c = xd + beta * (img - xd)
                pix = ((c - xd) ** 2).mean()
                ml_bin, ml_area = mask_loss({M: torch.cat([torch.zeros(1, 2, M, M, dtype=dt), 1 - a], 1)})
                tot = pix + ml_bin + ml_area
                tot.backward()
                for k, v in (('total', tot), ('pixel', pix), ('ml_area', ml_area), ('ml_binary', ml_bin), ('mean_1ma', (1 - a).mean()),
                             ('mean_min', torch.minimum(a, 1 - a).mean())):
                    terms[k][t - 1, b] = v.detach().double()
                opt.step()
            with torch.no_grad():
                a = torch.sigmoid(l)
                beta = F.interpolate(a, size=(SIZE, SIZE), mode='bilinear', align_corners=False)[0, 0].double()
            w_T[b], a_T[b] = w.detach().double()[0], a.detach().double()[0]
            beta_in[b], beta_out[b] = beta[inside].mean(), beta[~inside].mean()
            print(f'image {b} {tag}: total step 1 {terms["total"][0, b].item():.6f} -> step {STEPS} {terms["total"][-1, b].item():.6f}; beta inside '
                  f'{beta_in[b].item():.3f} outside {beta_out[b].item():.3f}; mean(1 - a) {1 - a.mean().item():.3f}', flush=True)
        for k, v in terms.items():
            g[f'{k}_{tag}'] = v
        g[f'w_T_{tag}'], g[f'a_T_{tag}'], g[f'a_kept_{tag}'] = (w_T.float() if tag == 'f32' else w_T), a_T, a_kept
        g[f'beta_in_{tag}'], g[f'beta_out_{tag}'] = beta_in, beta_out
    for k in ('total', 'pixel', 'ml_area', 'ml_binary'):
        d = (g[f'{k}_f32'] - g[f'{k}_f64']).abs()
        print(f'reference fp32 vs float64, {k}: max abs {d.max().item():.3e}, max rel {(d / g[k + "_f64"].abs().clamp_min(1e-30)).max().item():.3e}')
    print(f'reference fp32 vs float64, a_T: max abs {(g["a_T_f32"] - g["a_T_f64"]).abs().max().item():.3e}')
    MG.save('wplus_maskfit_64.npz', **g)


if __name__ == '__main__':
    main()
