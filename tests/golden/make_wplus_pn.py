#!/usr/bin/env python3
"""Generate tests/golden/wplus_pn.npz by RUNNING THE REAL REFERENCE (the way make_golden.py does: imported, never copied).

The W+ loop with the P_N+ prior (``WPlusInverter(pn_reg=...)``) at 64², B = 2: the reference ``Generator`` on seeded
weights (``synth.generator_state(64, seed=5)``) runs 20 steps of autograd + ``torch.optim.Adam`` (lr 0.01) on the per-image MSE plus
lambda * pn_b, lambda = 1e-3, in float32 and, as the yardstick for how far two correct implementations drift apart, in float64
(``G.double()``).  The statistics are tests/pn_ref.py's, float64, over n = 4096 outputs (seed 3) of the reference's own ``style`` MLP with the
relative floor 1e-4; the term is ``pn_ref.term``, through autograd.

Stored: the total loss and pn of every step (both precisions), the latents after steps 1, 10 and 20 (float32 run) and the reference's own
float32-versus-float64 distance of the loss curve.  No statistics: the test rebuilds them with ``pn_ref.stats`` from the same seeded weights.

    python tests/golden/make_wplus_pn.py
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
import pn_ref  # noqa: E402

SIZE, B, STEPS, LAMBDA = 64, 2, 20, 1e-3
STATS = dict(n=4096, seed=3, floor=1e-4)
SEEDS = dict(weights=5, x=9, noise=7, w0=14)
KEEP = (1, 10, 20)


def main():
    MG.install_stubs()
    torch.set_num_threads(8)
    from src.ops.StyleGAN.model import Generator
    x = synth.make_images(SIZE, B, seed=SEEDS['x'])
    noises = synth.make_noises(SIZE, B, seed=SEEDS['noise'])
    w0 = synth.make_latents(SIZE, B, seed=SEEDS['w0'])
    g = dict(seeds=torch.tensor([SEEDS[k] for k in ('weights', 'x', 'noise', 'w0')]), steps=torch.tensor(STEPS), pn_reg=torch.tensor(LAMBDA),
             stats_n=torch.tensor(STATS['n']), stats_seed=torch.tensor(STATS['seed']), stats_floor=torch.tensor(STATS['floor']))
    st = None
    for tag, dt in (('f32', torch.float32), ('f64', torch.float64)):
        G = Generator(SIZE, 512, 8).eval()
        G.load_state_dict(synth.generator_state(SIZE, seed=SEEDS['weights']), strict=True)
        for p in G.parameters():
            p.requires_grad_(False)
        if st is None:          # from the float32 mapping network, the one the generator ships with
            st = pn_ref.stats(G.style, 512, **STATS)
            g['stats_mean_head'] = st['mean'][:8].clone()           # a fingerprint: the test's rebuilt statistics must reproduce it
            g['stats_var_minmax'] = torch.stack([st['variance'].min(), st['variance'].max()])
        G = G.to(dt)
        xd, nd = x.to(dt), [n.to(dt) for n in noises]
        w = w0.to(dt).clone().requires_grad_(True)
        opt = torch.optim.Adam([w], lr=0.01, betas=(0.9, 0.999), eps=1e-8)
        losses, pns = [], []
        for t in range(1, STEPS + 1):
            opt.zero_grad()
            img, _ = G(w, input_is_tensor=True, input_is_latent=True, noise=nd)
            pn = pn_ref.term(w, st)
            per = ((img - xd) ** 2).mean(dim=(1, 2, 3)) + LAMBDA * pn
            per.sum().backward()
            losses.append(per.detach().double().clone())
            pns.append(pn.detach().double().clone())
            opt.step()
            if tag == 'f32' and t in KEEP:
                g[f'w_step{t}'] = w.detach().float().clone()
        g[f'losses_{tag}'], g[f'pn_{tag}'] = torch.stack(losses), torch.stack(pns)
        print(f'{tag}: loss step 1 {losses[0].tolist()} -> step {STEPS} {losses[-1].tolist()}; pn {pns[0].tolist()} -> {pns[-1].tolist()}', flush=True)
    rel = ((g['losses_f32'] - g['losses_f64']).abs() / g['losses_f64'].abs()).max()
    g['ref_f32_vs_f64'] = rel
    print(f'reference fp32 vs float64 loss curve: max rel {rel.item():.2e}')
    MG.save('wplus_pn.npz', **g)


if __name__ == '__main__':
    main()
