#!/usr/bin/env python3
"""Generate tests/golden/wplus_fspace.npz by RUNNING THE REAL REFERENCE (the way make_golden.py does: imported, never copied).

The F/W+ loop (``WPlusInverter(feature_layer=l)``), one image at a time: the reference ``Generator`` on seeded weights
(``synth.generator_state(size, seed=0)``), a ``register_forward_pre_hook`` on ``G.convs[l - 1]`` — the styled up-conv that reads latent l —
that adds a leaf delta (1, C, h, h) to the module's input, and ``torch.optim.Adam`` with two parameter groups (w: lr 0.01, delta: lr 0.01),
both from their start (w0, 0), on the per-image MSE; in float32 and, as the yardstick for how far two correct implementations drift apart,
in float64 (``G.double()``).

Cases: 256², l = 5, two images, 20 steps; 64², l = 3 and l = 7, two images, 12 steps.  Stored per case and precision: the per-image loss of
every step; w after steps 1, 5 and the last; of delta a fixed strided subsample, [:, ::16, ::2, ::2], after the last step, and ||delta||_2
per image after every kept step.

    python tests/golden/make_wplus_fspace.py
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

B = 2
CASES = (('s256_l5', 256, 5, 20), ('s64_l3', 64, 3, 12), ('s64_l7', 64, 7, 12))
SEEDS = dict(weights=0, x=91, noise=92, w0=93)
SUB = (slice(None), slice(None, None, 16), slice(None, None, 2), slice(None, None, 2))


def main():
    MG.install_stubs()
    torch.set_num_threads(8)
    from src.ops.StyleGAN.model import Generator
    g = dict(seeds=torch.tensor([SEEDS[k] for k in ('weights', 'x', 'noise', 'w0')]))
    for name, size, l, steps in CASES:
        keep = (1, 5, steps)
        x = synth.make_images(size, B, seed=SEEDS['x'])
        noises = synth.make_noises(size, B, seed=SEEDS['noise'])
        w0 = synth.make_latents(size, B, seed=SEEDS['w0'], std=0.3)
        g[f'{name}_meta'] = torch.tensor([size, l, steps])
        g[f'{name}_keep'] = torch.tensor(keep)
        for tag, dt in (('f32', torch.float32), ('f64', torch.float64)):
            G = Generator(size, 512, 8).eval()
            G.load_state_dict(synth.generator_state(size, seed=SEEDS['weights']), strict=True)
            for p in G.parameters():
                p.requires_grad_(False)
            G = G.to(dt)
            leaf = {}
            handle = G.convs[l - 1].register_forward_pre_hook(lambda mod, args: (args[0] + leaf['delta'],) + tuple(args[1:]))
            losses = torch.zeros(steps, B, dtype=torch.float64)
            kept_w = {t: torch.zeros_like(w0) for t in keep}
            norms = torch.zeros(len(keep), B, dtype=torch.float64)
            sub = None
            for b in range(B):
                xd, nd = x[b:b + 1].to(dt), [n[b:b + 1].to(dt) for n in noises]
                w = w0[b:b + 1].to(dt).clone().requires_grad_(True)
                with torch.no_grad():       # the shape of the hooked module's input, from one plain pass
                    seen = {}
                    probe = G.convs[l - 1].register_forward_pre_hook(lambda mod, args: seen.update(shape=tuple(args[0].shape)))
                    leaf['delta'] = 0.0
                    G(w, input_is_tensor=True, input_is_latent=True, noise=nd)
                    probe.remove()
                delta = torch.zeros(seen['shape'], dtype=dt, requires_grad=True)
                leaf['delta'] = delta
                opt = torch.optim.Adam([dict(params=[w], lr=0.01), dict(params=[delta], lr=0.01)], betas=(0.9, 0.999), eps=1e-8)
                for t in range(1, steps + 1):
                    opt.zero_grad()
                    img, _ = G(w, input_is_tensor=True, input_is_latent=True, noise=nd)
                    per = ((img - xd) ** 2).mean(dim=(1, 2, 3))
                    per.sum().backward()
                    losses[t - 1, b] = per.detach().double()[0]
                    opt.step()
                    if t in kept_w:
                        kept_w[t][b] = w.detach().float()[0]
                        norms[keep.index(t), b] = delta.detach().double().norm()
                d = delta.detach().float()
                sub = torch.zeros((B,) + tuple(d[SUB].shape[1:])) if sub is None else sub
                sub[b] = d[SUB][0]
                print(f'{name} image {b} {tag}: delta {tuple(d.shape)}, loss step 1 {losses[0, b].item():.6f} -> step {steps} {losses[-1, b].item():.6f}, '
                      f'max |delta| {d.abs().max().item():.3e}, ||delta|| {norms[-1, b].item():.4f}', flush=True)
            handle.remove()
            g[f'{name}_losses_{tag}'] = losses
            for t in keep:
                g[f'{name}_w_step{t}_{tag}'] = kept_w[t]
            g[f'{name}_delta_sub_{tag}'] = sub
            g[f'{name}_delta_norm_{tag}'] = norms
        rel = ((g[f'{name}_losses_f32'] - g[f'{name}_losses_f64']).abs() / g[f'{name}_losses_f64'].abs()).max().item()
        print(f'{name}: reference fp32 vs float64 loss curve: max rel {rel:.2e}', flush=True)
    MG.save('wplus_fspace.npz', **g)


if __name__ == '__main__':
    main()
