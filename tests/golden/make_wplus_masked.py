#!/usr/bin/env python3
"""Generate tests/golden/wplus_masked_256.npz by RUNNING THE REAL REFERENCE (the way make_golden.py does: imported, never copied).

The masked W+ objective of ``ood_faceGAN_e4e.invert(loss_region='blend')`` at 256², the smallest size at which the four
SAMM levels (32²..256²) are hooked:

1. the reference ``ood_faceGAN_e4e`` on seeded weights (``synth.ood_state(256, seed=41)``) runs its OOD forward at the start latents, with
   a stand-in encoder that returns recipe tensors and preset noise maps (``gold_ood`` of make_golden.py is the model); alpha0 is the mask
   its ``blending_mask`` stored, beta = (1 - alpha0)^blend_cnt (blend_cnt = 1);
2. the reference ``Generator`` (the model's own) then runs 20 steps of autograd + ``torch.optim.Adam`` (lr 0.01) from the start latents
   on the composite loss mean((beta * (G(w) - x))^2) per image, with the same noise maps — in float32 and, as the yardstick for how far
   two correct implementations drift apart, in float64 (``G.double()``; beta from the float32 forward in both).

Stored: beta sub-sampled ::4, its per-image mean, the start latents, the per-image loss of every step (both precisions), the latents
after steps 5 and 20 (float32 run).

    python tests/golden/make_wplus_masked.py
"""
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, HERE)

import make_golden as MG  # noqa: E402
from oodgan import synth  # noqa: E402

SIZE, B, STEPS = 256, 2, 20
SEEDS = dict(weights=41, enc_lats=42, enc_feats=43, x=44, noise=45)


def main():
    MG.install_stubs()
    torch.set_num_threads(8)
    from src.archs.OOD_faceGAN_e4e_arch import ood_faceGAN_e4e
    m = ood_faceGAN_e4e(out_size=SIZE, style_dim=512, encoder='E4E', enable_modulation=True, warp_scale=0.08, cycle_align=2,
                        blend_with_gen=True, ModSize=256).eval()
    # the reference sizes delta_latent for 1024² whatever out_size is (18 rows, OOD_faceGAN_e4e_arch.py:126-129; its latents have 14 here)
    m.delta_latent = torch.nn.Parameter(torch.zeros(1, m.style_cnt, 512), requires_grad=False)
    res = m.load_state_dict(synth.ood_state(SIZE, seed=SEEDS['weights']), strict=False)
    assert not res.unexpected_keys, res.unexpected_keys
    assert all(k.startswith('encoder.') for k in res.missing_keys)
    enc_lats = synth.make_latents(SIZE, B, seed=SEEDS['enc_lats'], std=0.3)
    enc_feats = synth.make_encoder_feats(B, seed=SEEDS['enc_feats'])

    class FakeEncoder(torch.nn.Module):
        channels = [64, 64, 128, 256, 512]

        def forward(self, x, return_feats=False):
            return enc_lats.clone(), [f.clone() for f in enc_feats] + [None]

    fe = FakeEncoder()
    fe.progressive_stage = m.encoder.progressive_stage
    m.encoder = fe
    x = synth.make_images(SIZE, B, seed=SEEDS['x'])
    noises = synth.make_noises(SIZE, B, seed=SEEDS['noise'])
    feed = MG._NoiseFeed(noises)
    feed.install()
    torch.manual_seed(1234)
    with torch.no_grad():
        _, lats = m(x)
    feed.remove()
    assert feed.calls == len(noises), feed.calls
    # blending_mask stores the composed, clipped mask under the key 1024 at every output size (OOD_faceGAN_e4e_arch.py:315-339)
    alpha = m.aligns[1024][:, :1].clone()
    assert alpha.shape == (B, 1, SIZE, SIZE), alpha.shape
    beta = (1.0 - alpha) ** m.blend_cnt
    print(f'beta: mean per image {beta.mean(dim=(1, 2, 3)).tolist()}, min {beta.min().item():.3f}, max {beta.max().item():.3f}')
    g = dict(seeds=torch.tensor([SEEDS[k] for k in ('weights', 'enc_lats', 'enc_feats', 'x', 'noise')]), steps=torch.tensor(STEPS),
             beta_sub=beta[:, :, ::4, ::4], beta_mean=beta.double().mean(dim=(1, 2, 3)), w0=lats)
    G = m.generator
    for p in G.parameters():
        p.requires_grad_(False)
    for tag, dt in (('f32', torch.float32), ('f64', torch.float64)):
        Gd = G.to(dt)
        xd, bd, nd = x.to(dt), beta.to(dt), [n.to(dt) for n in noises]
        w = lats.detach().to(dt).clone().requires_grad_(True)
        opt = torch.optim.Adam([w], lr=0.01, betas=(0.9, 0.999), eps=1e-8)
        losses = []
        for t in range(1, STEPS + 1):
            opt.zero_grad()
            img, _ = Gd(w, input_is_tensor=True, input_is_latent=True, noise=nd)
            per = ((bd * (img - xd)) ** 2).mean(dim=(1, 2, 3))
            per.sum().backward()
            losses.append(per.detach().double().clone())
            opt.step()
            if tag == 'f32' and t in (5, 20):
                g[f'w_step{t}'] = w.detach().float().clone()
        g[f'losses_{tag}'] = torch.stack(losses)
        print(f'{tag}: loss step 1 {losses[0].tolist()} -> step {STEPS} {losses[-1].tolist()}', flush=True)
    rel = ((g['losses_f32'] - g['losses_f64']).abs() / g['losses_f64'].abs()).max().item()
    print(f'reference fp32 vs float64 loss curve: max rel {rel:.2e}')
    MG.save('wplus_masked_256.npz', **g)


if __name__ == '__main__':
    main()
