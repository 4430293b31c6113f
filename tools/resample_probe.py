#!/usr/bin/env python3
"""Cost of the pixel term on an antialiased resampled view (csrc/loss_resample.hip) against the kernel it sits beside, what
a user would otherwise write, and the byte floor, in ONE process on one GPU.

Kernels, at B=8, 1024² (the bench geometry), after a warm-up, timed with HIP events over --launches calls per window, the variants
interleaved over --rounds windows each (a drift of the clock hits every variant alike); median with min .. max per call:
    resampled_<filter>_f<F>     oodgan_resampled_pixel_loss_fwd_bwd_row: kernel one, the finish, kernel two — as the W+ step issues them —
                                for bilinear, bicubic and lanczos3 at F in {2, 4, 8, 16}
    box_f<F>                    (a) oodgan_pooled_pixel_loss_fwd_bwd_row, the fused box kernel of §20 at the same F (+ its finish)
    torch_<filter>_f<F>         (b) torch on the same GPU: F.interpolate(G, antialias=True) -> mean((. - y)^2) per image -> autograd backward;
                                bilinear and bicubic (torch has no Lanczos: lanczos3 is compared with torch's bicubic)
    floor                       (c) the bytes a perfect kernel pair moves: read G once, write the gradient once (201 MB at B=8, 1024²);
                                every row carries its share of it as TB/s
The W+ loop: ``model.invert`` (bench.py's synthetic model and inputs, --streams streams, launch plans on) without pixel_size and with
--pixel-size and pixel_filter='bicubic' at two step counts, --reps interleaved runs; per W+ step = (T(long) - T(short)) / (long - short),
so the OOD forward and the set-up cancel.

Prints one line per measurement and a JSON summary; --out writes the summary to a file (profiles/resample_timing.json is one).

    python tools/resample_probe.py [--batch 8] [--size 1024] [--launches 30] [--rounds 7] [--steps 100 --short 20] [--reps 5] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'ood-gan-inversion_amd'))

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

FACTORS = (2, 4, 8, 16)
FILTERS = ('bilinear', 'bicubic', 'lanczos3')


def kernel_times(a, dev):
    from oodgan import _lib, ops, synth
    L, p = _lib.lib(), ops._p
    B, S = a.batch, a.size
    CHW = 3 * S * S
    img = torch.cat([synth.normal('probe.img', (1, 3, S, S), 10 + b) for b in range(B)]).to(dev)
    x = torch.cat([synth.make_images(S, 1, seed=1000 + b) for b in range(B)]).to(dev)
    g = torch.empty_like(img)
    nparts = max(max(L.oodgan_resampled_pixel_loss_nparts(3, S, S, f), L.oodgan_pooled_pixel_loss_nparts(CHW // (f * f), f)) for f in FACTORS)
    part = torch.empty(B, nparts, device=dev)
    table, row = torch.zeros(4, B, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)
    gmul, st = ops.loss_scale_for(CHW), ops._stream()
    floor = 2 * CHW * 4 * B
    calls, keep = {}, []
    for f in FACTORS:
        xs = ops.area_pool(x, f)
        keep.append(xs)
        calls[f'box_f{f}'] = (lambda f=f, xs=xs: L.oodgan_pooled_pixel_loss_fwd_bwd_row(p(img), None, p(xs), None, p(g), None, p(part), p(table), p(row),
                                                                                       4, B, 3, S, S, f, 0, 0.0, 1, gmul, st))
        for filt in FILTERS:
            A = ops.resample_tables(filt, S, f).to(dev)
            y = ops.resample_view(x, A, A, f)
            rs = torch.empty_like(y)
            keep.append((A, y, rs))
            s = ops.RESAMPLE_FILTERS[filt]
            calls[f'resampled_{filt}_f{f}'] = (lambda f=f, s=s, A=A, y=y, rs=rs: L.oodgan_resampled_pixel_loss_fwd_bwd_row(
                p(img), p(y), p(A), p(A), p(g), p(rs), p(part), p(table), p(row), 4, B, 3, S, S, f, s, 0, 0.0, gmul, st))
            if filt == 'lanczos3':
                continue
            leaf = img.clone().requires_grad_(True)
            keep.append(leaf)

            def torch_way(f=f, filt=filt, leaf=leaf, y=y):
                leaf.grad = None
                v = F.interpolate(leaf, size=(S // f, S // f), mode=filt, antialias=True, align_corners=False)
                ((v - y) ** 2).mean(dim=(1, 2, 3)).sum().backward()
                return 0

            calls[f'torch_{filt}_f{f}'] = torch_way
    for fn in calls.values():                           # warm-up: code objects, clocks, torch's allocator
        for _ in range(5):
            _lib.check(fn(), 'probe')
    torch.cuda.synchronize()
    t = {n: [] for n in calls}
    for _ in range(a.rounds):
        for n, fn in calls.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.launches):
                fn()
            e1.record()
            e1.synchronize()
            t[n].append(e0.elapsed_time(e1) / a.launches * 1e3)
    res = {'floor_mbytes': round(floor / 1e6, 1)}
    for n, v in t.items():
        med = statistics.median(v)
        res[n] = {'median_us': round(med, 2), 'min_us': round(min(v), 2), 'max_us': round(max(v), 2), 'floor_tb_per_s': round(floor / 1e6 / med, 3)}
    for n in list(res):
        if not n.startswith('resampled_'):
            continue
        _, filt, ff = n.split('_')
        res[n]['ratio_to_box'] = round(res[n]['median_us'] / res[f'box_{ff}']['median_us'], 3)
        against = f"torch_{'bicubic' if filt == 'lanczos3' else filt}_{ff}"
        res[n]['ratio_to_torch'] = round(res[n]['median_us'] / res[against]['median_us'], 4)
        res[n]['torch_variant'] = against
    for n, r in res.items():
        if isinstance(r, dict):
            print(f"{n:>24}: median {r['median_us']:9.2f} us ({r['min_us']:.2f} .. {r['max_us']:.2f}) per call; the {res['floor_mbytes']:.0f} MB floor "
                  f"at {r['floor_tb_per_s']:.2f} TB/s" + ''.join(f", {v:.3f} x {k[9:]}" for k, v in r.items() if k.startswith('ratio_to_')))
    return res


def loop_times(a, dev):
    from oodgan import synth
    from oodgan.arch import ood_faceGAN_e4e
    size, B = a.size, a.batch
    model = ood_faceGAN_e4e(out_size=size, style_dim=512, encoder='E4E', enable_modulation=True, warp_scale=0.08, cycle_align=2,
                            blend_with_gen=True, ModSize=256, build_encoder=False)
    model.load_state_dict(synth.ood_state(size, seed=0), strict=True)
    model = model.to(dev).eval()
    cat = lambda parts: torch.cat(parts, 0).to(dev)     # noqa: E731
    x = cat([synth.make_images(size, 1, seed=1000 + g) for g in range(B)])
    enc_lats = cat([synth.make_latents(size, 1, seed=3000 + g, std=0.3) for g in range(B)])
    feats_per = [synth.make_encoder_feats(1, seed=4000 + g) for g in range(B)]
    enc_feats = [cat([f[i] for f in feats_per]) for i in range(4)]
    noise_per = [synth.make_noises(size, 1, seed=2000 + g) for g in range(B)]
    noises = [cat([n[i] for n in noise_per]) for i in range(len(noise_per[0]))]
    modes = {'default': {}, 'box': dict(pixel_size=a.pixel_size), 'bicubic': dict(pixel_size=a.pixel_size, pixel_filter='bicubic')}

    def run(m, steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        model.invert(x, steps=steps, noise=noises, streams=a.streams, enc_lats=enc_lats, enc_feats=enc_feats, **modes[m])
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    for m in modes:                                     # warm-up: plans, allocator pools, scratch buffers of both step counts
        run(m, a.short)
        run(m, a.steps)
    t = {(m, s): [] for m in modes for s in (a.short, a.steps)}
    for _ in range(a.reps):                             # interleaved
        for m in modes:
            for s in (a.short, a.steps):
                t[(m, s)].append(run(m, s))
    med = {k: statistics.median(v) for k, v in t.items()}
    res = {}
    for m in modes:
        per = (med[(m, a.steps)] - med[(m, a.short)]) / (a.steps - a.short) * 1e3
        spread = (max(t[(m, a.steps)]) - min(t[(m, a.steps)])) / med[(m, a.steps)]
        res[m] = {'ms_per_step': round(per, 3), 'invert_ms': round(med[(m, a.steps)] * 1e3, 1), 'spread_pct': round(100 * spread, 2)}
    for m in modes:
        r = res[m]
        r['ratio_to_default'] = round(r['ms_per_step'] / res['default']['ms_per_step'], 4)
        print(f"{m:>8}: {r['ms_per_step']:.3f} ms per W+ step ({r['ratio_to_default']:.4f} x default); invert({a.steps}) {r['invert_ms']:.1f} ms "
              f"(spread {r['spread_pct']:.2f} %)")
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=8)
    ap.add_argument('--size', type=int, default=1024)
    ap.add_argument('--pixel-size', type=int, default=256)
    ap.add_argument('--launches', type=int, default=30)
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--streams', type=int, default=2)
    ap.add_argument('--steps', type=int, default=100)
    ap.add_argument('--short', type=int, default=20)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--no-loop', action='store_true', help='kernels only')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('resample_probe needs a GPU: a timing taken elsewhere says nothing')
    dev = torch.device('cuda:0')
    res = {'batch': a.batch, 'size': a.size, 'pixel_size': a.pixel_size, 'launches_per_window': a.launches, 'rounds': a.rounds,
           'streams': a.streams, 'steps': [a.short, a.steps], 'reps': a.reps, 'device': torch.cuda.get_device_name(0),
           'torch_note': 'F.interpolate(antialias=True) + mean((v - y)^2) per image + autograd backward on the same GPU; torch has no Lanczos, so '
                         'lanczos3 is compared with torch bicubic',
           'kernels': kernel_times(a, dev)}
    if not a.no_loop:
        res['loop'] = loop_times(a, dev)
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            json.dump(res, f, indent=1)
            f.write('\n')


if __name__ == '__main__':
    main()
