#!/usr/bin/env python3
"""Cost of the pixel term on an area-pooled view (csrc/loss_pixel.hip: pooled_pixel_kernel) against the kernels it sits
beside and the composition it replaces, in ONE process on one GPU.

Kernels, at B=8, 1024² (the bench geometry), after a warm-up, timed with HIP events over --launches calls per window, the variants
interleaved over --rounds windows each (a drift of the clock hits every variant alike); median and minimum per call (main kernel + the
finish kernel, as the W+ step issues them):
    oodgan_mse_fwd_bwd_row                    today's pixel term                                   (reads G, x; writes the gradient)
    oodgan_composite_mse_fwd_bwd_row          today's pixel term with beta, gradient w.r.t. G
    composition, F in {2, 4, 8, 16}           area_pool(G) -> the MSE at the small size -> area_pool(zeros)'s fill -> area_pool_bwd_add:
                                              the four passes the fused kernel replaces (the pooled target is made once, outside)
    oodgan_pooled_pixel_loss_fwd_bwd_row      the fused kernel, F in {2, 4, 8, 16}, without beta (reads G and the pooled target, writes the
                                              gradient) and with beta (reads G, x, beta; reads beta again; writes the gradient)
The W+ loop: ``model.invert`` (bench.py's synthetic model and inputs, --streams streams, launch plans on) with pixel_size None and
--pixel-size at two step counts; per W+ step = (T(long) - T(short)) / (long - short), so the OOD forward and the set-up cancel.  Medians over
--reps.

Prints one line per measurement and a JSON summary; --out writes the summary to a file (profiles/pixel_size_timing.json is one).

    python tools/pixel_size_probe.py [--batch 8] [--size 1024] [--launches 50] [--rounds 9] [--steps 100 --short 20] [--reps 5] [--out FILE]
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

FACTORS = (2, 4, 8, 16)


def kernel_times(a, dev):
    from oodgan import _lib, ops, synth
    L, p = _lib.lib(), ops._p
    B, S = a.batch, a.size
    HW, CHW = S * S, 3 * S * S
    img = torch.cat([synth.normal('probe.img', (1, 3, S, S), 10 + b) for b in range(B)]).to(dev)
    x = torch.cat([synth.make_images(S, 1, seed=1000 + b) for b in range(B)]).to(dev)
    beta = torch.sigmoid(2.0 * synth.normal('probe.beta', (B, 1, S, S), 5)).to(dev)
    g = torch.empty_like(img)
    part = torch.empty(B, max(L.oodgan_mse_nparts(CHW), max(L.oodgan_pooled_pixel_loss_nparts(CHW // (f * f), f) for f in FACTORS)), device=dev)
    table, row = torch.zeros(4, B, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)
    gmul, st = ops.loss_scale_for(CHW), ops._stream()
    calls = {'mse': lambda: L.oodgan_mse_fwd_bwd_row(p(img), p(x), p(g), p(part), p(table), p(row), 4, B, CHW, gmul, st),
             'composite_mse': lambda: L.oodgan_composite_mse_fwd_bwd_row(p(img), p(x), p(beta), p(g), None, p(part), p(table), p(row), 4, B, 3, HW, 1,
                                                                         gmul, st)}
    nbytes = {'mse': 3 * CHW * 4 * B, 'composite_mse': (3 * CHW + HW) * 4 * B}
    keep = []
    for f in FACTORS:
        s = S // f
        xs = ops.area_pool(x, f)
        small, gs, zs = torch.empty_like(xs), torch.empty_like(xs), torch.empty_like(xs)
        keep.append((xs, small, gs, zs))

        def composition(f=f, s=s, xs=xs, small=small, gs=gs, zs=zs):
            # pool G; the MSE at the small size; the zero fill of the full-resolution gradient (torch's fill kernel: a probe may use it, a
            # recorded step could not); the adjoint added into the zeroed buffer
            L.oodgan_area_pool_fwd(p(img), p(small), None, B * 3, S, S, f, st)
            L.oodgan_mse_fwd_bwd_row(p(small), p(xs), p(gs), p(part), p(table), p(row), 4, B, 3 * s * s, gmul, st)
            g.zero_()
            return L.oodgan_area_pool_bwd_add(p(gs), p(g), B * 3, S, S, f, st)

        calls[f'composition_f{f}'] = composition
        nbytes[f'composition_f{f}'] = (CHW + CHW + 2 * CHW) * 4 * B + 4 * (CHW // (f * f)) * 4 * B
        calls[f'fused_f{f}'] = (lambda f=f, xs=xs: L.oodgan_pooled_pixel_loss_fwd_bwd_row(p(img), None, p(xs), None, p(g), None, p(part), p(table), p(row),
                                                                                         4, B, 3, S, S, f, 0, 0.0, 1, gmul, st))
        nbytes[f'fused_f{f}'] = (2 * CHW + CHW // (f * f)) * 4 * B
        calls[f'fused_f{f}+beta'] = (lambda f=f: L.oodgan_pooled_pixel_loss_fwd_bwd_row(p(img), p(x), None, p(beta), p(g), None, p(part), p(table), p(row),
                                                                                       4, B, 3, S, S, f, 0, 0.0, 1, gmul, st))
        nbytes[f'fused_f{f}+beta'] = (3 * CHW + HW) * 4 * B               # HBM bytes: the second read of beta is expected from L2
    for f in calls.values():                            # warm-up: code objects, clocks
        for _ in range(10):
            _lib.check(f(), 'probe')
    torch.cuda.synchronize()
    t = {n: [] for n in calls}
    for _ in range(a.rounds):
        for n, f in calls.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.launches):
                f()
            e1.record()
            e1.synchronize()
            t[n].append(e0.elapsed_time(e1) / a.launches * 1e3)
    res = {}
    for n, v in t.items():
        res[n] = {'median_us': round(statistics.median(v), 2), 'min_us': round(min(v), 2), 'max_us': round(max(v), 2),
                  'mbytes': round(nbytes[n] / 1e6, 1), 'tb_per_s': round(nbytes[n] / 1e6 / statistics.median(v), 3)}
    for n in res:
        base = 'composite_mse' if n.endswith('+beta') else 'mse'
        if n not in ('mse', 'composite_mse'):
            res[n]['ratio_to_' + base] = round(res[n]['median_us'] / res[base]['median_us'], 4)
        if n.startswith('fused_f') and not n.endswith('+beta'):
            res[n]['ratio_to_composition'] = round(res[n]['median_us'] / res['composition_' + n[6:]]['median_us'], 4)
        print(f"{n:>18}: median {res[n]['median_us']:8.2f} us, min {res[n]['min_us']:8.2f}, max {res[n]['max_us']:8.2f} us per call "
              f"({res[n]['mbytes']:.0f} MB: {res[n]['tb_per_s']:.2f} TB/s)"
              + ''.join(f", {v:.3f} x {k[9:]}" for k, v in res[n].items() if k.startswith('ratio_to_')))
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

    def run(psize, steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        model.invert(x, steps=steps, noise=noises, streams=a.streams, pixel_size=psize, enc_lats=enc_lats, enc_feats=enc_feats)
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    modes = (None, a.pixel_size)
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
        res[str(m)] = {'ms_per_step': round(per, 3), 'invert_ms': round(med[(m, a.steps)] * 1e3, 1), 'spread_pct': round(100 * spread, 2)}
    for m in modes:
        r = res[str(m)]
        r['ratio_to_none'] = round(r['ms_per_step'] / res['None']['ms_per_step'], 4)
        print(f"pixel_size={m!s:>5}: {r['ms_per_step']:.3f} ms per W+ step ({r['ratio_to_none']:.4f} x None); invert({a.steps}) "
              f"{r['invert_ms']:.1f} ms (spread {r['spread_pct']:.2f} %)")
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=8)
    ap.add_argument('--size', type=int, default=1024)
    ap.add_argument('--pixel-size', type=int, default=256)
    ap.add_argument('--launches', type=int, default=50)
    ap.add_argument('--rounds', type=int, default=9)
    ap.add_argument('--streams', type=int, default=2)
    ap.add_argument('--steps', type=int, default=100)
    ap.add_argument('--short', type=int, default=20)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--no-loop', action='store_true', help='kernels only')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('pixel_size_probe needs a GPU: a timing taken elsewhere says nothing')
    dev = torch.device('cuda:0')
    res = {'batch': a.batch, 'size': a.size, 'pixel_size': a.pixel_size, 'launches_per_window': a.launches, 'rounds': a.rounds,
           'streams': a.streams, 'steps': [a.short, a.steps], 'reps': a.reps, 'device': torch.cuda.get_device_name(0),
           'composition_note': 'area_pool(G) + MSE at the small size + a torch zero fill of the full gradient + area_pool_bwd_add; the pooled '
                               'target is made once outside, as in the fused route',
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
