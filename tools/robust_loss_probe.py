#!/usr/bin/env python3
"""Cost of the robust pixel terms (csrc/loss_pixel.hip) against the MSE instantiations of the same kernels, in ONE process on one GPU.

Kernels, at B=8, 1024² (the bench geometry), after a warm-up, timed with HIP events over --launches calls per window, the variants
interleaved over --rounds windows each (a drift of the clock hits every variant alike); median and minimum per call (main kernel + the
finish kernel, as the W+ step issues them):
    oodgan_mse_fwd_bwd_row             against each robust kind, plain   (reads G, x; writes the gradient: 302 MB)
    oodgan_composite_mse_fwd_bwd_row   against each robust kind, with beta (+ 34 MB), gradient w.r.t. G
The W+ loop: ``model.invert`` (bench.py's synthetic model and inputs, --streams streams, launch plans on) with pixel_loss='mse' and each
kind at two step counts; per W+ step = (T(long) - T(short)) / (long - short), so the OOD forward and the set-up cancel.  Medians over --reps.

Prints one line per measurement and a JSON summary; --out writes the summary to a file.

    python tools/robust_loss_probe.py [--batch 8] [--size 1024] [--launches 50] [--rounds 9] [--steps 100 --short 20] [--reps 5] [--out FILE]
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


def kernel_times(a, dev):
    from oodgan import _lib, ops, synth
    L, p = _lib.lib(), ops._p
    B, S = a.batch, a.size
    HW, CHW = S * S, 3 * S * S
    img = torch.cat([synth.normal('probe.img', (1, 3, S, S), 10 + b) for b in range(B)]).to(dev)
    x = torch.cat([synth.make_images(S, 1, seed=1000 + b) for b in range(B)]).to(dev)
    beta = torch.sigmoid(2.0 * synth.normal('probe.beta', (B, 1, S, S), 5)).to(dev)
    g = torch.empty_like(img)
    part = torch.empty(B, L.oodgan_mse_nparts(CHW), device=dev)
    table, row = torch.zeros(4, B, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)
    gmul, st = ops.loss_scale_for(CHW), ops._stream()
    calls = {'mse': lambda: L.oodgan_mse_fwd_bwd_row(p(img), p(x), p(g), p(part), p(table), p(row), 4, B, CHW, gmul, st),
             'composite_mse': lambda: L.oodgan_composite_mse_fwd_bwd_row(p(img), p(x), p(beta), p(g), None, p(part), p(table), p(row), 4, B, 3, HW, 1,
                                                                         gmul, st)}
    for kind, k in ops.ROBUST_KINDS.items():
        calls[kind] = (lambda k=k: L.oodgan_robust_loss_fwd_bwd_row(p(img), p(x), None, p(g), None, p(part), p(table), p(row), 4, B, 3, HW, k,
                                                                    a.scale, 1, gmul, st))
        calls[kind + '+beta'] = (lambda k=k: L.oodgan_robust_loss_fwd_bwd_row(p(img), p(x), p(beta), p(g), None, p(part), p(table), p(row), 4, B, 3,
                                                                              HW, k, a.scale, 1, gmul, st))
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
        res[n] = {'median_us': round(statistics.median(v), 2), 'min_us': round(min(v), 2)}
    for n in res:
        base = 'composite_mse' if n.endswith('+beta') else 'mse'
        if n not in ('mse', 'composite_mse'):
            res[n]['ratio_to_' + base] = round(res[n]['median_us'] / res[base]['median_us'], 4)
        mb = (3 * CHW + (HW if (n.endswith('+beta') or n == 'composite_mse') else 0)) * 4 * B / 1e6
        print(f"{n:>22}: median {res[n]['median_us']:8.2f} us, min {res[n]['min_us']:8.2f} us per call ({mb:.0f} MB: "
              f"{mb / res[n]['median_us']:.2f} TB/s)" + (f", {res[n]['ratio_to_' + base]:.3f} x {base}" if 'ratio_to_' + base in res[n] else ''))
    return res


def loop_times(a, dev):
    from oodgan import ops, synth
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

    def run(kind, steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        model.invert(x, steps=steps, noise=noises, streams=a.streams, pixel_loss=kind, pixel_scale=a.scale, enc_lats=enc_lats, enc_feats=enc_feats)
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    modes = ('mse',) + tuple(ops.ROBUST_KINDS)
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
        res[m]['ratio_to_mse'] = round(res[m]['ms_per_step'] / res['mse']['ms_per_step'], 4)
        print(f"{m:>14}: {res[m]['ms_per_step']:.3f} ms per W+ step ({res[m]['ratio_to_mse']:.4f} x mse); invert({a.steps}) "
              f"{res[m]['invert_ms']:.1f} ms (spread {res[m]['spread_pct']:.2f} %)")
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=8)
    ap.add_argument('--size', type=int, default=1024)
    ap.add_argument('--scale', type=float, default=0.1)
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
        raise SystemExit('robust_loss_probe needs a GPU: a timing taken elsewhere says nothing')
    dev = torch.device('cuda:0')
    res = {'batch': a.batch, 'size': a.size, 'scale': a.scale, 'launches_per_window': a.launches, 'rounds': a.rounds, 'streams': a.streams,
           'steps': [a.short, a.steps], 'reps': a.reps, 'device': torch.cuda.get_device_name(0), 'kernels': kernel_times(a, dev)}
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
