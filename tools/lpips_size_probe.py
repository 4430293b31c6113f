#!/usr/bin/env python3
"""Cost of the pooled view of the LPIPS term (``lpips_size``; csrc/loss_pool.hip), in ONE process on one GPU, seeded inputs.

Kernels, at B=8, 1024² (the bench geometry), after a warm-up, timed with HIP events over --launches calls per window, the calls interleaved
over --rounds windows each (a drift of the clock hits every one alike); median and minimum per call:
    oodgan_area_pool_fwd (with the zeroed gradient buffer)   algorithmic bytes B*3*S²*4*(1 + 2/f²)
    oodgan_area_pool_bwd_add                                 algorithmic bytes B*3*S²*4*(2 + 1/f²)
    oodgan_scale_by_plane on the same gimg                   the yardstick of the backward: a read-modify-write of the same bytes, + beta
for every factor; TB/s from those bytes and the backward's time against the yardstick's, scaled by the byte ratio.
The W+ loop: ``model.invert`` (bench.py's synthetic model and inputs, --streams streams, launch plans on) without LPIPS, with LPIPS at the
image size and with ``lpips_size`` = --lpips-size, alternated --reps times at two step counts; per W+ step =
(T(long) - T(short)) / (long - short), i.e. the mean over steps short..long, so the OOD forward and the set-up cancel.  Medians and the
spread of the repeats.

    python tools/lpips_size_probe.py [--batch 8] [--size 1024] [--lpips-size 256] [--launches 50] [--rounds 9] [--steps 100 --short 20] [--reps 5]
                                     [--out profiles/lpips_size_timing.json]
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
    x = torch.cat([synth.make_images(S, 1, seed=1000 + b) for b in range(B)]).to(dev)
    gimg = torch.cat([synth.normal('probe.g', (1, 3, S, S), 10 + b) for b in range(B)]).to(dev)
    beta = torch.ones(B, 1, S, S, device=dev)           # ones and a zero gs: the timed calls leave gimg's values alone
    st = ops._stream()
    full_bytes = B * 3 * S * S * 4
    calls = {'scale_by_plane': (lambda: L.oodgan_scale_by_plane(p(gimg), p(beta), B, 3, S * S, st), full_bytes * (2 + 1 / 3))}
    keep = []
    for f in (2, 4, 8, 16):
        y, gz, gs = (torch.zeros(B, 3, S // f, S // f, device=dev) for _ in range(3))
        keep.append((y, gz, gs))
        calls[f'pool_fwd_f{f}'] = (lambda f=f, y=y, gz=gz: L.oodgan_area_pool_fwd(p(x), p(y), p(gz), B * 3, S, S, f, st), full_bytes * (1 + 2 / f ** 2))
        calls[f'pool_bwd_add_f{f}'] = (lambda f=f, gs=gs: L.oodgan_area_pool_bwd_add(p(gs), p(gimg), B * 3, S, S, f, st), full_bytes * (2 + 1 / f ** 2))
    for fn, _ in calls.values():                        # warm-up: code objects, clocks
        for _ in range(10):
            _lib.check(fn(), 'probe')
    torch.cuda.synchronize()
    t = {n: [] for n in calls}
    for _ in range(a.rounds):
        for n, (fn, _) in calls.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.launches):
                fn()
            e1.record()
            e1.synchronize()
            t[n].append(e0.elapsed_time(e1) / a.launches * 1e3)
    res = {}
    for n, v in t.items():
        med, nbytes = statistics.median(v), calls[n][1]
        res[n] = {'median_us': round(med, 2), 'min_us': round(min(v), 2), 'max_us': round(max(v), 2), 'bytes': int(nbytes),
                  'tb_per_s': round(nbytes / med / 1e6, 3)}
    ys = res['scale_by_plane']
    ys['spread_pct'] = round(100 * (ys['max_us'] - ys['min_us']) / ys['median_us'], 2)
    for n, r in res.items():
        line = f"{n:>18}: median {r['median_us']:8.2f} us, min {r['min_us']:8.2f}, max {r['max_us']:8.2f} per call ({r['bytes'] / 1e6:.0f} MB: {r['tb_per_s']:.2f} TB/s)"
        if n.startswith('pool_bwd'):
            # the yardstick's time scaled to this kernel's bytes; > 1: slower per byte than scale_by_plane
            r['ratio_to_scaled_yardstick'] = round(r['median_us'] / (ys['median_us'] * r['bytes'] / ys['bytes']), 4)
            line += f", {r['ratio_to_scaled_yardstick']:.3f} x scale_by_plane per byte"
        print(line)
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
    modes = {'no_lpips': dict(lpips_weight=0.0), f'lpips_{size}': dict(lpips_weight=a.lpips_weight),
             f'lpips_size_{a.lpips_size}': dict(lpips_weight=a.lpips_weight, lpips_size=a.lpips_size)}

    def run(mode, steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        model.invert(x, steps=steps, noise=noises, streams=a.streams, enc_lats=enc_lats, enc_feats=enc_feats, **modes[mode])
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    for m in modes:                                     # warm-up: plans, allocator pools, scratch buffers of both step counts
        run(m, a.short)
        run(m, a.steps)
    t = {(m, s): [] for m in modes for s in (a.short, a.steps)}
    for _ in range(a.reps):                             # alternated
        for m in modes:
            for s in (a.short, a.steps):
                t[(m, s)].append(run(m, s))
    res = {}
    for m in modes:
        per = [(hi - lo) / (a.steps - a.short) * 1e3 for lo, hi in zip(t[(m, a.short)], t[(m, a.steps)])]
        res[m] = {'ms_per_step': round(statistics.median(per), 3), 'min': round(min(per), 3), 'max': round(max(per), 3),
                  'invert_ms': round(statistics.median(t[(m, a.steps)]) * 1e3, 1)}
    base = res['no_lpips']['ms_per_step']
    for m, r in res.items():
        r['over_no_lpips_ms'] = round(r['ms_per_step'] - base, 3)
        print(f"{m:>16}: {r['ms_per_step']:.3f} ms per W+ step (repeats {r['min']:.3f} .. {r['max']:.3f}), +{r['over_no_lpips_ms']:.3f} ms over no LPIPS; "
              f"invert({a.steps}) {r['invert_ms']:.1f} ms")
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=8)
    ap.add_argument('--size', type=int, default=1024)
    ap.add_argument('--lpips-size', type=int, default=256)
    ap.add_argument('--lpips-weight', type=float, default=0.8)
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
        raise SystemExit('lpips_size_probe needs a GPU: a timing taken elsewhere says nothing')
    dev = torch.device('cuda:0')
    res = {'batch': a.batch, 'size': a.size, 'lpips_size': a.lpips_size, 'lpips_weight': a.lpips_weight, 'launches_per_window': a.launches,
           'rounds': a.rounds, 'streams': a.streams, 'steps': [a.short, a.steps], 'reps': a.reps, 'device': torch.cuda.get_device_name(0),
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
