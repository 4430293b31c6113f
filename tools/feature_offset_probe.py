#!/usr/bin/env python3
"""Cost and effect of the feature offset of the W+ loop (csrc/feature_offset.hip), in ONE process on one GPU.

Kernels, at B=8 and the three offset shapes (512 x 8², 16², 32²), after a warm-up, timed with HIP events over --launches calls per window,
interleaved over --rounds windows (a drift of the clock hits every variant alike); median and minimum per call:
    oodgan_feature_add     reads x and delta, writes x'
    oodgan_feature_step    reads and writes delta, g, m, v; with the regulariser's table also the partial sums and the finish kernel
The W+ loop: ``model.invert`` (bench.py's synthetic model and inputs, --streams streams, launch plans on) without the option and with
feature_layer 3, 5 and 7, at two step counts, interleaved; per W+ step = (T(long) - T(short)) / (long - short), so the OOD forward and the set-up
cancel.  Medians over --reps.  The comparison is against the plain W+ step of the same process.
The fit: the same inputs with an occluder pasted into every target — a flat rectangle over the upper third of the image, content no latent
expresses — inverted with --steps steps without the option and with feature_layer 5: the last loss of the loop and the mean squared error of
the blended output, over the whole image and inside the rectangle.

Prints one line per measurement and a JSON summary; --out writes the summary to a file.

    python tools/feature_offset_probe.py [--batch 8] [--size 1024] [--launches 50] [--rounds 9] [--steps 100 --short 20] [--reps 5] [--out FILE]
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

LAYERS = (3, 5, 7)


def kernel_times(a, dev):
    from oodgan import _lib, ops, synth
    B = a.batch
    calls = {}
    keep = []
    for l in LAYERS:
        h = 4 << ((l - 1) // 2)
        shape = (B, 512, h, h)
        x, d = synth.normal('probe.x', shape, 10 + l).to(dev), synth.normal('probe.d', shape, 20 + l, 0.1).to(dev)
        y, g = torch.empty_like(x), synth.normal('probe.g', shape, 30 + l).to(dev)
        m, v = torch.zeros_like(x), torch.zeros_like(x)
        t = torch.ones(1, dtype=torch.int32, device=dev)
        table, part = torch.zeros(4, B, device=dev), ops.feature_step_parts(B, 512 * h * h, dev)
        keep.append((x, d, y, g, m, v, t, table, part))
        calls[f'feature_add l={l}'] = (lambda x=x, d=d, y=y: ops.feature_add(x, d, out=y), 3 * x.numel() * 4)
        calls[f'feature_step l={l}'] = (lambda d=d, g=g, m=m, v=v, t=t: ops.feature_step(d, g, m, v, t, 100, lr=1e-4), 8 * x.numel() * 4)
        calls[f'feature_step+reg l={l}'] = (lambda d=d, g=g, m=m, v=v, t=t, table=table, part=part:
                                            ops.feature_step(d, g, m, v, t, 100, lr=1e-4, feature_reg=0.5, table=table, part=part), 8 * x.numel() * 4)
    for f, _ in calls.values():                         # warm-up: code objects, clocks
        for _ in range(10):
            f()
    torch.cuda.synchronize()
    ts = {n: [] for n in calls}
    for _ in range(a.rounds):
        for n, (f, _) in calls.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.launches):
                f()
            e1.record()
            e1.synchronize()
            ts[n].append(e0.elapsed_time(e1) / a.launches * 1e3)
    res = {}
    for n, v in ts.items():
        mb = calls[n][1] / 1e6
        res[n] = {'median_us': round(statistics.median(v), 2), 'min_us': round(min(v), 2), 'max_us': round(max(v), 2), 'MB': round(mb, 1)}
        print(f"{n:>24}: median {res[n]['median_us']:8.2f} us (min {res[n]['min_us']:.2f}, max {res[n]['max_us']:.2f}) per call, {mb:.0f} MB: "
              f"{mb / res[n]['median_us']:.2f} TB/s")
    return res


def bench_model(a, dev):
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
    return model, x, dict(noise=noises, enc_lats=enc_lats, enc_feats=enc_feats)


def loop_times(a, model, x, kw):
    launches = {}

    def run(layer, steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        model.invert(x, steps=steps, streams=a.streams, feature_layer=layer, **kw)
        torch.cuda.synchronize()
        launches[layer] = model.last_invert_plan['launches']
        return time.perf_counter() - t0

    modes = (None,) + LAYERS
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
        res[str(m)] = {'ms_per_step': round(per, 3), 'invert_ms': round(med[(m, a.steps)] * 1e3, 1), 'spread_pct': round(100 * spread, 2),
                       'launches_per_step': launches[m]}
    for m in modes:
        r = res[str(m)]
        r['ratio_to_wplus'] = round(r['ms_per_step'] / res['None']['ms_per_step'], 4)
        print(f"feature_layer {str(m):>4}: {r['ms_per_step']:.3f} ms per W+ step ({r['ratio_to_wplus']:.4f} x the plain step); invert({a.steps}) "
              f"{r['invert_ms']:.1f} ms (spread {r['spread_pct']:.2f} %)")
    return res


def fit(a, model, x, kw):
    S = a.size
    xo = x.clone()
    y0, y1, x0, x1 = S // 16, S // 3, S // 4, 3 * S // 4
    xo[:, 0, y0:y1, x0:x1], xo[:, 1, y0:y1, x0:x1], xo[:, 2, y0:y1, x0:x1] = 0.8, -0.6, 0.1
    res = {'occluder': [y0, y1, x0, x1]}
    for layer in (None, 5):
        out, _, losses = model.invert(xo, steps=a.steps, streams=a.streams, feature_layer=layer, **kw)
        e = (out - xo) ** 2
        res[str(layer)] = {'first_loss': round(losses[0].mean().item(), 5), 'last_loss': round(losses[-1].mean().item(), 5),
                           'output_mse': round(e.mean().item(), 5), 'output_mse_in_occluder': round(e[:, :, y0:y1, x0:x1].mean().item(), 5)}
        r = res[str(layer)]
        print(f"occluded targets, feature_layer {str(layer):>4}: loss {r['first_loss']:.4f} -> {r['last_loss']:.4f} after {a.steps} steps; blended output "
              f"MSE {r['output_mse']:.4f}, inside the occluder {r['output_mse_in_occluder']:.4f}")
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=8)
    ap.add_argument('--size', type=int, default=1024)
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
        raise SystemExit('feature_offset_probe needs a GPU: a timing taken elsewhere says nothing')
    dev = torch.device('cuda:0')
    res = {'batch': a.batch, 'size': a.size, 'launches_per_window': a.launches, 'rounds': a.rounds, 'streams': a.streams,
           'steps': [a.short, a.steps], 'reps': a.reps, 'device': torch.cuda.get_device_name(0), 'kernels': kernel_times(a, dev)}
    if not a.no_loop:
        model, x, kw = bench_model(a, dev)
        res['loop'] = loop_times(a, model, x, kw)
        res['fit'] = fit(a, model, x, kw)
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            json.dump(res, f, indent=1)
            f.write('\n')


if __name__ == '__main__':
    main()
