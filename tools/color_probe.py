#!/usr/bin/env python3
"""Cost of the colour map of the W+ loop (csrc/loss_color.hip), in ONE process on one GPU.

Kernels, at B=8, 3 x 1024², after a warm-up, timed with HIP events over --launches calls per window, interleaved over --rounds windows (a
drift of the clock hits every variant alike); median and minimum per call:
    mse + finish                     oodgan_mse_fwd_bwd: reads G and x, writes the gradient — the yardstick of the same process
    color term + finish              oodgan_color_pixel_loss_fwd_bwd (MSE): the same bytes, plus the colour map, its transpose and the 12 sums
    color term + finish, beta/huber  the same with a loss weight and the Huber kind
    color_step                       oodgan_color_step: the partial sums, theta and its moments
    color_apply                      reads G, writes C(G)
The W+ loop: ``model.invert`` (bench.py's synthetic model and inputs, --streams streams, launch plans on) without the option and with
``color='affine'``, at two step counts, interleaved; per W+ step = (T(long) - T(short)) / (long - short), so the OOD forward and the set-up
cancel.  Medians over --reps, the spread stated.  The comparison is against the plain W+ step of the same process.

Prints one line per measurement and a JSON summary; --out writes the summary to a file.

    python tools/color_probe.py [--batch 8] [--size 1024] [--launches 50] [--rounds 9] [--steps 100 --short 20] [--reps 5] [--out FILE]
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
    from oodgan import ops, synth
    B, S = a.batch, a.size
    shape = (B, 3, S, S)
    img, x = synth.normal('probe.img', shape, 10).to(dev), synth.normal('probe.x', shape, 11).to(dev)
    beta = torch.rand(B, 1, S, S, device=dev)
    gimg = torch.empty_like(img)
    th = torch.tensor([[0.80, 0.15, 0.05, 0.10, 0.75, 0.05, 0.05, 0.10, 0.60, -0.04, 0.02, 0.06]] * B, device=dev)
    g, m, v = (torch.zeros(B, 12, device=dev) for _ in range(3))
    t, parts, loss = torch.ones(1, dtype=torch.int32, device=dev), ops.color_parts(B, S, S, dev), torch.empty(B, device=dev)
    gmul = ops.loss_scale_for(3 * S * S)
    nbytes = img.numel() * 4
    calls = {
        'mse + finish': (lambda: ops.pixel_loss_grad(img, x, grad_mul=gmul, loss_out=loss), 3 * nbytes),
        'color term + finish': (lambda: ops.color_pixel_loss_grad(img, x, th, 'mse', grad_mul=gmul, loss_out=loss, parts=parts, out=gimg), 3 * nbytes),
        'color term + finish, beta/huber': (lambda: ops.color_pixel_loss_grad(img, x, th, 'huber', 0.1, beta, gmul, loss_out=loss, parts=parts, out=gimg),
                                            3 * nbytes + nbytes // 3),
        'color_step': (lambda: ops.color_step(th, g, m, v, parts[1], t, 100, lr=0.0, grad_div=gmul), parts[1].numel() * 8),
        'color_apply': (lambda: ops.color_apply(img, th, out=gimg), 2 * nbytes),
    }
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
    for n, vals in ts.items():
        mb = calls[n][1] / 1e6
        res[n] = {'median_us': round(statistics.median(vals), 2), 'min_us': round(min(vals), 2), 'max_us': round(max(vals), 2), 'MB': round(mb, 1)}
        print(f"{n:>32}: median {res[n]['median_us']:8.2f} us (min {res[n]['min_us']:.2f}, max {res[n]['max_us']:.2f}) per call, {mb:.0f} MB: "
              f"{mb / res[n]['median_us']:.2f} TB/s")
    res['color_term_over_mse'] = round(res['color term + finish']['median_us'] / res['mse + finish']['median_us'], 3)
    print(f"fused colour term + finish / MSE kernel + finish: {res['color_term_over_mse']:.3f}")
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

    def run(mode, steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        model.invert(x, steps=steps, streams=a.streams, color=mode, **kw)
        torch.cuda.synchronize()
        launches[mode] = model.last_invert_plan['launches']
        return time.perf_counter() - t0

    modes = (None, 'affine')
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
        print(f"color {str(m):>8}: {r['ms_per_step']:.3f} ms per W+ step ({r['ratio_to_wplus']:.4f} x the plain step); invert({a.steps}) "
              f"{r['invert_ms']:.1f} ms (spread {r['spread_pct']:.2f} %), launches {r['launches_per_step']}")
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
        raise SystemExit('color_probe needs a GPU: a timing taken elsewhere says nothing')
    dev = torch.device('cuda:0')
    res = {'batch': a.batch, 'size': a.size, 'launches_per_window': a.launches, 'rounds': a.rounds, 'streams': a.streams,
           'steps': [a.short, a.steps], 'reps': a.reps, 'device': torch.cuda.get_device_name(0), 'kernels': kernel_times(a, dev)}
    if not a.no_loop:
        model, x, kw = bench_model(a, dev)
        res['loop'] = loop_times(a, model, x, kw)
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            json.dump(res, f, indent=1)
            f.write('\n')


if __name__ == '__main__':
    main()
