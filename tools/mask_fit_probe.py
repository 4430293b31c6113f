#!/usr/bin/env python3
"""Cost of the fitted mask of the W+ loop (csrc/loss_maskfit.hip) against the frozen-beta step it extends, in ONE process on one GPU.

Kernels, at B=8, 1024², m=64 (the bench geometry, the default mask size), after a warm-up, timed with HIP events over --launches calls per
window, the variants interleaved over --rounds windows each (a drift of the clock hits every variant alike); median and minimum per call:
    oodgan_scale_by_plane   reads and writes dL/dc, reads beta                                   (what the frozen-beta step does)
    oodgan_maskfit_chain    reads dL/dc, G, x, beta; writes dL/dc and e                          (takes its place)
    oodgan_maskfit_expand   writes a and beta
    oodgan_maskfit_step     reads e (each pixel row by the two cell rows above and below it), a; Adam on the logits
The W+ loop: ``model.invert`` (bench.py's synthetic model and inputs, --streams streams, launch plans on) with ``loss_region`` = a beta tensor
(the frozen-beta step) and ``loss_region='fit'`` at two step counts; per W+ step = (T(long) - T(short)) / (long - short), so the OOD forward
and the set-up cancel.  Medians over --reps, the two modes interleaved.

Prints one line per measurement and a JSON summary; --out writes the summary to a file.

    python tools/mask_fit_probe.py [--batch 8] [--size 1024] [--mask 64] [--launches 50] [--rounds 9] [--steps 100 --short 20] [--reps 5] [--out FILE]
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
    B, S, m = a.batch, a.size, a.mask
    img = torch.cat([synth.normal('probe.img', (1, 3, S, S), 10 + b) for b in range(B)]).to(dev)
    x = torch.cat([synth.make_images(S, 1, seed=1000 + b) for b in range(B)]).to(dev)
    g = (1e-3 * synth.normal('probe.g', (B, 3, S, S), 6)).to(dev)
    logit = (1.5 + synth.normal('probe.l', (B, 1, m, m), 5)).to(dev)
    av, beta = ops.maskfit_expand(logit, S)
    e = torch.empty(B, 1, S, S, device=dev)
    gl, mm, mv = (torch.zeros_like(logit) for _ in range(3))
    ta, tb, t = torch.zeros(4, B, device=dev), torch.zeros(4, B, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)
    stat = ops.maskfit_stat(B, dev)
    img_mb, plane_mb = 3 * S * S * 4 * B / 1e6, S * S * 4 * B / 1e6
    calls = {'scale_by_plane': (lambda: ops.scale_by_plane(g, beta), 2 * img_mb + plane_mb),
             'maskfit_chain': (lambda: ops.maskfit_chain(g, img, x, beta, e=e), 4 * img_mb + 2 * plane_mb),
             'maskfit_expand': (lambda: ops.maskfit_expand(logit, S, a=av, beta=beta), plane_mb),
             'maskfit_step': (lambda: ops.maskfit_step(logit, gl, mm, mv, av, e, t, 100, lr=1e-6, grad_div=1.0, area_table=ta, binary_table=tb,
                                                       stat=stat), plane_mb)}
    for f, _ in calls.values():                         # warm-up: code objects, clocks
        for _ in range(10):
            f()
    torch.cuda.synchronize()
    tm = {n: [] for n in calls}
    for _ in range(a.rounds):
        for n, (f, _) in calls.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.launches):
                f()
            e1.record()
            e1.synchronize()
            tm[n].append(e0.elapsed_time(e1) / a.launches * 1e3)
    res = {}
    for n, v in tm.items():
        mb = calls[n][1]
        res[n] = {'median_us': round(statistics.median(v), 2), 'min_us': round(min(v), 2), 'mb': round(mb, 1),
                  'tb_per_s': round(mb / statistics.median(v), 3)}
        print(f"{n:>16}: median {res[n]['median_us']:8.2f} us, min {res[n]['min_us']:8.2f} us per call ({mb:.0f} MB: {res[n]['tb_per_s']:.2f} TB/s)")
    added = res['maskfit_chain']['median_us'] - res['scale_by_plane']['median_us'] + res['maskfit_expand']['median_us'] + res['maskfit_step']['median_us']
    res['added_us_per_step'] = round(added, 2)
    print(f'added per step over the frozen-beta step with a second term (chain - scale_by_plane + expand + step): {added:.1f} us')
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
    frozen = torch.full((B, 1, size, size), 0.88, device=dev)
    modes = {'frozen_beta': dict(loss_region=frozen), 'fit': dict(loss_region='fit', mask_size=a.mask)}

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
    for _ in range(a.reps):                             # interleaved
        for m in modes:
            for s in (a.short, a.steps):
                t[(m, s)].append(run(m, s))
    med = {k: statistics.median(v) for k, v in t.items()}
    res = {}
    for m in modes:
        per = (med[(m, a.steps)] - med[(m, a.short)]) / (a.steps - a.short) * 1e3
        spread = (max(t[(m, a.steps)]) - min(t[(m, a.steps)])) / med[(m, a.steps)]
        res[m] = {'ms_per_step': round(per, 3), 'invert_ms': round(med[(m, a.steps)] * 1e3, 1), 'spread_pct': round(100 * spread, 2),
                  'launches_per_step': model.last_invert_plan['launches'] if m == list(modes)[-1] else None}
    res['fit']['ratio_to_frozen_beta'] = round(res['fit']['ms_per_step'] / res['frozen_beta']['ms_per_step'], 4)
    for m in modes:
        print(f"{m:>12}: {res[m]['ms_per_step']:.3f} ms per W+ step; invert({a.steps}) {res[m]['invert_ms']:.1f} ms (spread {res[m]['spread_pct']:.2f} %)")
    print(f"fit / frozen beta: {res['fit']['ratio_to_frozen_beta']:.4f}")
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=8)
    ap.add_argument('--size', type=int, default=1024)
    ap.add_argument('--mask', type=int, default=64)
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
        raise SystemExit('mask_fit_probe needs a GPU: a timing taken elsewhere says nothing')
    torch.set_num_threads(min(16, torch.get_num_threads()))
    dev = torch.device('cuda:0')
    res = {'batch': a.batch, 'size': a.size, 'mask_size': a.mask, 'launches_per_window': a.launches, 'rounds': a.rounds, 'streams': a.streams,
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
