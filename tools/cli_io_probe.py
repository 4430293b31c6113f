#!/usr/bin/env python3
"""Wall time per image of the command-line tool, files in to files out — what ``bench.py`` does not measure.

Writes --files seeded 1024² PNGs (smoothed noise: the encoder's cost resembles a photo's, not white noise's) and a seeded checkpoint built
as tests/test_cli.py builds it, then runs ``oodgan.cli.run`` with --steps W+ steps, batch --batch, --streams streams and PSNR + SSIM at
crop 2, each LEG in a fresh child process under its own ``timeout``.  A leg is ``this`` (this checkout) or ``tree`` (the checkout --tree
names, with its own built library: the parent commit), optionally with ``:io=host`` / ``:io_workers=N``.  The default legs with --tree are
tree, this, tree, this, this:io_workers=8 — interleaved, so a drift of the box hits both alike; the median of each kind is reported.
Every leg runs two data sets: ``warm`` (the first --batch files: code objects, allocator, launch plans) and ``timed`` (all files).  Wall
per image of ``timed`` is taken by the child from the call that lists its files to the return of ``run``, the same way for a tree whose
summary has no ``wall`` key; ``time`` per image is the summary's (the model call only).  A leg that fails ends the probe.

    python tools/cli_io_probe.py [--tree PATH] [--legs a,b,...] [--files 16] [--steps 100] [--batch 8] [--streams 2] [--leg-timeout 400]
                                 [--commit LABEL] [--tree-commit LABEL] [--work DIR] [--out profiles/cli_io_timing.json]
"""
import argparse
import json
import os
import platform
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZE = 1024


def child(tree, opt_path, result_path):
    """One leg: ``cli.run`` of the checkout ``tree`` on the options file; the result as JSON."""
    sys.path.insert(0, os.path.join(tree, 'ood-gan-inversion_amd'))
    import yaml
    from oodgan import cli
    with open(opt_path) as f:
        opts = yaml.load(f, Loader=yaml.FullLoader)
    started = {}
    list_files = cli.load_files_from_path

    def stamped(dopt, directions_dir=None):
        started[os.path.basename(dopt['dataroot'])] = time.time()
        return list_files(dopt, directions_dir)

    cli.load_files_from_path = stamped
    summary = cli.run(opts)
    end = time.time()
    assert started['warm'] < started['timed'], 'the warm data set must run first'
    n = summary['timed']['n']
    res = {'wall_per_image': (end - started['timed']) / n, 'time_per_image': summary['timed']['time'], 'n': n,
           'summary_wall_per_image': summary['timed'].get('wall'), 'psnr': summary['timed']['psnr'], 'ssim': summary['timed']['ssim'],
           'warm_wall_per_image': (started['timed'] - started['warm']) / summary['warm']['n']}
    with open(result_path, 'w') as f:
        json.dump(res, f)


def make_inputs(work, files, batch):
    """The PNGs (``timed`` holds all, ``warm`` the first ``batch``) and the checkpoint; returns the ``network_g`` / ``path`` option blocks."""
    sys.path.insert(0, os.path.join(ROOT, 'ood-gan-inversion_amd'))
    import numpy as np
    import torch
    from oodgan import imgio, synth
    from oodgan.arch import ood_faceGAN_e4e
    rng = np.random.default_rng(2024)
    for i in range(files):
        a = rng.standard_normal((SIZE, SIZE, 3))
        for axis in (0, 1):                     # a 9-tap box filter, three times per axis: close to a Gaussian of sigma 4.5
            for _ in range(3):
                a = sum(np.roll(a, s, axis) for s in range(-4, 5)) / 9.0
        a = (a - a.min()) / (a.max() - a.min())
        img = np.round(255.0 * a).astype(np.uint8)
        for name in (['timed', 'warm'] if i < batch else ['timed']):
            imgio.imwrite(os.path.join(work, name, f'{i:05d}.png'), img)
    net = {'type': 'ood_faceGAN_e4e', 'out_size': SIZE, 'style_dim': 512, 'encoder': 'E4E', 'enable_modulation': True, 'warp_scale': 0.08,
           'cycle_align': 2, 'blend_with_gen': True, 'ModSize': 256}
    m = ood_faceGAN_e4e(**{k: v for k, v in net.items() if k != 'type'})
    sd = synth.ood_state(SIZE, seed=31)
    enc = synth.encoder_state({k: tuple(v.shape) for k, v in m.encoder.state_dict().items()}, seed=41)
    sd.update({'encoder.' + k: (v * 0.1 if k.endswith('linear.weight') else v) for k, v in enc.items()})
    torch.save({'params_ema': sd}, os.path.join(work, 'net_g.pth'))
    return net, {'pretrain_network_g': os.path.join(work, 'net_g.pth'), 'param_key_g': 'params_ema', 'strict_load_g': False}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--tree', default=None, help='another checkout (built) for the "tree" legs')
    ap.add_argument('--legs', default=None, help='comma-separated: this | tree, each optionally :io=host|device and/or :io_workers=N')
    ap.add_argument('--files', type=int, default=16)
    ap.add_argument('--steps', type=int, default=100)
    ap.add_argument('--batch', type=int, default=8)
    ap.add_argument('--streams', type=int, default=2)
    ap.add_argument('--leg-timeout', type=int, default=400, help='seconds per leg')
    ap.add_argument('--commit', default=None, help='label of this checkout in the output (default: git rev-parse, if it is a repository)')
    ap.add_argument('--tree-commit', default=None, help='label of --tree in the output')
    ap.add_argument('--work', default=None, help='directory for inputs and outputs (default: a temporary one)')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'cli_io_timing.json'))
    ap.add_argument('--child', nargs=3, metavar=('TREE', 'OPT', 'RESULT'), help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(*a.child)
    import yaml
    legs = a.legs.split(',') if a.legs else (['tree', 'this', 'tree', 'this', 'this:io_workers=8'] if a.tree else ['this', 'this:io_workers=8'])
    if any(leg.split(':')[0] not in ('this', 'tree') for leg in legs) or (a.tree is None and any(leg.startswith('tree') for leg in legs)):
        ap.error('--legs: each leg is "this" or "tree" (the latter needs --tree)')
    commit = a.commit
    if commit is None:
        r = subprocess.run(['git', '-C', ROOT, 'rev-parse', '--short', 'HEAD'], capture_output=True, text=True)
        commit = r.stdout.strip() if r.returncode == 0 else 'unknown'
    tmp = None if a.work else tempfile.TemporaryDirectory(prefix='cli_io_probe_')
    work = os.path.abspath(a.work or tmp.name)
    os.makedirs(work, exist_ok=True)
    net, path = make_inputs(work, a.files, a.batch)
    metrics = {k: {'crop_border': 2, 'test_y_channel': False} for k in ('psnr', 'ssim')}
    results = []
    for i, leg in enumerate(legs):
        kind, *extra = leg.split(':')
        inv = {'wplus_steps': a.steps, 'batch': a.batch, 'streams': a.streams}
        for kv in extra:
            k, v = kv.split('=')
            inv[k] = int(v) if k == 'io_workers' else v
        opts = {'name': f'leg{i}', 'save_dir': os.path.join(work, 'results'), 'directions_dir': os.path.join(work, 'directions'),
                'datasets': {'warm': {'dataroot': os.path.join(work, 'warm')}, 'timed': {'dataroot': os.path.join(work, 'timed')}},
                'network_g': net, 'path': path, 'metrics': metrics, 'inversion': inv}
        opt_path, res_path = os.path.join(work, f'leg{i}.yml'), os.path.join(work, f'leg{i}.json')
        with open(opt_path, 'w') as f:
            yaml.safe_dump(opts, f, sort_keys=False)           # the data sets run in this order: warm, then timed
        tree = os.path.abspath(a.tree) if kind == 'tree' else ROOT
        t0 = time.time()
        r = subprocess.run(['timeout', '-k', '10', str(a.leg_timeout), sys.executable, os.path.abspath(__file__), '--child', tree, opt_path, res_path])
        if r.returncode != 0:
            print(f'leg {i} ({leg}) ended with status {r.returncode}: stopping', file=sys.stderr)
            return r.returncode
        with open(res_path) as f:
            res = json.load(f)
        res.update(leg=leg, tree=kind, commit=(a.tree_commit or 'unknown') if kind == 'tree' else commit, process_seconds=round(time.time() - t0, 1))
        print(json.dumps(res), flush=True)
        results.append(res)
    import torch
    medians = {}
    for leg in dict.fromkeys(legs):
        rs = [r for r in results if r['leg'] == leg]
        medians[leg] = {'wall_per_image': statistics.median(r['wall_per_image'] for r in rs),
                        'time_per_image': statistics.median(r['time_per_image'] for r in rs), 'legs': len(rs)}
    out = {'what': f'tools/cli_io_probe.py: oodgan.cli.run on {a.files} seeded 1024x1024 PNGs, {a.steps} W+ steps, batch {a.batch}, {a.streams} streams, '
                   'psnr + ssim at crop 2; seconds per image of the timed data set; wall = files in to files out, time = the model call only',
           'box': platform.node(), 'gpu': torch.cuda.get_device_name(0) if torch.cuda.is_available() else None, 'legs': results, 'median': medians}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(out, f, indent=1)
    print(json.dumps(medians))
    return 0


if __name__ == '__main__':
    sys.exit(main())
