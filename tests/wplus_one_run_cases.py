"""The cases that pin the W+ loop to the commit before its three ways of running a step (from Python, from a launch plan, from a
hipGraph) became one run class (engine._WRun): what tests/golden/make_wplus_one_run_parent.py records on that commit and
tests/test_hip_wplus_one_run.py recomputes.

Per case three runs — ``use_plan=False``, the default plan, ``use_graph=True`` — and per run the float32 bits of the returned losses, the
SHA-256 of the latents' bytes, ``last_stats`` and every dispatch counter of the library (which kernel family each conv went to, how often).
Only ``WPlusInverter``'s public surface is used, so the same code drives both commits."""
import hashlib

import numpy as np
import torch

from oodgan import synth

# size, B, streams, steps: the smallest shapes at which all three replay kinds, the carry path and the two-stream split are live
CASES = {'s32_b2': (32, 2, 1, 6), 's64_b3': (64, 3, 1, 6), 's64_b4_x2': (64, 4, 2, 6)}
MODES = {'python': (dict(use_plan=False), {}), 'plan': ({}, {}), 'graph': ({}, dict(use_graph=True))}
# g_dc_name of csrc/runtime.hip: every name oodgan_dispatch_count knows
COUNTERS = ('stripx', 'strip', 's1big', 's1v2', 's1pp', 'tiny', 't2big', 't2v2', 't2gen', 's2big', 's2v2', 's2gen', 'upvb', 's1big_ys',
            's2big_fuse', 's2big_dotx_sform', 's1big_g2', 's2big_g2', 'stripx_g2', 's2big_xh', 's1big_xh', 'composite_mse', 'ssim', 'robust',
            'area_pool')


def inputs(size, B, dev):
    """Engine, target, noises and start latents: the seeds of test_wplus_streams_and_graph_match_single_stream."""
    from oodgan.engine import GeneratorEngine
    eng = GeneratorEngine({k: v.to(dev) for k, v in synth.generator_state(size, seed=5).items()}, size)
    target = synth.make_images(size, B, seed=9).to(dev)
    noises = [n.to(dev) for n in synth.make_noises(size, B, seed=7)]
    w0 = synth.make_latents(size, B, seed=14).to(dev)
    return eng, target, noises, w0


def run_mode(eng, target, noises, w0, streams, steps, mode):
    """One run of one mode on a fresh inverter: (inverter, w, losses, dispatch counters of the run)."""
    from oodgan import _lib
    from oodgan.engine import WPlusInverter
    ctor, call = MODES[mode]
    inv = WPlusInverter(eng, **ctor)
    _lib.dispatch_reset()
    w, losses = inv.invert(target, w0, noises, steps=steps, streams=streams, **call)
    torch.cuda.synchronize()
    return inv, w, losses, np.array([_lib.dispatch_count(c) for c in COUNTERS], dtype=np.int64)


def record(name, dev):
    """{mode: dict(loss_bits uint32 (steps, B), w_sha 32 bytes, steps_run, rollbacks, counters)} of one case."""
    size, B, streams, steps = CASES[name]
    eng, target, noises, w0 = inputs(size, B, dev)
    out = {}
    for mode in MODES:
        inv, w, losses, counters = run_mode(eng, target, noises, w0, streams, steps, mode)
        out[mode] = dict(loss_bits=losses.detach().cpu().contiguous().numpy().view(np.uint32).copy(),
                         w_sha=np.frombuffer(hashlib.sha256(w.detach().cpu().contiguous().numpy().tobytes()).digest(), dtype=np.uint8),
                         steps_run=np.array(inv.last_stats['steps_run'], dtype=np.int64),
                         rollbacks=np.array(inv.last_stats['rollbacks'], dtype=np.int64), counters=counters)
    return out
