"""The pixel term on an antialiased resampled view (``pixel_filter``, csrc/loss_resample.hip).

The two kernels against float64 dense matrices (tests/resample_ref.py) with the same formula in torch's CPU fp32 as the yardstick, for the
three named filters and one random asymmetric table per factor and support (a flipped or transposed adjoint shows there); the bit
identities; the refusals; one W+ step's dL/dW+ against float64 autograd through the oracle; 20 steps against the reference's own autograd
loop on ``F.interpolate(antialias=True)`` (tests/golden/make_wplus_resample.py); launch plans, streams and the untouched default."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import ref_cpu as R  # noqa: E402
from oodgan import synth  # noqa: E402
import resample_ref as RR  # noqa: E402
from robust_ref import scale32  # noqa: E402
from wplus_grads import recover_grad  # noqa: E402


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


NAMED = {2: 'bilinear', 4: 'bicubic', 6: 'lanczos3'}
# (H, W) x F x s x B at C = 3.  32x32 at F = 16, s = 6 is a 2x2 view whose 96-tap windows are three times the image; 32x64 has different
# tables on the two axes; every case up to 64² is one partly filled tile per plane (a tile is 64 pixels wide, 128 at F = 16).  C = 1: the
# plane index without the channel.  128x128 at F = 2 and F = 4: 2 x 2 tiles per plane, so halo rows and columns come from another tile's
# pooled pixels and the image's interior borders are exercised in both kernels.
CASES = [(H, W, F, s, B, 3) for (H, W) in ((32, 32), (32, 64), (64, 64)) for F in (2, 4, 8, 16) for s in (2, 4, 6) for B in (1, 3)]
CASES += [(32, 64, 2, 4, 3, 1), (64, 64, 8, 6, 1, 1), (128, 128, 2, 6, 1, 3), (128, 128, 4, 4, 1, 3)]
KIND_SCALES = [('mse', 1.0)] + [(k, s) for k in RR.KINDS[1:] for s in (0.1, 1.0)]
_ids = lambda c: f'{c[0]}x{c[1]}-F{c[2]}-s{c[3]}-B{c[4]}-C{c[5]}'  # noqa: E731


@functools.lru_cache(maxsize=None)
def _random_taps(F, s):
    """One seeded asymmetric tap sequence per (F, s): positive (no row can lose its weight at a border), a ramp times noise."""
    g = torch.Generator().manual_seed(1000 * F + s)
    T = s * F
    return tuple(((0.25 + torch.rand(T, generator=g, dtype=torch.float64)) * torch.linspace(0.5, 1.5, T, dtype=torch.float64)).tolist())


def _tables(ops, dev, H, W, F, s, which):
    filt = NAMED[s] if which == 'named' else _random_taps(F, s)
    return ops.resample_tables(filt, H, F).to(dev), ops.resample_tables(filt, W, F).to(dev)


def _inputs(dev, H, W, F, B, C):
    img = synth.normal('resample.img', (B, C, H, W), 1)
    y = synth.normal('resample.y', (B, C, H // F, W // F), 2)
    return img, y, img.to(dev), y.to(dev)


# ------------------------------------------------------------------------------------------------------------- against float64
@pytest.mark.parametrize('case', CASES, ids=_ids)
def test_kernel_vs_float64(dev, case):
    """The view and r (max|d| over max|value|), the loss (relative) and the gradient (max|dg| / max|g|) within 4x the error of the same
    formula — dense matrices built from the same float32 tables — evaluated by torch in fp32 on the CPU.  The yardstick rule of DESIGN.md
    §20, applied as it is there: per case each quantity's figure is the largest over the case's tables, kinds and scales, and so is its
    yardstick.  Every figure is printed beside its yardstick."""
    from oodgan import ops
    H, W, F, s, B, C = case
    img, y, a, t = _inputs(dev, H, W, F, B, C)
    gmul = ops.loss_scale_for(C * H * W)
    worst = {q: [0.0, 0.0] for q in ('view', 'r', 'loss', 'gradient')}

    def check(what, got, ref64, ref32, rel_to):
        err = ((got.double().cpu() - ref64).abs() / rel_to).max().item()
        yard = ((ref32.double() - ref64).abs() / rel_to).max().item()
        print(f'{_ids(case)} {what}: {err:.2e} (the same formula in fp32 on the CPU: {yard:.2e})')
        q = worst[what.split()[-1]]
        q[0], q[1] = max(q[0], err), max(q[1], yard)

    for which in ('named', 'random'):
        Ay, Ax = _tables(ops, dev, H, W, F, s, which)
        assert Ay.shape == (H // F, s * F) and Ax.shape == (W // F, s * F)
        for kind, sc in KIND_SCALES:
            tag = f'{which} {kind} s={sc:g}'
            l64, g64, r64, v64 = RR.loss_and_grad(img, y, Ay, Ax, F, kind, sc, gmul)
            l32, g32, r32, v32 = RR.loss_and_grad(img, y, Ay, Ax, F, kind, sc, gmul, dtype=torch.float32)
            loss, g, psi = ops.resampled_pixel_loss_grad(a, t, Ay, Ax, F, kind, sc, gmul)
            assert loss.shape == (B,) and g.shape == a.shape and psi.shape == t.shape
            check(f'{tag} loss', loss, l64, l32, l64.abs())
            check(f'{tag} gradient', g, g64, g32, g64.abs().max())
            if kind == 'mse':
                check(f'{tag} r', psi, r64, r32, r64.abs().max())
                check(f'{tag} view', ops.resample_view(a, Ay, Ax, F), v64, v32, v64.abs().max())
    for q, (err, yard) in worst.items():
        print(f'{_ids(case)} worst {q}: {err:.2e} (yardstick {yard:.2e}, ratio {err / yard:.2f}, bar 4x)')
    assert all(err <= 4 * yard for err, yard in worst.values()), worst


# ------------------------------------------------------------------------------------------------------------- bit identities
@pytest.mark.parametrize('case', CASES, ids=_ids)
def test_kernel_bit_identities(dev, case):
    """A second call, grad=False and the table sink give the same bits; ``pixel_loss_grad(pool=, resample=)`` is the same call; the view of
    ``resample_view`` is the view inside the loss kernel: with y = 0 the square's psi is r = D(G) - 0, the view itself, bit for bit (for any
    other y, r + y is rounded once more than the view and says nothing bitwise)."""
    from oodgan import ops
    H, W, F, s, B, C = case
    _, _, a, t = _inputs(dev, H, W, F, B, C)
    gmul = ops.loss_scale_for(C * H * W)
    for which in ('named', 'random'):
        Ay, Ax = _tables(ops, dev, H, W, F, s, which)
        _, _, r0 = ops.resampled_pixel_loss_grad(a, torch.zeros_like(t), Ay, Ax, F, grad=False)
        v = ops.resample_view(a, Ay, Ax, F)
        assert torch.equal(r0, v) and torch.equal(ops.resample(a, Ay, Ax, F), v)
        full_target = synth.normal('resample.x', (B, C, H, W), 3).to(dev)
        for kind, sc in KIND_SCALES:
            loss, g, psi = ops.resampled_pixel_loss_grad(a, t, Ay, Ax, F, kind, sc, gmul)
            loss2, g2, psi2 = ops.resampled_pixel_loss_grad(a, t, Ay, Ax, F, kind, sc, gmul)
            assert torch.equal(loss2, loss) and torch.equal(g2, g) and torch.equal(psi2, psi), (which, kind, sc)
            l_fwd, g_none, psi3 = ops.resampled_pixel_loss_grad(a, t, Ay, Ax, F, kind, sc, gmul, grad=False)
            assert g_none is None and torch.equal(l_fwd, loss) and torch.equal(psi3, psi)
            l4, g4, none = ops.pixel_loss_grad(a, full_target, kind, sc, grad_mul=gmul, pool=F, resample=(Ay, Ax), target_pooled=t)
            assert none is None and torch.equal(l4, loss) and torch.equal(g4, g)
            table = torch.full((4, B), -1.0, device=dev)
            for row in (2, 9):
                row_dev = torch.tensor([row], dtype=torch.int32, device=dev)
                none, g5, _ = ops.pixel_loss_grad(a, full_target, kind, sc, grad_mul=gmul, pool=F, resample=(Ay, Ax), target_pooled=t, table=table,
                                                  row_dev=row_dev)
                assert none is None and torch.equal(table[min(row, 3)], loss) and torch.equal(g5, g)
            assert torch.equal(table[:2], torch.full((2, B), -1.0, device=dev))
        # the target's view left out: made here from the full target by the same kernel
        l6, g6, _ = ops.pixel_loss_grad(a, full_target, grad_mul=gmul, pool=F, resample=(Ay, Ax))
        l7, g7, _ = ops.resampled_pixel_loss_grad(a, ops.resample_view(full_target, Ay, Ax, F), Ay, Ax, F, grad_mul=gmul)
        assert torch.equal(l6, l7) and torch.equal(g6, g7)


def test_box_tables_give_the_area_pooled_term(dev):
    """The reduction §23 states: with box taps (s = 2, the middle F taps 1/F) the view is the area pool and the gradient gscale * psi on
    every pixel of a window, so the resampled term agrees with the fused box kernel of §20 to fp32 rounding."""
    from oodgan import ops
    B, C, H, W, F = 2, 3, 64, 32, 4
    _, _, a, _ = _inputs(dev, H, W, F, B, C)
    x = synth.normal('resample.x', (B, C, H, W), 3).to(dev)
    box = [0.0] * (F // 2) + [1.0] * F + [0.0] * (F // 2)
    Ay, Ax = ops.resample_tables(box, H, F).to(dev), ops.resample_tables(box, W, F).to(dev)
    gmul = ops.loss_scale_for(C * H * W)
    assert (ops.resample_view(a, Ay, Ax, F) - ops.area_pool(a, F)).abs().max().item() <= 1e-6
    for kind, sc in KIND_SCALES:
        l_box, g_box, _ = ops.pixel_loss_grad(a, x, kind, sc, grad_mul=gmul, pool=F)
        l_rs, g_rs, _ = ops.pixel_loss_grad(a, x, kind, sc, grad_mul=gmul, pool=F, resample=(Ay, Ax))
        assert ((l_rs - l_box).abs() / l_box).max().item() <= 1e-5, (kind, sc)
        assert (g_rs - g_box).abs().max().item() <= 1e-5 * g_box.abs().max().item(), (kind, sc)


# ------------------------------------------------------------------------------------------------------------- bad arguments
def test_bad_arguments_are_a_status_and_launch_nothing(dev):
    from oodgan import _lib, ops
    h, p = _lib.lib(), ops._p
    B, C, H, W, F, s = 2, 3, 16, 16, 4, 4
    a, y = torch.zeros(B, C, H, W, device=dev), torch.ones(B, C, 4, 4, device=dev)
    A = ops.resample_tables('bicubic', H, F).to(dev)
    g, rs = torch.full((B, C, H, W), -1.0, device=dev), torch.full((B, C, 4, 4), -1.0, device=dev)
    part, loss = torch.zeros(B, 8, device=dev), torch.full((B,), -1.0, device=dev)
    before = _lib.dispatch_count('resampled_pixel')

    def call(F=F, s=s, H=H, W=W, img=a, tview=y, Ay=A, Ax=A, kind=0, scale=0.5, B=B, C=C):
        return h.oodgan_resampled_pixel_loss_fwd_bwd(p(img), p(tview), p(Ay), p(Ax), p(g), p(rs), p(part), p(loss), B, C, H, W, F, s, kind, scale,
                                                     1.0, ops._stream())

    for word, kw in ((b'factor', dict(F=3)), (b'factor', dict(F=32)), (b'factor', dict(F=1)), (b'support', dict(s=3)), (b'support', dict(s=8)),
                     (b'multiple', dict(H=18)), (b'multiple', dict(F=8, W=20)), (b'tables', dict(Ay=None)), (b'tables', dict(Ax=None)),
                     (b'kind', dict(kind=4)), (b'kind', dict(kind=-1)), (b'scale', dict(kind=1, scale=0.0)),
                     (b'scale', dict(kind=3, scale=float('nan'))), (b'shape', dict(B=0)), (b'shape', dict(C=0)), (b'bad args', dict(img=None)),
                     (b'bad args', dict(tview=None))):
        assert call(**kw) == -1 and word in h.oodgan_last_error(), (kw, h.oodgan_last_error())
    out = torch.full((B * C, 4, 4), -1.0, device=dev)
    for word, kw in ((b'factor', dict(F=5)), (b'support', dict(s=5)), (b'multiple', dict(H=18)), (b'tables', dict(Ay=None)), (b'shape', dict(BC=0))):
        args = dict(BC=B * C, H=H, W=W, F=F, s=s, Ay=A)
        args.update(kw)
        assert h.oodgan_resample_fwd(p(a), p(args['Ay']), p(A), p(out), args['BC'], args['H'], args['W'], args['F'], args['s'], ops._stream()) == -1
        assert word in h.oodgan_last_error(), (kw, h.oodgan_last_error())
    torch.cuda.synchronize()
    assert (loss == -1.0).all() and (g == -1.0).all() and (rs == -1.0).all() and (out == -1.0).all()
    assert _lib.dispatch_count('resampled_pixel') == before
    assert call() == 0 and _lib.dispatch_count('resampled_pixel') == before + 1        # the same call with nothing wrong
    t = torch.ones(B, C, H, W, device=dev)
    w = torch.ones(B, 1, H, W, device=dev)
    with pytest.raises(ValueError, match='masked objective'):
        ops.pixel_loss_grad(a, t, beta=w, pool=F, resample=(A, A))
    with pytest.raises(ValueError, match='pool'):
        ops.pixel_loss_grad(a, t, resample=(A, A))
    with pytest.raises(ValueError, match='kind'):
        ops.pixel_loss_grad(a, t, 'l1', 0.5, pool=F, resample=(A, A))
    with pytest.raises(RuntimeError, match='scale'):
        ops.pixel_loss_grad(a, t, 'huber', 0.0, pool=F, resample=(A, A))
    with pytest.raises(ValueError, match='table'):
        ops.pixel_loss_grad(a, t, pool=F, resample=(A[:2], A))
    with pytest.raises(ValueError, match='target_view'):
        ops.pixel_loss_grad(a, t, pool=F, resample=(A, A), target_pooled=y[:, :, :2])


# ------------------------------------------------------------------------------------------------------- W+ step gradients
SIZE, PSIZE = 64, 16


def _step_inputs():
    """(generator state, target, noises, w0): the seeds of test_hip_pixel_size.py's 64² step tests."""
    B = 2
    return (synth.generator_state(SIZE, seed=5), synth.make_images(SIZE, B, seed=9), synth.make_noises(SIZE, B, seed=7),
            synth.make_latents(SIZE, B, seed=14))


@functools.lru_cache(maxsize=None)
def _oracle_step(filt, kind):
    """dL/dW+ and the per-image loss of the first step through the oracle in float64 — the view by the dense float64 matrices of the
    definition, not by the float32 tables — and the oracle's own float32-vs-float64 distance of that gradient (relative to its max).
    Computed once and shared by the precisions."""
    P, target, noises, w0 = _step_inputs()
    s, F = scale32(1.0), SIZE // PSIZE
    D64 = RR.dense_from_taps(filt, SIZE, F)

    def run(dt):
        D = D64.to(dt)
        w = w0.to(dt).clone().requires_grad_(True)
        img = R.generator_forward({k: v.to(dt) for k, v in P.items()}, w, [n.to(dt) for n in noises], SIZE)
        r = RR.view(img, D, D) - RR.view(target.to(dt), D, D)
        loss = RR.rho(r, kind, s).mean(dim=(1, 2, 3))
        loss.sum().backward()
        return w.grad.double(), loss.detach().double()

    g64, l64 = run(torch.float64)
    g32, _ = run(torch.float32)
    return g64, l64, (g32 - g64).abs().max().item() / g64.abs().max().item()


@pytest.mark.parametrize('prec,bar', [('f16s', 1e-4), ('f16s-g2', 3e-4)])
@pytest.mark.parametrize('kind', ['mse', 'charbonnier'])
@pytest.mark.parametrize('filt', ['bicubic', 'lanczos3'])
def test_wplus_step_64_vs_float64_autograd(dev, filt, kind, prec, bar):
    """pixel_size=16 at 64² (factor 4), s = 1: the step's dL/dW+, recovered from Adam's first moment, within the project's bar of §20 (the
    oracle's own fp32-vs-float64 distance is printed beside it); the loss within 1e-5."""
    from oodgan import _lib
    from oodgan.engine import GeneratorEngine, WPlusInverter
    P, target, noises, w0 = _step_inputs()
    g64, l64, e_self = _oracle_step(filt, kind)
    eng = GeneratorEngine({k: v.to(dev) for k, v in P.items()}, SIZE, precision=prec)
    inv = WPlusInverter(eng, pixel_loss=kind, pixel_scale=1.0, pixel_size=PSIZE, pixel_filter=filt)
    caps = {}
    inv.on_step = lambda run: caps.__setitem__(run.t, run.m.clone())
    _lib.dispatch_reset()
    _, losses = inv.invert(target.to(dev), w0.to(dev), [n.to(dev) for n in noises], steps=1)
    torch.cuda.synchronize()
    assert inv.last_stats['rollbacks'] == [0]
    assert _lib.dispatch_count('resampled_pixel') == 1 and _lib.dispatch_count('pooled_pixel') == 0 and _lib.dispatch_count('robust') == 0
    g = recover_grad(torch.zeros_like(caps[1]).cpu(), caps[1].cpu(), inv.betas[0])
    rel = (g - g64).abs().max().item() / g64.abs().max().item()
    e_loss = ((losses[0].double().cpu() - l64).abs() / l64).max().item()
    print(f'{kind} pixel_size={PSIZE} {filt} W+ step {SIZE}² {prec}: dL/dW+ rel {rel:.2e} (bar {bar:g}; oracle f32 vs f64 {e_self:.2e}), '
          f'loss rel {e_loss:.2e}')
    assert rel < bar and e_loss < 1e-5


# ------------------------------------------------------------------------------------------------------- the reference's own loop
@pytest.mark.parametrize('run', ['derived', 'given'])
def test_loop_256_vs_reference(dev, golden, run):
    """20 steps at 256², B = 2, pixel_size=64, pixel_filter='bicubic', the square: the loss curve against the reference Generator's autograd
    + torch.optim.Adam on ``F.interpolate(., antialias=True)`` in float32 within 1e-3 relative on every step — with the target's view
    derived from x, and with a seeded 64² ``pixel_target`` given at its own size; the fixture's own fp32-vs-float64 figure beside it."""
    from oodgan.engine import GeneratorEngine, WPlusInverter
    g = golden('wplus_resample_256.npz')
    steps, F = int(g['steps']), int(g['factor'])
    _, sx, sn, sw, sy = g['seeds'].tolist()
    size, B = 256, 2
    eng = GeneratorEngine({k: v.to(dev) for k, v in synth.generator_state(size, seed=0).items()}, size)
    x = synth.make_images(size, B, seed=sx).to(dev)
    noises = [n.to(dev) for n in synth.make_noises(size, B, seed=sn)]
    w0 = synth.make_latents(size, B, seed=sw, std=0.3).to(dev)
    given = run == 'given'
    y = synth.make_images(size // F, B, seed=sy).to(dev) if given else None
    inv = WPlusInverter(eng, pixel_size=None if given else size // F, pixel_filter='bicubic')
    w, losses = inv.invert(x, w0, noises, steps=steps, pixel_target=y)
    l32, l64 = g[f'{run}_losses_f32'], g[f'{run}_losses_f64']
    e_curve = ((losses.double().cpu() - l32).abs() / l32).max().item()
    e_fix = ((l32 - l64).abs() / l64).max().item()
    e_w = (w.cpu() - g[f'{run}_w_step{steps}']).abs().max().item()
    print(f'{run} target, bicubic pixel_size={size // F} at 256², {steps} steps: loss curve rel {e_curve:.2e} (the fixture\'s own fp32 vs float64: '
          f'{e_fix:.2e}); |w_{steps} - reference w_{steps}| {e_w:.2e}; loss {losses[0].tolist()} -> {losses[-1].tolist()}')
    assert e_curve <= 1e-3
    assert (losses[-1] < losses[0]).all()
    assert inv.last_terms['pixel'] is not None and inv.last_terms['mse'] is inv.last_terms['pixel']


# ------------------------------------------------------------------------------------------------------- plans, streams, default, refusals
def _loop_inputs(dev, size, B, seed):
    eng_state = {k: v.to(dev) for k, v in synth.generator_state(size, seed=5 if size == 64 else 0).items()}
    target = synth.make_images(size, B, seed=seed).to(dev)
    noises = [n.to(dev) for n in synth.make_noises(size, B, seed=seed + 1)]
    w0 = synth.make_latents(size, B, seed=seed + 2, std=0.3).to(dev)
    return eng_state, target, noises, w0


@pytest.mark.parametrize('kind,filt,given', [('mse', 'bicubic', False), ('charbonnier', 'lanczos3', False), ('mse', 'bilinear', True)],
                         ids=['mse-bicubic', 'charbonnier-lanczos3', 'mse-bilinear-given'])
def test_plans_and_streams(dev, kind, filt, given):
    """The recorded plan, the Python-driven loop and the run that returns its trajectory agree bit for bit; a recorded step with
    pixel_filter is exactly one launch longer than the box pixel_size step (kernel one, the finish, kernel two against the fused kernel and
    the finish); two streams against one within 5e-3 (the same comparison with the box is printed).  ``given``: with a pixel_target, which
    the streams slice like the target."""
    from oodgan.engine import GeneratorEngine, WPlusInverter
    B, steps = 4, 12
    state, target, noises, w0 = _loop_inputs(dev, SIZE, B, 171)
    eng = GeneratorEngine(state, SIZE)
    y = synth.make_images(PSIZE, B, seed=175).to(dev) if given else None
    kw = dict(pixel_loss=kind, pixel_scale=0.5, pixel_size=PSIZE)
    inv = WPlusInverter(eng, use_plan=True, pixel_filter=filt, **kw)
    w1, l1 = inv.invert(target, w0, noises, steps=steps, pixel_target=y)
    plan1 = inv.last_plan
    assert plan1['steps'] == [steps - 3] and inv.last_stats['rollbacks'] == [0]
    assert (inv.last_terms['mse'] is not None) == (kind == 'mse') and inv.last_terms['pixel'].shape == (steps, B)
    inv2 = WPlusInverter(eng, use_plan=False, pixel_filter=filt, **kw)
    w2, l2 = inv2.invert(target, w0, noises, steps=steps, pixel_target=y)
    assert inv2.last_plan['steps'] == [0] and torch.equal(w1, w2) and torch.equal(l1, l2)
    w3, l3, traj = inv.invert(target, w0, noises, steps=steps, return_trajectory=True, pixel_target=y)
    assert torch.equal(w1, w3) and torch.equal(l1, l3) and len(traj) == steps and torch.equal(traj[-1], w1)
    box = WPlusInverter(eng, use_plan=True, **kw)
    _, m1 = box.invert(target, w0, noises, steps=steps, pixel_target=y)
    assert box.last_plan['steps'] == plan1['steps'] and plan1['launches'][0] == box.last_plan['launches'][0] + 1
    assert not torch.equal(m1, l1)
    w4, l4 = inv.invert(target, w0, noises, steps=steps, streams=2, pixel_target=y)
    assert inv.last_plan['steps'] == [steps - 3] * 2 and inv.last_stats['rollbacks'] == [0, 0]
    _, m2 = box.invert(target, w0, noises, steps=steps, streams=2, pixel_target=y)
    rel, r_ref = ((l4 - l1).abs() / l1.abs()).max().item(), ((m2 - m1).abs() / m1.abs()).max().item()
    print(f'{kind} {filt}{" + pixel_target" if given else ""} pixel_size={PSIZE}, 2 streams vs 1 at {SIZE}², B={B}: loss rel diff {rel:.2e} (box: '
          f'{r_ref:.2e}); plan {plan1} (box: {box.last_plan})')
    assert rel <= 5e-3
    assert (l1[-1] < l1[0]).all()


def _counters():
    from oodgan import _lib
    import wplus_one_run_cases as C
    return {c: _lib.dispatch_count(c) for c in C.COUNTERS + ('pooled_pixel', 'pn', 'resampled_pixel')}


def test_parent_paths_are_unchanged(dev):
    """pixel_filter None and 'box' give the bits, the launch count and the dispatch counters of the call without the argument — at the
    image's own size and with the box pixel_size; a box pixel_target equal to the pooled target is the derived run bit for bit."""
    from oodgan import _lib, ops
    from oodgan.engine import GeneratorEngine, WPlusInverter
    B, steps = 2, 6
    state, target, noises, w0 = _loop_inputs(dev, SIZE, B, 191)
    eng = GeneratorEngine(state, SIZE)
    for ps in (None, PSIZE):
        _lib.dispatch_reset()
        base = WPlusInverter(eng, pixel_size=ps)
        w_b, l_b = base.invert(target, w0, noises, steps=steps)
        c_b = _counters()
        assert c_b['resampled_pixel'] == 0 and (c_b['pooled_pixel'] > 0) == (ps is not None)
        for pf in (None, 'box'):
            _lib.dispatch_reset()
            inv = WPlusInverter(eng, pixel_size=ps, pixel_filter=pf)
            w1, l1 = inv.invert(target, w0, noises, steps=steps)
            assert torch.equal(w1, w_b) and torch.equal(l1, l_b) and inv.last_plan == base.last_plan and _counters() == c_b, (ps, pf)
    yt = ops.area_pool(target, SIZE // PSIZE)
    _lib.dispatch_reset()
    inv = WPlusInverter(eng, pixel_filter='box')
    w2, l2 = inv.invert(target, w0, noises, steps=steps, pixel_target=yt)
    want = dict(c_b, area_pool=c_b['area_pool'] - 1)                # the run no longer pools the target itself
    assert torch.equal(w2, w_b) and torch.equal(l2, l_b) and inv.last_plan == base.last_plan and _counters() == want


def test_refusals(dev):
    """What the option does not take, refused before anything is launched."""
    from oodgan import _lib
    from oodgan.engine import GeneratorEngine, WPlusInverter
    B, steps = 2, 4
    state, target, noises, w0 = _loop_inputs(dev, SIZE, B, 201)
    eng = GeneratorEngine(state, SIZE)
    y = synth.make_images(PSIZE, B, seed=205).to(dev)
    beta = torch.ones(B, 1, SIZE, SIZE, device=dev)
    _lib.dispatch_reset()
    with pytest.raises(NotImplementedError, match='pixel'):
        WPlusInverter(eng, pixel_size=PSIZE, pixel_filter='bicubic').invert(target, w0, noises, steps=steps, use_graph=True)
    with pytest.raises(ValueError, match='loss weight'):
        WPlusInverter(eng, pixel_size=PSIZE, pixel_filter='bicubic').invert(target, w0, noises, steps=steps, loss_weight=beta)
    with pytest.raises(ValueError, match='loss weight'):
        WPlusInverter(eng).invert(target, w0, noises, steps=steps, loss_weight=beta, pixel_target=y)
    with pytest.raises(ValueError, match='pixel_size'):
        WPlusInverter(eng, pixel_filter='bicubic').invert(target, w0, noises, steps=steps)                       # no view to filter
    with pytest.raises(ValueError, match='pixel_size'):
        WPlusInverter(eng, pixel_size=32, pixel_filter='bicubic').invert(target, w0, noises, steps=steps, pixel_target=y)   # 32 != 16
    for bad in (y[:1], y.double(), y.cpu(), y[:, :, :8], synth.make_images(SIZE, B, seed=1).to(dev), synth.make_images(24, B, seed=1).to(dev)):
        with pytest.raises(ValueError, match='pixel_target'):
            WPlusInverter(eng, pixel_filter='bicubic').invert(target, w0, noises, steps=steps, pixel_target=bad)
    assert _lib.dispatch_count('resampled_pixel') == 0


def test_model_invert_and_cli_pixel_target(dev):
    """``invert(pixel_filter=, pixel_target=)`` on the model: checked before anything runs; a target given at its own size runs the
    resampled kernels while x stays the full-size input; the CLI's ``pixel_target: file`` helper converts without a resize and refuses
    mixed sizes and a full-size file."""
    import numpy as np
    from oodgan import _lib, cli, imgio
    from oodgan.arch import ood_faceGAN_e4e
    size, B = 256, 2
    m = ood_faceGAN_e4e(out_size=size, style_dim=512, encoder='E4E', enable_modulation=True, warp_scale=0.08, cycle_align=2, blend_with_gen=True,
                        ModSize=256, build_encoder=False)
    res = m.load_state_dict(synth.ood_state(size, seed=41), strict=False)
    assert not res.missing_keys and not res.unexpected_keys, res
    m = m.to(dev).eval()
    x = synth.make_images(size, B, seed=44).to(dev)
    y = synth.make_images(64, B, seed=46).to(dev)
    kw = dict(enc_lats=synth.make_latents(size, B, seed=42, std=0.3).to(dev), enc_feats=[f.to(dev) for f in synth.make_encoder_feats(B, seed=43)],
              noise=[n.to(dev) for n in synth.make_noises(size, B, seed=45)])
    for bad in ('lanczos', 'nearest', 3, True):
        with pytest.raises(ValueError, match='pixel_filter'):
            m.invert(x, steps=2, pixel_size=64, pixel_filter=bad, **kw)
    with pytest.raises(ValueError, match='pixel_size'):
        m.invert(x, steps=2, pixel_filter='bicubic', **kw)
    with pytest.raises(ValueError, match='pixel_size'):
        m.invert(x, steps=2, pixel_size=128, pixel_target=y, **kw)
    with pytest.raises(ValueError, match='loss_region'):
        m.invert(x, steps=2, pixel_size=64, pixel_filter='bicubic', loss_region='blend', **kw)
    with pytest.raises(NotImplementedError):
        m.invert(x, steps=2, pixel_size=64, pixel_filter='bicubic', use_graph=True, **kw)
    _lib.dispatch_reset()
    _, _, l_box = m.invert(x, steps=6, pixel_size=64, **kw)
    plan_box = m.last_invert_plan
    assert _lib.dispatch_count('resampled_pixel') == 0
    out, lats, l1 = m.invert(x, steps=6, pixel_filter='lanczos3', pixel_target=y, **kw)
    assert _lib.dispatch_count('resampled_pixel') >= 1 and out.shape == x.shape and torch.isfinite(out).all() and torch.isfinite(l1).all()
    assert plan_box['launches'][0] > 0 and m.last_invert_plan['launches'][0] == plan_box['launches'][0] + 1 and m.last_loss_terms['mse'] is m.last_loss_terms['pixel']
    assert not torch.equal(l1, l_box)
    # the CLI helper: the file's own pixels, converted as the input is
    rng = np.random.RandomState(3)
    small = [rng.randint(0, 256, (64, 64, 3)).astype(np.uint8) for _ in range(B)]
    t_host = cli.pixel_target_from_files([s.astype(np.float64) for s in small], ['a.png', 'b.png'], size)
    t_dev = cli.pixel_target_from_files([torch.from_numpy(s).to(dev) for s in small], ['a.png', 'b.png'], size)
    assert t_host.shape == (B, 3, 64, 64) and torch.equal(t_host, t_dev)
    assert torch.equal(t_host, torch.cat([imgio.image_to_input(s.astype(np.float64), 64, device='cuda') for s in small], 0))
    big = rng.randint(0, 256, (size, size, 3)).astype(np.float64)
    for bad, word in (([small[0].astype(np.float64), big], 'one size'), ([big, big], 'generator size'),
                      ([np.zeros((64, 32, 3))] * 2, 'square'), ([np.zeros((96, 96, 3))] * 2, 'side n')):
        with pytest.raises(ValueError, match=word):
            cli.pixel_target_from_files(bad, ['a.png', 'b.png'], size)
