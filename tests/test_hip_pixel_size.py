"""The pixel term on an area-pooled view (``pixel_size``, csrc/loss_pixel.hip: pooled_pixel_kernel).

The fused kernel bit for bit against the composition it replaces (area_pool, the unpooled pixel term at the small size, area_pool_bwd_add)
and, with a loss weight, against the area pool of the elementwise product; against float64 (tests/pixsize_ref.py) with the same formula in
torch's CPU fp32 as the yardstick; its refusals; one W+ step's dL/dW+ against float64 autograd through the oracle; 20 steps against the
reference's own autograd loop (tests/golden/make_wplus_pixsize.py); launch plans, streams, the untouched default and the refusals."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import ref_cpu as R  # noqa: E402
from oodgan import synth  # noqa: E402
import pixsize_ref as PR  # noqa: E402
from robust_ref import scale32  # noqa: E402
from wplus_grads import recover_grad  # noqa: E402


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


def _beta(B, H, W, seed):
    """A seeded, non-binary plane in [0, 1] with an exact-zero and an exact-one block."""
    b = torch.sigmoid(2.0 * synth.normal('pixsize.beta', (B, 1, H, W), seed))
    b[:, :, : H // 4, : W // 4] = 0.0
    b[:, :, -(H // 4):, -(W // 4):] = 1.0
    return b.contiguous()


# (H, W) x f x B at C = 3: 32x32 with f = 16 is a 2x2 pooled image in one partly filled block; 64x64 with f = 2 takes three blocks without a
# loss weight.  With a loss weight C = 3 takes the three-plane form up to f = 8 and the one-plane form at f = 16; C = 1: the one-plane form
# at the small factors (float2 rows; the row-by-row summing pass of f = 8).  128x128: more than one block of the three-plane form (4096 and
# 1024 pooled positions against 1024 and 512 per block).
CASES = [(H, W, f, B, 3) for (H, W) in ((64, 64), (32, 32), (32, 64)) for f in (2, 4, 8, 16) for B in (1, 3)]
CASES += [(32, 64, 2, 3, 1), (64, 64, 8, 1, 1), (128, 128, 2, 1, 3), (128, 128, 4, 1, 3)]
# every kind at both scales (the square has none): residuals of order 1 lie on both sides of s = 1.0 and mostly beyond s = 0.1
KIND_SCALES = [('mse', 1.0)] + [(k, s) for k in PR.KINDS[1:] for s in (0.1, 1.0)]
_ids = lambda c: f'{c[0]}x{c[1]}-f{c[2]}-B{c[3]}-C{c[4]}'  # noqa: E731


def _inputs(dev, H, W, B, C):
    img = synth.normal('pixsize.img', (B, C, H, W), 1)
    x = synth.normal('pixsize.x', (B, C, H, W), 2)
    beta = _beta(B, H, W, 3)
    return img, x, beta, img.to(dev), x.to(dev), beta.to(dev)


def _residuals(ops, a, t, w, f, ts):
    """The pooled residuals as the kernel formed them, read through the square kind's gradient at gscale = 1 (grad_mul = CHW/2, exact):
    (r without beta, r with beta); every pixel of a window must hold its window's value."""
    unit = a[0].numel() / 2.0
    out = []
    for kw in (dict(target_pooled=ts), dict(beta=w, wrt='composite')):
        _, g, _ = ops.pixel_loss_grad(a, t, grad_mul=unit, pool=f, **kw)
        r = g[:, :, ::f, ::f].contiguous()
        assert torch.equal(PR.unpool(r, f), g)
        out.append(r)
    return out


# ------------------------------------------------------------------------------------------------------------- bit identities
@pytest.mark.parametrize('case', CASES, ids=_ids)
def test_kernel_bit_identities(dev, case):
    """Without a loss weight: r and the gradient equal the composition area_pool(G), area_pool(x) -> pixel_loss_grad at the small size ->
    area_pool_bwd_add into zeros, bit for bit (every scale that differs between the two routes is a power of two).  With one: r equals
    area_pool of the elementwise beta*(G - x), the composite equals the unpooled entry's.  grad=False, a second call and the table sink
    give the same bits."""
    from oodgan import ops
    H, W, f, B, C = case
    _, _, _, a, t, w = _inputs(dev, H, W, B, C)
    gmul = ops.loss_scale_for(C * H * W)
    a_s, ts = ops.area_pool(a, f), ops.area_pool(t, f)
    r, rb = _residuals(ops, a, t, w, f, ts)
    assert torch.equal(r, a_s - ts)
    assert torch.equal(rb, ops.area_pool((w * (a - t)).contiguous(), f))
    for kind, s in KIND_SCALES:
        loss, g, none = ops.pixel_loss_grad(a, t, kind, s, grad_mul=gmul, pool=f, target_pooled=ts)
        assert none is None and g.shape == a.shape and loss.shape == (B,)
        _, g_small, _ = ops.pixel_loss_grad(a_s, ts, kind, s, grad_mul=gmul)
        assert torch.equal(g, ops.area_pool_bwd_add(g_small, torch.zeros_like(a), f)), (kind, s)
        loss2, g2, _ = ops.pixel_loss_grad(a, t, kind, s, grad_mul=gmul, pool=f)                 # pools the target itself; a second call
        assert torch.equal(loss2, loss) and torch.equal(g2, g)
        l_fwd, g_none, _ = ops.pixel_loss_grad(a, t, kind, s, grad_mul=gmul, pool=f, target_pooled=ts, grad=False)
        assert g_none is None and torch.equal(l_fwd, loss)
        # with a loss weight
        lb, gg, c = ops.pixel_loss_grad(a, t, kind, s, w, gmul, wrt='gen', composite=True, pool=f)
        lb2, gc, c2 = ops.pixel_loss_grad(a, t, kind, s, w, gmul, wrt='composite', pool=f)
        assert c2 is None and torch.equal(lb2, lb)
        _, _, c_full = ops.pixel_loss_grad(a, t, kind, s, w, gmul, composite=True)
        assert torch.equal(c, c_full), (kind, s)
        l_fwd, g_none, c_fwd = ops.pixel_loss_grad(a, t, kind, s, w, gmul, composite=True, pool=f, grad=False)
        assert g_none is None and torch.equal(l_fwd, lb) and torch.equal(c_fwd, c)
        lb3, gg3, c3 = ops.pixel_loss_grad(a, t, kind, s, w, gmul, wrt='gen', composite=True, pool=f)
        assert torch.equal(lb3, lb) and torch.equal(gg3, gg) and torch.equal(c3, c)
        # the loss-table form writes row min(row_dev[0], nrows - 1) and no other
        for kw, want_l, want_g in ((dict(target_pooled=ts), loss, g), (dict(beta=w), lb, gg)):
            table = torch.full((4, B), -1.0, device=dev)
            for row in (2, 9):
                row_dev = torch.tensor([row], dtype=torch.int32, device=dev)
                none, g4, _ = ops.pixel_loss_grad(a, t, kind, s, grad_mul=gmul, pool=f, table=table, row_dev=row_dev, **kw)
                assert none is None and torch.equal(table[min(row, 3)], want_l) and torch.equal(g4, want_g)
            assert torch.equal(table[:2], torch.full((2, B), -1.0, device=dev))


# ------------------------------------------------------------------------------------------------------------- against float64
@pytest.mark.parametrize('case', CASES, ids=_ids)
def test_kernel_vs_float64(dev, case):
    """r element by element within the any-order summation bound (f^2 + 2) * 2^-24 * mean_window|terms|; the loss (relative), the gradient
    (max|dg| / max|g|) and the composite (max|dc|) within 4x the error of the same formula evaluated by torch in fp32 on the CPU.  The
    yardstick rule of tests/test_hip_sspace.py, applied as it is there: per case — a shape, factor and batch — each quantity's figure is the
    largest over the case's images, kinds, scales and forms, and so is its yardstick (a single image's loss is one fp32 number: its CPU
    value may happen to be the correctly rounded one, 1.7e-9 off where the format's half-ulp is 6e-8, and says nothing alone).  Every
    figure is printed beside its yardstick."""
    from oodgan import ops
    H, W, f, B, C = case
    img, x, beta, a, t, w = _inputs(dev, H, W, B, C)
    gmul = ops.loss_scale_for(C * H * W)
    ts = ops.area_pool(t, f)
    for r, bt in zip(_residuals(ops, a, t, w, f, ts), (None, beta)):
        r64 = PR.residual(img.double(), x.double(), f, None if bt is None else bt.double())
        bound = (f * f + 2) * 2.0 ** -24 * PR.window_mean_abs_terms(img, x, f, bt)
        worst = ((r.double().cpu() - r64).abs() / bound.clamp_min(1e-300)).max().item()
        print(f'{_ids(case)} r{"" if bt is None else " (beta)"}: worst |dr| / bound {worst:.3f}')
        assert ((r.double().cpu() - r64).abs() <= bound).all()
    worst = {q: [0.0, 0.0] for q in ('loss', 'gradient', 'composite')}

    def check(what, got, ref64, ref32, rel_to):
        err = ((got.double().cpu() - ref64).abs() / rel_to).max().item()
        yard = ((ref32.double() - ref64).abs() / rel_to).max().item()
        print(f'{_ids(case)} {what}: {err:.2e} (the same formula in fp32 on the CPU: {yard:.2e})')
        q = worst[what.split()[-1]]
        q[0], q[1] = max(q[0], err), max(q[1], yard)

    for kind, s in KIND_SCALES:
        tag = f'{kind} s={s:g}'
        l64, g64, _, _ = PR.loss_and_grad(img, x, f, kind, s, None, gmul)
        l32, g32, _, _ = PR.loss_and_grad(img, x, f, kind, s, None, gmul, dtype=torch.float32)
        loss, g, _ = ops.pixel_loss_grad(a, t, kind, s, grad_mul=gmul, pool=f, target_pooled=ts)
        check(f'{tag} loss', loss, l64, l32, l64.abs())
        check(f'{tag} gradient', g, g64, g32, g64.abs().max())
        for wrt in ('gen', 'composite'):
            l64, g64, c64, _ = PR.loss_and_grad(img, x, f, kind, s, beta, gmul, wrt=wrt)
            l32, g32, c32, _ = PR.loss_and_grad(img, x, f, kind, s, beta, gmul, wrt=wrt, dtype=torch.float32)
            loss, g, c = ops.pixel_loss_grad(a, t, kind, s, w, gmul, wrt=wrt, composite=True, pool=f)
            check(f'{tag} beta wrt={wrt} loss', loss, l64, l32, l64.abs())
            check(f'{tag} beta wrt={wrt} gradient', g, g64, g32, g64.abs().max())
            check(f'{tag} beta wrt={wrt} composite', c, c64, c32, torch.tensor(1.0, dtype=torch.float64))
    for q, (err, yard) in worst.items():
        print(f'{_ids(case)} worst {q}: {err:.2e} (yardstick {yard:.2e}, bar 4x)')
    assert all(err <= 4 * yard for err, yard in worst.values()), worst


# ------------------------------------------------------------------------------------------------------------- bad arguments
def test_bad_arguments_are_a_status_and_launch_nothing(dev):
    from oodgan import _lib, ops
    h, p = _lib.lib(), ops._p
    B, C, H, W = 2, 3, 16, 16
    a, t, w = torch.zeros(B, C, H, W, device=dev), torch.ones(B, C, H, W, device=dev), torch.ones(B, 1, H, W, device=dev)
    ts, g, c = torch.ones(B, C, 4, 4, device=dev), torch.full((B, C, H, W), -1.0, device=dev), torch.full((B, C, H, W), -1.0, device=dev)
    part, loss = torch.zeros(B, 8, device=dev), torch.full((B,), -1.0, device=dev)
    before = _lib.dispatch_count('pooled_pixel')

    def call(f=4, H=H, W=W, img=a, target=None, tpool=ts, beta=None, gimg=g, comp=None, kind=0, scale=0.5):
        ptr = lambda v: v if isinstance(v, int) else p(v)  # noqa: E731
        return h.oodgan_pooled_pixel_loss_fwd_bwd(ptr(img), ptr(target), ptr(tpool), ptr(beta), ptr(gimg), ptr(comp), p(part), p(loss), B, C, H, W,
                                                  f, kind, scale, 1, 1.0, ops._stream())

    for word, kw in ((b'factor', dict(f=3)), (b'factor', dict(f=32)), (b'multiple', dict(H=18)), (b'multiple', dict(f=8, W=20)),
                     (b'aligned', dict(img=a.data_ptr() + 4)), (b'aligned', dict(f=2, gimg=g.data_ptr() + 4)),
                     (b'aligned', dict(target=t, tpool=None, beta=w.data_ptr() + 8)), (b'composite', dict(comp=c)), (b'kind', dict(kind=4)),
                     (b'scale', dict(kind=1, scale=0.0)), (b'scale', dict(kind=3, scale=float('nan'))), (b'target', dict(target=t)),
                     (b'target', dict(tpool=None)), (b'target', dict(beta=w, target=t)), (b'target', dict(beta=w, tpool=None))):
        assert call(**kw) == -1 and word in h.oodgan_last_error(), (kw, h.oodgan_last_error())
    torch.cuda.synchronize()
    assert (loss == -1.0).all() and (g == -1.0).all() and (c == -1.0).all() and _lib.dispatch_count('pooled_pixel') == before
    assert call() == 0 and _lib.dispatch_count('pooled_pixel') == before + 1        # the same call with nothing wrong
    with pytest.raises(ValueError, match='kind'):
        ops.pixel_loss_grad(a, t, 'l1', 0.5, pool=4)
    with pytest.raises(RuntimeError, match='scale'):
        ops.pixel_loss_grad(a, t, 'huber', 0.0, pool=4)
    with pytest.raises(RuntimeError, match='factor'):
        ops.pixel_loss_grad(a, t, pool=3)
    with pytest.raises(ValueError, match='composite'):
        ops.pixel_loss_grad(a, t, composite=True, pool=4)
    with pytest.raises(ValueError, match='target_pooled'):
        ops.pixel_loss_grad(a, t, beta=w, pool=4, target_pooled=ts)
    with pytest.raises(ValueError, match='target_pooled'):
        ops.pixel_loss_grad(a, t, pool=4, target_pooled=ts[:, :, :2])
    with pytest.raises(ValueError, match='target_pooled'):
        ops.pixel_loss_grad(a, t, target_pooled=ts)


# ------------------------------------------------------------------------------------------------------- W+ step gradients
SIZE, PSIZE = 64, 16


def _step_inputs():
    """(generator state, target, noises, w0, beta): the seeds of test_hip_robust_loss.py's 64² step tests."""
    B = 2
    return (synth.generator_state(SIZE, seed=5), synth.make_images(SIZE, B, seed=9), synth.make_noises(SIZE, B, seed=7),
            synth.make_latents(SIZE, B, seed=14), _beta(B, SIZE, SIZE, 65))


@functools.lru_cache(maxsize=None)
def _oracle_step(kind, with_beta):
    """dL/dW+ and the per-image loss of the first step through the oracle in float64, and the oracle's own float32-vs-float64 distance of
    that gradient (relative to its max).  Computed once and shared by the precisions."""
    P, target, noises, w0, beta = _step_inputs()
    s, f = scale32(1.0), SIZE // PSIZE

    def run(dt):
        w = w0.to(dt).clone().requires_grad_(True)
        img = R.generator_forward({k: v.to(dt) for k, v in P.items()}, w, [n.to(dt) for n in noises], SIZE)
        r = PR.residual(img, target.to(dt), f, beta.to(dt) if with_beta else None)
        loss = PR.rho(r, kind, s).mean(dim=(1, 2, 3))
        loss.sum().backward()
        return w.grad.double(), loss.detach().double()

    g64, l64 = run(torch.float64)
    g32, _ = run(torch.float32)
    return g64, l64, (g32 - g64).abs().max().item() / g64.abs().max().item()


@pytest.mark.parametrize('prec,bar', [('f16s', 1e-4), ('f16s-g2', 3e-4)])
@pytest.mark.parametrize('with_beta', [False, True], ids=['full', 'beta'])
@pytest.mark.parametrize('kind', ['mse', 'charbonnier'])
def test_wplus_step_64_vs_float64_autograd(dev, kind, with_beta, prec, bar):
    """pixel_size=16 at 64² (factor 4), s = 1: the step's dL/dW+, recovered from Adam's first moment, within the project's bar (or, as the
    robust term's test has it, 3x the oracle's own fp32-vs-float64 distance where that is larger — printed); the loss within 1e-5."""
    from oodgan import _lib
    from oodgan.engine import GeneratorEngine, WPlusInverter
    P, target, noises, w0, beta = _step_inputs()
    g64, l64, e_self = _oracle_step(kind, with_beta)
    eng = GeneratorEngine({k: v.to(dev) for k, v in P.items()}, SIZE, precision=prec)
    inv = WPlusInverter(eng, pixel_loss=kind, pixel_scale=1.0, pixel_size=PSIZE)
    caps = {}
    inv.on_step = lambda run: caps.__setitem__(run.t, run.m.clone())
    _lib.dispatch_reset()
    _, losses = inv.invert(target.to(dev), w0.to(dev), [n.to(dev) for n in noises], steps=1, loss_weight=beta.to(dev) if with_beta else None)
    torch.cuda.synchronize()
    assert inv.last_stats['rollbacks'] == [0]
    assert _lib.dispatch_count('pooled_pixel') == 1 and _lib.dispatch_count('robust') == 0 and _lib.dispatch_count('composite_mse') == 0
    g = recover_grad(torch.zeros_like(caps[1]).cpu(), caps[1].cpu(), inv.betas[0])
    rel = (g - g64).abs().max().item() / g64.abs().max().item()
    e_loss = ((losses[0].double().cpu() - l64).abs() / l64).max().item()
    print(f'{kind} pixel_size={PSIZE} W+ step {SIZE}² {prec}{" + beta" if with_beta else ""}: dL/dW+ rel {rel:.2e} (bar {bar:g}; oracle f32 vs f64 '
          f'{e_self:.2e}), loss rel {e_loss:.2e}')
    assert rel < max(bar, 3 * e_self) and e_loss < 1e-5


# ------------------------------------------------------------------------------------------------------- the reference's own loop
@pytest.mark.parametrize('kind', ['mse', 'charbonnier'])
def test_loop_256_vs_reference(dev, golden, kind):
    """20 steps at 256², B = 2, pixel_size=64 (F.avg_pool2d(., 4) on image and target), s = 1: the loss curve against the reference
    Generator's autograd + torch.optim.Adam in float32 within 1e-3 relative on every step; the fixture's own fp32-vs-float64 figure beside it."""
    from oodgan.engine import GeneratorEngine, WPlusInverter
    g = golden('wplus_pixsize_256.npz')
    steps, s, f = int(g['steps']), float(g['scale']), int(g['factor'])
    _, sx, sn, sw = g['seeds'].tolist()
    size, B = 256, 2
    eng = GeneratorEngine({k: v.to(dev) for k, v in synth.generator_state(size, seed=0).items()}, size)
    x = synth.make_images(size, B, seed=sx).to(dev)
    noises = [n.to(dev) for n in synth.make_noises(size, B, seed=sn)]
    w0 = synth.make_latents(size, B, seed=sw, std=0.3).to(dev)
    inv = WPlusInverter(eng, pixel_loss=kind, pixel_scale=s, pixel_size=size // f)
    w, losses = inv.invert(x, w0, noises, steps=steps)
    l32, l64 = g[f'{kind}_losses_f32'], g[f'{kind}_losses_f64']
    e_curve = ((losses.double().cpu() - l32).abs() / l32).max().item()
    e_fix = ((l32 - l64).abs() / l64).max().item()
    e_w = (w.cpu() - g[f'{kind}_w_step{steps}']).abs().max().item()
    print(f'{kind} pixel_size={size // f} at 256², {steps} steps: loss curve rel {e_curve:.2e} (the fixture\'s own fp32 vs float64: {e_fix:.2e}); '
          f'|w_{steps} - reference w_{steps}| {e_w:.2e}; loss {losses[0].tolist()} -> {losses[-1].tolist()}')
    assert e_curve <= 1e-3
    assert (losses[-1] < losses[0]).all()
    assert inv.last_terms['pixel'] is not None and (inv.last_terms['mse'] is not None) == (kind == 'mse')


# ------------------------------------------------------------------------------------------------------- plans, streams, default, refusals
def _loop_inputs(dev, size, B, seed):
    eng_state = {k: v.to(dev) for k, v in synth.generator_state(size, seed=5 if size == 64 else 0).items()}
    target = synth.make_images(size, B, seed=seed).to(dev)
    noises = [n.to(dev) for n in synth.make_noises(size, B, seed=seed + 1)]
    w0 = synth.make_latents(size, B, seed=seed + 2, std=0.3).to(dev)
    return eng_state, target, noises, w0


@pytest.mark.parametrize('kind,with_beta', [('mse', False), ('charbonnier', False), ('mse', True)], ids=['mse', 'charbonnier', 'mse+beta'])
def test_plans_and_streams(dev, kind, with_beta):
    """The recorded plan, the Python-driven loop and the run that returns its trajectory agree bit for bit; a recorded step with pixel_size
    is as many launches as one without; two streams against one within 5e-3 (the same comparison without pixel_size is printed)."""
    from oodgan.engine import GeneratorEngine, WPlusInverter
    B, steps = 4, 12
    state, target, noises, w0 = _loop_inputs(dev, SIZE, B, 71)
    eng = GeneratorEngine(state, SIZE)
    beta = _beta(B, SIZE, SIZE, 74).to(dev) if with_beta else None
    kw = dict(pixel_loss=kind, pixel_scale=0.5)
    inv = WPlusInverter(eng, use_plan=True, pixel_size=PSIZE, **kw)
    w1, l1 = inv.invert(target, w0, noises, steps=steps, loss_weight=beta)
    plan1 = inv.last_plan
    assert plan1['steps'] == [steps - 3] and inv.last_stats['rollbacks'] == [0]
    assert (inv.last_terms['mse'] is not None) == (kind == 'mse') and inv.last_terms['pixel'].shape == (steps, B)
    inv2 = WPlusInverter(eng, use_plan=False, pixel_size=PSIZE, **kw)
    w2, l2 = inv2.invert(target, w0, noises, steps=steps, loss_weight=beta)
    assert inv2.last_plan['steps'] == [0] and torch.equal(w1, w2) and torch.equal(l1, l2)
    w3, l3, traj = inv.invert(target, w0, noises, steps=steps, return_trajectory=True, loss_weight=beta)
    assert torch.equal(w1, w3) and torch.equal(l1, l3) and len(traj) == steps and torch.equal(traj[-1], w1)
    ref = WPlusInverter(eng, use_plan=True, **kw)
    _, m1 = ref.invert(target, w0, noises, steps=steps, loss_weight=beta)
    assert ref.last_plan['steps'] == plan1['steps'] and ref.last_plan['launches'] == plan1['launches'] and plan1['launches'][0] > 0
    assert not torch.equal(m1, l1)
    w4, l4 = inv.invert(target, w0, noises, steps=steps, streams=2, loss_weight=beta)
    assert inv.last_plan['steps'] == [steps - 3] * 2 and inv.last_stats['rollbacks'] == [0, 0]
    _, m2 = ref.invert(target, w0, noises, steps=steps, streams=2, loss_weight=beta)
    rel, r_ref = ((l4 - l1).abs() / l1.abs()).max().item(), ((m2 - m1).abs() / m1.abs()).max().item()
    print(f'{kind}{" + beta" if with_beta else ""} pixel_size={PSIZE}, 2 streams vs 1 at {SIZE}², B={B}: loss rel diff {rel:.2e} (without pixel_size: '
          f'{r_ref:.2e}); plan {plan1}')
    assert rel <= 5e-3
    assert (l1[-1] < l1[0]).all()


def test_every_term_together(dev):
    """pixel_size + a loss weight + LPIPS at lpips_size + SSIM at 128²: the run finishes, every table is finite, the step is as long as the
    same step without pixel_size."""
    from oodgan.engine import GeneratorEngine, WPlusInverter
    from oodgan.lpips import LPIPSAlex
    size, B, steps = 128, 2, 8
    state, target, noises, w0 = _loop_inputs(dev, size, B, 81)
    eng = GeneratorEngine(state, size)
    beta = _beta(B, size, size, 84).to(dev)
    kw = dict(lpips=LPIPSAlex({k: v.to(dev) for k, v in synth.lpips_state(0).items()}, min_max=(-1.0, 1.0)), lpips_weight=0.8, lpips_size=64,
              ssim_weight=0.5, pixel_loss='huber', pixel_scale=0.5, use_plan=True)
    inv = WPlusInverter(eng, pixel_size=64, **kw)
    w, losses = inv.invert(target, w0, noises, steps=steps, loss_weight=beta)
    assert torch.isfinite(w).all() and torch.isfinite(losses).all() and inv.last_stats['rollbacks'] == [0]
    for k in ('pixel', 'lpips', 'ssim'):
        assert inv.last_terms[k].shape == (steps, B) and torch.isfinite(inv.last_terms[k]).all() and (inv.last_terms[k] > 0).all()
    ref = WPlusInverter(eng, **kw)
    ref.invert(target, w0, noises, steps=steps, loss_weight=beta)
    assert inv.last_plan['steps'] == ref.last_plan['steps'] == [steps - 3] and inv.last_plan['launches'] == ref.last_plan['launches']


def test_default_refusals_and_style_space(dev):
    """pixel_size=None and pixel_size=size are today's path bit for bit (the pooled kernel never runs); use_graph raises; the option is
    checked against the image; latent_space='s' takes it."""
    from oodgan import _lib
    from oodgan.engine import GeneratorEngine, WPlusInverter
    B, steps = 2, 6
    state, target, noises, w0 = _loop_inputs(dev, SIZE, B, 91)
    eng = GeneratorEngine(state, SIZE)
    _lib.dispatch_reset()
    base = WPlusInverter(eng)
    w0_, l0 = base.invert(target, w0, noises, steps=steps)
    for ps in (None, SIZE):
        inv = WPlusInverter(eng, pixel_size=ps)
        w1, l1 = inv.invert(target, w0, noises, steps=steps)
        assert torch.equal(w1, w0_) and torch.equal(l1, l0) and inv.last_plan == base.last_plan
        assert inv.last_terms['mse'] is inv.last_terms['pixel']
    assert _lib.dispatch_count('pooled_pixel') == 0
    w2, l2 = WPlusInverter(eng, pixel_size=PSIZE).invert(target, w0, noises, steps=steps)
    assert _lib.dispatch_count('pooled_pixel') >= 1 and not torch.equal(l2, l0)
    with pytest.raises(NotImplementedError, match='pixel_size'):
        WPlusInverter(eng, pixel_size=PSIZE).invert(target, w0, noises, steps=steps, use_graph=True)
    for bad in (48, 2, 128):                                  # not a divisor, a quotient of 32, larger than the image
        with pytest.raises(ValueError, match='pixel_size'):
            WPlusInverter(eng, pixel_size=bad).invert(target, w0, noises, steps=steps)
    inv = WPlusInverter(eng, pixel_size=PSIZE, latent_space='s', style_reg=0.1)
    n0 = _lib.dispatch_count('pooled_pixel')
    delta, ls = inv.invert(target, w0, noises, steps=steps)
    assert delta.shape == (B, eng.R) and torch.isfinite(delta).all() and torch.isfinite(ls).all() and (ls[-1] < ls[0]).all()
    assert _lib.dispatch_count('pooled_pixel') > n0              # counted per call of the entry point: replayed steps make none


def test_model_invert_takes_pixel_size(dev):
    """``invert(pixel_size=)`` on the model: checked beside lpips_size before anything runs; the image's own size is the default bit for bit;
    a smaller one runs the pooled kernel in a step of the same length."""
    from oodgan import _lib
    from oodgan.arch import ood_faceGAN_e4e
    size, B = 256, 2
    m = ood_faceGAN_e4e(out_size=size, style_dim=512, encoder='E4E', enable_modulation=True, warp_scale=0.08, cycle_align=2, blend_with_gen=True,
                        ModSize=256, build_encoder=False)
    res = m.load_state_dict(synth.ood_state(size, seed=41), strict=False)
    assert not res.missing_keys and not res.unexpected_keys, res
    m = m.to(dev).eval()
    x = synth.make_images(size, B, seed=44).to(dev)
    kw = dict(enc_lats=synth.make_latents(size, B, seed=42, std=0.3).to(dev), enc_feats=[f.to(dev) for f in synth.make_encoder_feats(B, seed=43)],
              noise=[n.to(dev) for n in synth.make_noises(size, B, seed=45)])
    for bad in (True, 64.0, '64', 96, 8):
        with pytest.raises(ValueError, match='pixel_size'):
            m.invert(x, steps=2, pixel_size=bad, **kw)
    with pytest.raises(NotImplementedError):
        m.invert(x, steps=2, pixel_size=64, use_graph=True, **kw)
    _lib.dispatch_reset()
    _, lats0, l0 = m.invert(x, steps=6, **kw)
    plan0 = m.last_invert_plan
    _, lats1, l1 = m.invert(x, steps=6, pixel_size=size, **kw)
    assert torch.equal(lats0, lats1) and torch.equal(l0, l1) and m.last_invert_plan == plan0 and _lib.dispatch_count('pooled_pixel') == 0
    _, lats2, l2 = m.invert(x, steps=6, pixel_size=64, loss_region='blend', **kw)
    assert _lib.dispatch_count('pooled_pixel') >= 1 and torch.isfinite(lats2).all() and torch.isfinite(l2).all()
    _, _, l3 = m.invert(x, steps=6, pixel_size=64, **kw)
    assert m.last_invert_plan['launches'] == plan0['launches'] and m.last_loss_terms['mse'] is m.last_loss_terms['pixel']
    assert not torch.equal(l3, l0)
