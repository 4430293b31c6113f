"""Robust pixel terms of the W+ loss (csrc/loss_pixel.hip): Charbonnier, Huber and Geman-McClure in the MSE's place.

The kernel against float64 on the same float32 inputs (tests/robust_ref.py) in all of its forms and, with beta == 1, bit for bit against
its plain form; one W+ step's dL/dW+ against float64 autograd through the oracle; 20 steps against the reference's own autograd loop
(tests/golden/make_wplus_robust.py); launch plans and streams; beta = 0 pixels; the untouched default path and the refusals."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import ref_cpu as R  # noqa: E402
from oodgan import synth  # noqa: E402
from robust_ref import KINDS, loss_and_grad, rho, scale32  # noqa: E402
from wplus_grads import recover_grad  # noqa: E402


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


def _beta(B, H, W, seed):
    """A seeded, non-binary plane in [0, 1] with an exact-zero and an exact-one block."""
    b = torch.sigmoid(2.0 * synth.normal('robust.beta', (B, 1, H, W), seed))
    b[:, :, : H // 4, : W // 4] = 0.0
    b[:, :, -(H // 4):, -(W // 4):] = 1.0
    return b.contiguous()


# ------------------------------------------------------------------------------------------------------------- kernel
@pytest.mark.parametrize('B', [1, 3, 8])
@pytest.mark.parametrize('H,W', [(256, 256), (64, 64), (37, 37)])     # plane form with beta (HW % 16384 == 0), flat float4 form, scalar form
@pytest.mark.parametrize('kind', KINDS)
def test_kernel_vs_float64(dev, kind, H, W, B):
    """Seeded residuals of order 1 against s = 1e-6 (every |d| >> s), 0.5 (both sides) and 10 (every |d| < s); with and without a loss
    weight; the gradient w.r.t. the generator output and w.r.t. the composite; the composite itself."""
    from oodgan import ops
    img = synth.normal('robust.img', (B, 3, H, W), 1)
    x = synth.make_images(H, B, seed=2)[:, :, :H, :W].contiguous() if H == W else synth.normal('robust.x', (B, 3, H, W), 2)
    beta = _beta(B, H, W, 3)
    gmul = ops.loss_scale_for(3 * H * W)
    a, t, w = img.to(dev), x.to(dev), beta.to(dev)
    ones = torch.ones(B, 1, H, W, device=dev)
    for s in (1e-6, 0.5, 10.0):
        # plain form
        l_ref, g_ref, _ = loss_and_grad(img, x, kind, s, None, gmul)
        loss, g, c = ops.robust_loss_grad(a, t, kind, s, grad_mul=gmul)
        assert c is None
        e_loss = ((loss.double().cpu() - l_ref).abs() / l_ref).max().item()
        e_g = (g.double().cpu() - g_ref).abs().max().item() / g_ref.abs().max().item()
        print(f'{kind} s={s:g} B={B} {H}x{W} plain: loss rel {e_loss:.2e}, gradient {e_g:.2e} of max')
        assert e_loss <= 1e-6 and e_g <= 1e-6
        # forward only: the same loss bit for bit
        l_fwd, g_none, _ = ops.robust_loss_grad(a, t, kind, s, grad_mul=gmul, grad=False)
        assert g_none is None and torch.equal(l_fwd, loss)
        # with a loss weight
        lb_ref, gg_ref, c_ref = loss_and_grad(img, x, kind, s, beta, gmul, wrt='gen')
        _, gc_ref, _ = loss_and_grad(img, x, kind, s, beta, gmul, wrt='composite')
        lb, gg, c = ops.robust_loss_grad(a, t, kind, s, w, gmul, wrt='gen', composite=True)
        lb2, gc, c2 = ops.robust_loss_grad(a, t, kind, s, w, gmul, wrt='composite')
        assert c2 is None and torch.equal(lb2, lb)
        e_loss = ((lb.double().cpu() - lb_ref).abs() / lb_ref).max().item()
        e_gg = (gg.double().cpu() - gg_ref).abs().max().item() / gg_ref.abs().max().item()
        e_gc = (gc.double().cpu() - gc_ref).abs().max().item() / gc_ref.abs().max().item()
        e_c = (c.double().cpu() - c_ref).abs().max().item()
        print(f'{kind} s={s:g} B={B} {H}x{W} beta: loss rel {e_loss:.2e}, dL/dG {e_gg:.2e}, dL/dc {e_gc:.2e} of max, |c| err {e_c:.2e}')
        assert e_loss <= 1e-6 and e_gg <= 1e-6 and e_gc <= 1e-6 and e_c <= 1e-6
        l_fwd, _, c_fwd = ops.robust_loss_grad(a, t, kind, s, w, gmul, composite=True, grad=False)
        assert torch.equal(l_fwd, lb) and torch.equal(c_fwd, c)
        # the loss-table form writes row min(row_dev[0], nrows - 1) and no other
        for bt, want_l, want_g in ((None, loss, g), (w, lb, gg)):
            table = torch.full((4, B), -1.0, device=dev)
            for row in (2, 9):
                row_dev = torch.tensor([row], dtype=torch.int32, device=dev)
                none, g2, _ = ops.robust_loss_grad(a, t, kind, s, bt, gmul, table=table, row_dev=row_dev)
                assert none is None and torch.equal(table[min(row, 3)], want_l) and torch.equal(g2, want_g)
            assert torch.equal(table[:2], torch.full((2, B), -1.0, device=dev))
        # beta == 1: the plain form's loss and gradient, bit for bit (same chunks, same reduction order)
        for wrt in ('gen', 'composite'):
            l1, g1, _ = ops.robust_loss_grad(a, t, kind, s, ones, gmul, wrt=wrt)
            assert torch.equal(l1, loss) and torch.equal(g1, g), (s, wrt)


@pytest.mark.parametrize('H,W', [(256, 256), (64, 64), (37, 37)])
def test_huber_with_a_large_scale_is_half_the_mse(dev, H, W):
    from oodgan import ops
    B = 3
    a, t = synth.normal('robust.img', (B, 3, H, W), 1).to(dev), synth.normal('robust.x', (B, 3, H, W), 2).to(dev)
    gmul = ops.loss_scale_for(3 * H * W)
    l_mse, g_mse = ops.mse_loss_grad(a, t, gmul)
    l_h, g_h, _ = ops.robust_loss_grad(a, t, 'huber', 1e6, grad_mul=gmul)
    e_l = ((l_h - 0.5 * l_mse).abs() / (0.5 * l_mse)).max().item()
    e_g = (g_h - 0.5 * g_mse).abs().max().item() / (0.5 * g_mse).abs().max().item()
    print(f'huber s=1e6 {H}x{W} vs MSE/2: loss rel {e_l:.2e}, gradient rel {e_g:.2e}')
    assert e_l <= 1e-6 and e_g <= 1e-6


def test_bad_kind_or_scale_is_a_status_not_a_crash(dev):
    from oodgan import _lib, ops
    h = _lib.lib()
    a, t = torch.zeros(1, 3, 8, 8, device=dev), torch.ones(1, 3, 8, 8, device=dev)
    part, loss = torch.zeros(1, 1, device=dev), torch.full((1,), -1.0, device=dev)
    p = ops._p
    before = _lib.dispatch_count('robust')
    for kind, s, word in ((0, 0.5, b'kind'), (4, 0.5, b'kind'), (1, 0.0, b'scale'), (2, -1.0, b'scale'), (3, float('nan'), b'scale'),
                          (1, float('inf'), b'scale')):
        rc = h.oodgan_robust_loss_fwd_bwd(p(a), p(t), None, None, None, p(part), p(loss), 1, 3, 64, kind, s, 1, 1.0, ops._stream())
        assert rc == -1 and word in h.oodgan_last_error(), (kind, s)
    torch.cuda.synchronize()
    assert loss.item() == -1.0 and _lib.dispatch_count('robust') == before
    with pytest.raises(ValueError, match='kind'):
        ops.robust_loss_grad(a, t, 'l1', 0.5)
    with pytest.raises(RuntimeError, match='scale'):
        ops.robust_loss_grad(a, t, 'huber', 0.0)
    with pytest.raises(ValueError, match='composite'):
        ops.robust_loss_grad(a, t, 'huber', 0.5, composite=True)


# ------------------------------------------------------------------------------------------------------- W+ step gradients
def _step_grads(inv, target, w0, noises, beta, steps=1):
    """Run ``steps`` steps of the loop and recover each step's dL/dW+ from Adam's first moment."""
    caps = {}
    inv.on_step = lambda run: caps.__setitem__(run.t, run.m.clone())
    _, losses = inv.invert(target, w0, noises, steps=steps, loss_weight=beta)
    torch.cuda.synchronize()
    assert inv.last_stats['rollbacks'] == [0]
    m_prev = torch.zeros_like(caps[1]).cpu()
    grads = []
    for t in range(1, steps + 1):
        grads.append(recover_grad(m_prev, caps[t].cpu(), inv.betas[0]))
        m_prev = caps[t].cpu()
    return grads, losses


def _step_inputs(size):
    """(generator state, target, noises, w0, beta) of the step tests: the seeds of test_hip_wplus_masked.py's step tests at that size."""
    B = 2
    if size == 64:
        return (synth.generator_state(size, seed=5), synth.make_images(size, B, seed=9), synth.make_noises(size, B, seed=7),
                synth.make_latents(size, B, seed=14), _beta(B, size, size, 65))
    return (synth.generator_state(size, seed=0), synth.make_images(size, B, seed=61), synth.make_noises(size, B, seed=62),
            synth.make_latents(size, B, seed=63, std=0.3), _beta(B, size, size, 64))


@functools.lru_cache(maxsize=None)
def _oracle_step(size, kind, with_beta):
    """dL/dW+ and the per-image loss of the first step through the oracle in float64, and the oracle's own float32-vs-float64 distance
    e_self of that gradient (relative to its max).  Computed once and shared by the precisions."""
    P, target, noises, w0, beta = _step_inputs(size)
    s = scale32(1.0)

    def run(dt):
        w = w0.to(dt).clone().requires_grad_(True)
        img = R.generator_forward({k: v.to(dt) for k, v in P.items()}, w, [n.to(dt) for n in noises], size)
        d = img - target.to(dt)
        if with_beta:
            d = beta.to(dt) * d
        loss = rho(d, kind, s).mean(dim=(1, 2, 3))
        loss.sum().backward()
        return w.grad.double(), loss.detach().double()

    g64, l64 = run(torch.float64)
    g32, _ = run(torch.float32)
    return g64, l64, (g32 - g64).abs().max().item() / g64.abs().max().item()


def _check_step(dev, size, kind, with_beta, prec, bar):
    from oodgan import _lib
    from oodgan.engine import GeneratorEngine, WPlusInverter
    P, target, noises, w0, beta = _step_inputs(size)
    g64, l64, e_self = _oracle_step(size, kind, with_beta)
    eng = GeneratorEngine({k: v.to(dev) for k, v in P.items()}, size, precision=prec)
    _lib.dispatch_reset()
    (g,), losses = _step_grads(WPlusInverter(eng, pixel_loss=kind, pixel_scale=1.0), target.to(dev), w0.to(dev), [n.to(dev) for n in noises],
                               beta.to(dev) if with_beta else None)
    assert _lib.dispatch_count('robust') == 1 and _lib.dispatch_count('composite_mse') == 0
    rel = (g - g64).abs().max().item() / g64.abs().max().item()
    e_loss = ((losses[0].double().cpu() - l64).abs() / l64).max().item()
    print(f'{kind} W+ step {size}² {prec}{" + beta" if with_beta else ""}: dL/dW+ rel {rel:.2e} (bar max({bar:g}, 3 x oracle f32 vs f64 '
          f'{e_self:.2e})), loss rel {e_loss:.2e}')
    assert rel < max(bar, 3 * e_self) and e_loss < 1e-5


@pytest.mark.parametrize('prec,bar', [('f16s', 1e-4), ('f16s-g2', 3e-4)])
@pytest.mark.parametrize('with_beta', [False, True], ids=['full', 'beta'])
@pytest.mark.parametrize('kind', KINDS)
def test_wplus_step_64_vs_float64_autograd(dev, kind, with_beta, prec, bar):
    _check_step(dev, 64, kind, with_beta, prec, bar)


@pytest.mark.parametrize('prec,bar', [('f16s', 1e-4), ('f16s-g2', 3e-4)])
def test_wplus_step_256_vs_float64_autograd(dev, prec, bar):
    _check_step(dev, 256, 'geman_mcclure', True, prec, bar)


# ------------------------------------------------------------------------------------------------------- the reference's own loop
@pytest.mark.parametrize('kind', KINDS)
def test_loop_256_vs_reference(dev, golden, kind):
    """20 steps at 256², B = 2, s = 1: the loss curve against the reference Generator's autograd + torch.optim.Adam in float32, within
    max(1e-3, 3 x the fixture's own float32-vs-float64 distance)."""
    from oodgan.engine import GeneratorEngine, WPlusInverter
    g = golden('wplus_robust_256.npz')
    steps, s = int(g['steps']), float(g['scale'])
    _, sx, sn, sw = g['seeds'].tolist()
    size, B = 256, 2
    eng = GeneratorEngine({k: v.to(dev) for k, v in synth.generator_state(size, seed=0).items()}, size)
    x = synth.make_images(size, B, seed=sx).to(dev)
    noises = [n.to(dev) for n in synth.make_noises(size, B, seed=sn)]
    w0 = synth.make_latents(size, B, seed=sw, std=0.3).to(dev)
    inv = WPlusInverter(eng, pixel_loss=kind, pixel_scale=s)
    w, losses = inv.invert(x, w0, noises, steps=steps)
    l32, l64 = g[f'{kind}_losses_f32'], g[f'{kind}_losses_f64']
    e_curve = ((losses.double().cpu() - l32).abs() / l32).max().item()
    e_fix = ((l32 - l64).abs() / l64).max().item()
    e_w = (w.cpu() - g[f'{kind}_w_step{steps}']).abs().max().item()
    print(f'{kind} 256², {steps} steps: loss curve rel {e_curve:.2e} (the fixture\'s own fp32 vs float64: {e_fix:.2e}); '
          f'|w_{steps} - reference w_{steps}| {e_w:.2e}; loss {losses[0].tolist()} -> {losses[-1].tolist()}')
    assert e_curve <= max(1e-3, 3 * e_fix)
    assert (losses[-1] < losses[0]).all()
    assert inv.last_terms['pixel'] is not None and inv.last_terms['mse'] is None


# ------------------------------------------------------------------------------------------------------- plans, streams
@pytest.mark.parametrize('kind,extra', [(k, False) for k in KINDS] + [('charbonnier', True)], ids=list(KINDS) + ['charbonnier+beta+lpips+ssim'])
def test_plans_and_streams(dev, kind, extra):
    """The recorded plan against the Python-driven loop, bit for bit; two streams against one, within max(5e-3, 3 x what the same comparison
    gives for pixel_loss='mse' with the same other terms)."""
    from oodgan.engine import GeneratorEngine, WPlusInverter
    from oodgan.lpips import LPIPSAlex
    size, B, steps = 256, 4, 12
    eng = GeneratorEngine({k: v.to(dev) for k, v in synth.generator_state(size, seed=0).items()}, size)
    target = synth.make_images(size, B, seed=71).to(dev)
    noises = [n.to(dev) for n in synth.make_noises(size, B, seed=72)]
    w0 = synth.make_latents(size, B, seed=73, std=0.3).to(dev)
    kw, beta = {}, None
    if extra:
        beta = _beta(B, size, size, 74).to(dev)
        kw.update(lpips=LPIPSAlex({k: v.to(dev) for k, v in synth.lpips_state(0).items()}, min_max=(-1.0, 1.0)), lpips_weight=0.8, ssim_weight=0.5)
    terms = ('pixel', 'lpips', 'ssim') if extra else ('pixel',)
    inv = WPlusInverter(eng, use_plan=True, pixel_loss=kind, pixel_scale=0.5, **kw)
    w1, l1 = inv.invert(target, w0, noises, steps=steps, loss_weight=beta)
    t1 = {k: inv.last_terms[k].clone() for k in terms}
    assert inv.last_plan['steps'] == [9] and inv.last_stats['rollbacks'] == [0]
    assert inv.last_terms['mse'] is None
    inv2 = WPlusInverter(eng, use_plan=False, pixel_loss=kind, pixel_scale=0.5, **kw)
    w2, l2 = inv2.invert(target, w0, noises, steps=steps, loss_weight=beta)
    assert torch.equal(w1, w2) and torch.equal(l1, l2)
    assert inv2.last_plan['steps'] == [0] and all(torch.equal(t1[k], inv2.last_terms[k]) for k in terms)
    w3, l3 = inv.invert(target, w0, noises, steps=steps, streams=2, loss_weight=beta)
    assert inv.last_plan['steps'] == [9, 9] and inv.last_stats['rollbacks'] == [0, 0]
    assert all(inv.last_terms[k].shape == (steps, B) for k in terms)
    rel = ((l3 - l1).abs() / l1.abs()).max().item()
    ref = WPlusInverter(eng, use_plan=True, **kw)
    _, m1 = ref.invert(target, w0, noises, steps=steps, loss_weight=beta)
    _, m2 = ref.invert(target, w0, noises, steps=steps, streams=2, loss_weight=beta)
    r_mse = ((m2 - m1).abs() / m1.abs()).max().item()
    print(f'{kind}{" + beta + LPIPS + SSIM" if extra else ""}, 2 streams vs 1 at 256², B={B}: loss rel diff {rel:.2e} (mse: {r_mse:.2e}); '
          f'plan {inv.last_plan}')
    assert rel <= max(5e-3, 3 * r_mse)
    assert (l1[-1] < l1[0]).all()


# ------------------------------------------------------------------------------------------------------- beta = 0
@pytest.mark.parametrize('kind', KINDS)
def test_zero_weight_pixels_have_no_influence(dev, kind):
    """Launch plans on: a target changed only where beta = 0 gives the same latents and loss table, bit for bit."""
    from oodgan.engine import GeneratorEngine, WPlusInverter
    size, B, steps = 64, 2, 12
    eng = GeneratorEngine({k: v.to(dev) for k, v in synth.generator_state(size, seed=5).items()}, size)
    target = synth.make_images(size, B, seed=9).to(dev)
    noises = [n.to(dev) for n in synth.make_noises(size, B, seed=7)]
    w0 = synth.make_latents(size, B, seed=14).to(dev)
    beta = _beta(B, size, size, 66).to(dev)
    beta[:, :, 20:40, 10:50] = 0.0
    other = torch.where(beta == 0, synth.make_images(size, B, seed=99).to(dev), target)
    assert (other != target).any()
    inv = WPlusInverter(eng, use_plan=True, pixel_loss=kind, pixel_scale=0.5)
    w1, l1 = inv.invert(target, w0, noises, steps=steps, loss_weight=beta)
    assert inv.last_plan['steps'] == [steps - 3]
    w2, l2 = inv.invert(other, w0, noises, steps=steps, loss_weight=beta)
    assert torch.equal(w1, w2) and torch.equal(l1, l2)
    w3, l3 = inv.invert(other, w0, noises, steps=steps)        # without the weight the changed pixels do count
    assert not torch.equal(l3, l1)


# ------------------------------------------------------------------------------------------------------- the default, the refusals
def _ood_model(dev, size=256):
    from oodgan.arch import ood_faceGAN_e4e
    m = ood_faceGAN_e4e(out_size=size, style_dim=512, encoder='E4E', enable_modulation=True, warp_scale=0.08, cycle_align=2, blend_with_gen=True,
                        ModSize=256, build_encoder=False)
    res = m.load_state_dict(synth.ood_state(size, seed=41), strict=False)
    assert not res.missing_keys and not res.unexpected_keys, res
    return m.to(dev).eval()


def _ood_inputs(dev, size=256, B=2):
    enc_lats = synth.make_latents(size, B, seed=42, std=0.3).to(dev)
    enc_feats = [f.to(dev) for f in synth.make_encoder_feats(B, seed=43)]
    x = synth.make_images(size, B, seed=44).to(dev)
    noises = [n.to(dev) for n in synth.make_noises(size, B, seed=45)]
    return x, dict(enc_lats=enc_lats, enc_feats=enc_feats, noise=noises)


def test_the_default_is_untouched(dev):
    """``invert()`` with no option and with pixel_loss='mse': identical latents and losses, the same launch list, no robust kernel."""
    from oodgan import _lib
    m = _ood_model(dev)
    x, kw = _ood_inputs(dev)
    _lib.dispatch_reset()
    _, lats0, l0 = m.invert(x, steps=6, **kw)
    plan0, terms0 = m.last_invert_plan, m.last_loss_terms
    assert terms0['mse'] is terms0['pixel'] and terms0['mse'] is not None
    _, lats1, l1 = m.invert(x, steps=6, pixel_loss='mse', **kw)
    assert torch.equal(lats0, lats1) and torch.equal(l0, l1) and m.last_invert_plan == plan0
    assert m.last_loss_terms['mse'] is m.last_loss_terms['pixel']
    _, lats2, l2 = m.invert(x, steps=6, pixel_loss='mse', pixel_scale=3.0, **kw)      # the scale is not read by 'mse'
    assert torch.equal(lats0, lats2) and torch.equal(l0, l2) and m.last_invert_plan == plan0
    assert _lib.dispatch_count('robust') == 0
    _, _, l3 = m.invert(x, steps=6, pixel_loss='huber', **kw)
    assert _lib.dispatch_count('robust') >= 1 and not torch.equal(l3, l0)
    assert m.last_loss_terms['mse'] is None and m.last_loss_terms['pixel'] is not None
    assert m.last_invert_plan['launches'] == plan0['launches']          # one kernel in another's place: the step is as long as before


def test_refusals(dev):
    from oodgan.engine import GeneratorEngine, WPlusInverter
    m = _ood_model(dev)
    x, kw = _ood_inputs(dev, B=1)
    with pytest.raises(ValueError, match='pixel_loss'):
        m.invert(x, steps=2, pixel_loss='l1', **kw)
    for bad in (0, -0.5, float('nan'), float('inf'), 'wide'):
        with pytest.raises(ValueError, match='pixel_scale'):
            m.invert(x, steps=2, pixel_loss='huber', pixel_scale=bad, **kw)
        with pytest.raises(ValueError, match='pixel_scale'):
            WPlusInverter(None, pixel_loss='huber', pixel_scale=bad)
    with pytest.raises(ValueError, match='pixel_loss'):
        WPlusInverter(None, pixel_loss='l1')
    with pytest.raises(NotImplementedError):
        m.invert(x, steps=2, pixel_loss='charbonnier', use_graph=True, **kw)
    eng = GeneratorEngine({k: v.to(dev) for k, v in synth.generator_state(64, seed=5).items()}, 64)
    for kind in KINDS:
        with pytest.raises(NotImplementedError):
            WPlusInverter(eng, pixel_loss=kind).invert(synth.make_images(64, 1, seed=1).to(dev), synth.make_latents(64, 1, seed=2).to(dev),
                                                       [n.to(dev) for n in synth.make_noises(64, 1, seed=3)], steps=2, use_graph=True)
