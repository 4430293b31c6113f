"""The masked W+ objective: the loss on the composite c = x + beta*(G(w) - x), beta one (B,1,S,S) plane per image.

Kernels (csrc/loss_pixel.hip, csrc/loss_masked.hip) against float64 torch and, with beta == 1, bit for bit against the plain MSE form; one W+ step's dL/dW+
against float64 autograd through the oracle (with and without the LPIPS term); beta = 0 pixels have no influence on the run; the
``loss_region='blend'`` inversion at 256² against the reference's own autograd loop (tests/golden/make_wplus_masked.py); launch plans,
streams, the untouched default path and the refusals."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import lpips_cpu as LO  # noqa: E402
from oracle import ref_cpu as R  # noqa: E402
from oodgan import synth  # noqa: E402
from wplus_grads import recover_grad  # noqa: E402


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


def _beta(B, H, W, seed):
    """A seeded, non-binary plane in [0, 1] with an exact-zero and an exact-one block."""
    b = torch.sigmoid(2.0 * synth.normal('masked.beta', (B, 1, H, W), seed))
    b[:, :, : H // 4, : W // 4] = 0.0
    b[:, :, -(H // 4):, -(W // 4):] = 1.0
    return b.contiguous()


# ------------------------------------------------------------------------------------------------------------- kernels
@pytest.mark.parametrize('B', [1, 3, 8])
@pytest.mark.parametrize('H,W', [(256, 256), (64, 64), (37, 37)])     # plane form (HW % 16384 == 0), flat float4 form, scalar form
def test_composite_kernel_vs_float64(dev, B, H, W):
    from oodgan import ops
    img = synth.normal('masked.img', (B, 3, H, W), 1)
    x = synth.make_images(H, B, seed=2)[:, :, :H, :W].contiguous() if H == W else synth.normal('masked.x', (B, 3, H, W), 2)
    beta = _beta(B, H, W, 3)
    gmul = ops.loss_scale_for(3 * H * W)
    d = beta.double() * (img.double() - x.double())
    loss_ref = (d ** 2).mean(dim=(1, 2, 3))
    gc_ref = gmul * 2.0 / (3 * H * W) * d                                   # dL/dc
    gg_ref = gc_ref * beta.double()                                         # dL/dG = beta * dL/dc
    a, t, w = img.to(dev), x.to(dev), beta.to(dev)
    loss, gg, c = ops.composite_mse_loss_grad(a, t, w, gmul, wrt='gen', composite=True)
    _, gc, _ = ops.composite_mse_loss_grad(a, t, w, gmul, wrt='composite')
    e_loss = ((loss.double().cpu() - loss_ref).abs() / loss_ref).max().item()
    e_gg = (gg.double().cpu() - gg_ref).abs().max().item() / gg_ref.abs().max().item()
    e_gc = (gc.double().cpu() - gc_ref).abs().max().item() / gc_ref.abs().max().item()
    e_c = (c.double().cpu() - (x.double() + d)).abs().max().item()
    print(f'composite MSE B={B} {H}x{W}: loss rel {e_loss:.2e}, dL/dG {e_gg:.2e}, dL/dc {e_gc:.2e} of max, |c| err {e_c:.2e}')
    assert e_loss <= 1e-6 and e_gg <= 1e-6 and e_gc <= 1e-6 and e_c <= 1e-6
    # the loss-table form writes row row_dev[0] (clamped to the table)
    table = torch.full((4, B), -1.0, device=dev)
    for row in (2, 9):
        row_dev = torch.tensor([row], dtype=torch.int32, device=dev)
        _, g2, _ = ops.composite_mse_loss_grad(a, t, w, gmul, table=table, row_dev=row_dev)
        assert torch.equal(table[min(row, 3)], loss) and torch.equal(g2, gg)
    assert torch.equal(table[0], torch.full((B,), -1.0, device=dev))
    # beta == 1: the plain MSE kernel's loss and gradient, bit for bit (same chunks, same reduction order)
    ones = torch.ones(B, 1, H, W, device=dev)
    l1, g1 = ops.mse_loss_grad(a, t, gmul)
    for wrt in ('gen', 'composite'):
        lm, gm, _ = ops.composite_mse_loss_grad(a, t, ones, gmul, wrt=wrt)
        assert torch.equal(lm, l1) and torch.equal(gm, g1), wrt


def test_scale_by_plane_and_loss_weight_from_alpha(dev):
    from oodgan import ops
    for (H, W) in ((64, 64), (37, 37)):
        g = synth.normal('masked.g', (3, 3, H, W), 4).to(dev)
        beta = _beta(3, H, W, 5).to(dev)
        want = g * beta
        assert torch.equal(ops.scale_by_plane(g, beta), want) and torch.equal(g, want)
    alpha = torch.sigmoid(3.0 * synth.normal('masked.alpha', (2, 1, 64, 64), 6)).to(dev)
    alpha[0, 0, 0, :8] = torch.tensor([-0.5, 0.0, 1.0, 1.5, 0.25, 0.5, 0.75, 2.0])      # out of range: clipped as blending_mask clips
    for n in (0, 1, 2, 3):
        want = (1.0 - alpha.double()).clamp(0.0, 1.0) ** n
        got = ops.loss_weight_from_alpha(alpha, n)
        assert (got.double() - want).abs().max().item() <= 1e-6, n


# ------------------------------------------------------------------------------------------------------- W+ step gradients
def _step_grads(inv, target, w0, noises, beta, steps=1):
    """Run ``steps`` steps of the loop with the loss weight ``beta`` and recover each step's dL/dW+ from Adam's first moment."""
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


@pytest.mark.parametrize('prec,bar', [('f16s', 1e-4), ('f16s-g2', 3e-4)])
def test_wplus_step_256_vs_float64_autograd(dev, prec, bar):
    """dL/dW+ of the first W+ step at 256² with a seeded non-binary beta (the bars of test_hip_wplus_golden.py)."""
    from oodgan import _lib
    from oodgan.engine import GeneratorEngine, WPlusInverter
    size, B = 256, 2
    P = synth.generator_state(size, seed=0)
    target = synth.make_images(size, B, seed=61)
    noises = synth.make_noises(size, B, seed=62)
    w0 = synth.make_latents(size, B, seed=63, std=0.3)
    beta = _beta(B, size, size, 64)
    w = w0.double().clone().requires_grad_(True)
    img = R.generator_forward({k: v.double() for k, v in P.items()}, w, [n.double() for n in noises], size)
    loss_ref = ((beta.double() * (img - target.double())) ** 2).mean(dim=(1, 2, 3))
    loss_ref.sum().backward()
    eng = GeneratorEngine({k: v.to(dev) for k, v in P.items()}, size, precision=prec)
    _lib.dispatch_reset()
    (g,), losses = _step_grads(WPlusInverter(eng), target.to(dev), w0.to(dev), [n.to(dev) for n in noises], beta.to(dev))
    assert _lib.dispatch_count('composite_mse') == 1
    rel = (g - w.grad).abs().max().item() / w.grad.abs().max().item()
    e_loss = ((losses[0].double().cpu() - loss_ref.detach()).abs() / loss_ref.detach()).max().item()
    print(f'masked W+ step 256² {prec}: dL/dW+ rel {rel:.2e} (bar {bar:g}), loss rel {e_loss:.2e}')
    assert rel < bar and e_loss < 1e-5


@pytest.mark.parametrize('prec,bar', [('f16s', 1e-4), ('f16s-g2', 3e-4)])
def test_wplus_step_64_with_lpips_vs_float64_autograd(dev, prec, bar):
    """The same with the LPIPS term on seeded weights: L = mean((beta (G - x))^2) + lam * LPIPS(x + beta (G - x), x).  A ReLU or max-pool
    decision within rounding flips between fp32 and float64 (test_hip_lpips.py): the bar is also met against the oracle's own fp32 autograd
    where that is closer, and never looser than 3x the oracle's fp32-vs-float64 distance."""
    from oodgan.engine import GeneratorEngine, WPlusInverter
    from oodgan.lpips import LPIPSAlex
    size, B, lam = 64, 2, 0.8
    P, PL = synth.generator_state(size, seed=5), synth.lpips_state(0)
    target = synth.make_images(size, B, seed=9)
    noises = synth.make_noises(size, B, seed=7)
    w0 = synth.make_latents(size, B, seed=14)
    beta = _beta(B, size, size, 65)

    def oracle(dt):
        w = w0.to(dt).clone().requires_grad_(True)
        img = R.generator_forward({k: v.to(dt) for k, v in P.items()}, w, [n.to(dt) for n in noises], size)
        c = target.to(dt) + beta.to(dt) * (img - target.to(dt))
        mse = ((c - target.to(dt)) ** 2).mean(dim=(1, 2, 3))
        _, lp = LO.lpips_loss({k: v.to(dt) for k, v in PL.items()}, c, target.to(dt), min_max=(-1.0, 1.0), reduction='none')
        (mse.sum() + lam * lp.sum()).backward()
        return w.grad.double(), (mse + lam * lp).detach().double()

    g64, l64 = oracle(torch.float64)
    g32, _ = oracle(torch.float32)
    eng = GeneratorEngine({k: v.to(dev) for k, v in P.items()}, size, precision=prec)
    net = LPIPSAlex({k: v.to(dev) for k, v in PL.items()}, min_max=(-1.0, 1.0))
    (g,), losses = _step_grads(WPlusInverter(eng, lpips=net, lpips_weight=lam), target.to(dev), w0.to(dev), [n.to(dev) for n in noises],
                               beta.to(dev))
    scale = g64.abs().max().item()
    rel, rel32, e_self = ((g - g64).abs().max().item() / scale, (g - g32).abs().max().item() / scale, (g32 - g64).abs().max().item() / scale)
    e_loss = ((losses[0].double().cpu() - l64).abs() / l64).max().item()
    print(f'masked W+ step 64² + LPIPS {prec}: dL/dW+ rel {rel:.2e} vs f64, {rel32:.2e} vs the f32 oracle (oracle f32 vs f64 {e_self:.2e}; '
          f'bar {bar:g}), loss rel {e_loss:.2e}')
    assert min(rel, rel32) < max(bar, 3 * e_self) and e_loss < 1e-4


# ------------------------------------------------------------------------------------------------------- beta = 0
def test_zero_weight_pixels_have_no_influence(dev):
    """MSE-only loss, launch plans on: a target changed only where beta = 0 gives the same latents and loss table, bit for bit."""
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
    inv = WPlusInverter(eng, use_plan=True)
    w1, l1 = inv.invert(target, w0, noises, steps=steps, loss_weight=beta)
    assert inv.last_plan['steps'] == [steps - 3]
    w2, l2 = inv.invert(other, w0, noises, steps=steps, loss_weight=beta)
    assert torch.equal(w1, w2) and torch.equal(l1, l2)
    w3, l3 = inv.invert(other, w0, noises, steps=steps)        # without the weight the changed pixels do count
    assert not torch.equal(l3, l1)


# ------------------------------------------------------------------------------------------------------- 'blend' vs the reference
def _ood_model(dev, size=256, **kw):
    from oodgan.arch import ood_faceGAN_e4e
    m = ood_faceGAN_e4e(out_size=size, style_dim=512, encoder='E4E', enable_modulation=kw.pop('enable_modulation', True), warp_scale=0.08,
                        cycle_align=2, blend_with_gen=kw.pop('blend_with_gen', True), ModSize=256, build_encoder=False, **kw)
    res = m.load_state_dict(synth.ood_state(size, seed=41), strict=False)
    assert not res.missing_keys and (m.modulation is None or not res.unexpected_keys), res
    return m.to(dev).eval()


def _ood_inputs(dev, size=256, B=2):
    """The inputs of tests/golden/make_wplus_masked.py (seeds 42-45)."""
    enc_lats = synth.make_latents(size, B, seed=42, std=0.3).to(dev)
    enc_feats = [f.to(dev) for f in synth.make_encoder_feats(B, seed=43)]
    x = synth.make_images(size, B, seed=44).to(dev)
    noises = [n.to(dev) for n in synth.make_noises(size, B, seed=45)]
    return x, dict(enc_lats=enc_lats, enc_feats=enc_feats, noise=noises)


def test_blend_region_256_vs_reference(dev, golden):
    from oodgan import _lib
    g = golden('wplus_masked_256.npz')
    steps = int(g['steps'])
    m = _ood_model(dev)
    x, kw = _ood_inputs(dev)
    _lib.dispatch_reset()
    out, lats, losses = m.invert(x, steps=steps, loss_region='blend', **kw)
    assert _lib.dispatch_count('composite_mse') >= 1
    beta = m.last_loss_weight
    e_beta = (beta[:, :, ::4, ::4].cpu() - g['beta_sub']).abs().max().item()
    e_curve = ((losses.double().cpu() - g['losses_f32']).abs() / g['losses_f32']).max().item()
    e_fix = ((g['losses_f32'] - g['losses_f64']).abs() / g['losses_f64']).max().item()
    e_w20 = (lats.cpu() - g['w_step20']).abs().max().item()
    print(f"'blend' 256²: beta mean {beta.double().mean(dim=(1, 2, 3)).tolist()} (reference {g['beta_mean'].tolist()}), |d beta| {e_beta:.2e}; "
          f'loss curve rel {e_curve:.2e} over {steps} steps (the fixture\'s own fp32 vs float64: {e_fix:.2e}); |w_20 - reference w_20| {e_w20:.2e}')
    assert e_beta < 1e-3
    assert e_curve < 1e-3
    assert (losses[-1] < losses[0]).all()


def test_blend_region_leaves_no_state_behind(dev):
    """'blend' runs an extra OOD forward before the loop: the loop must then do exactly what it does with that beta passed as a tensor;
    beta == 1 reproduces the default 'full' run bit for bit; 'full' passed explicitly is the default."""
    from oodgan import _lib
    m = _ood_model(dev)
    x, kw = _ood_inputs(dev)
    _, l_blend, = m.invert(x, steps=6, loss_region='blend', **kw)[1:]
    w_blend = m.ori_lats.clone()
    beta = m.last_loss_weight.clone()
    _, l_t = m.invert(x, steps=6, loss_region=beta, **kw)[1:]
    assert torch.equal(l_t, l_blend) and torch.equal(m.ori_lats, w_blend)
    _lib.dispatch_reset()
    _, l_full = m.invert(x, steps=6, **kw)[1:]
    w_full = m.ori_lats.clone()
    assert m.last_loss_weight is None and _lib.dispatch_count('composite_mse') == 0
    _, l_full2 = m.invert(x, steps=6, loss_region='full', **kw)[1:]
    assert torch.equal(l_full2, l_full) and torch.equal(m.ori_lats, w_full) and _lib.dispatch_count('composite_mse') == 0
    _, l_one = m.invert(x, steps=6, loss_region=torch.ones_like(beta), **kw)[1:]
    assert torch.equal(l_one, l_full) and torch.equal(m.ori_lats, w_full)
    assert _lib.dispatch_count('composite_mse') >= 1


# ------------------------------------------------------------------------------------------------------- plans, streams
@pytest.mark.parametrize('terms,steps', [((), 30), (('lpips',), 12), (('ssim',), 12), (('lpips', 'ssim'), 12)], ids=['none', 'lpips', 'ssim', 'lpips+ssim'])
def test_plans_and_streams_with_a_loss_weight(dev, terms, steps):
    """The recorded plan against the Python-driven loop, bit for bit, and two streams against one, for every set of terms taken on the composite
    (LPIPS on seeded weights, as tests/test_hip_lpips.py).  The added term sets run 12 steps: nine replayed ones.  The two-stream bound is the one
    of the plain masked loss for every set: the sub-batches differ from the batch in the kernels their sizes select, not in the loss."""
    from oodgan.engine import GeneratorEngine, WPlusInverter
    from oodgan.lpips import LPIPSAlex
    size, B = 256, 4
    eng = GeneratorEngine({k: v.to(dev) for k, v in synth.generator_state(size, seed=0).items()}, size)
    target = synth.make_images(size, B, seed=71).to(dev)
    noises = [n.to(dev) for n in synth.make_noises(size, B, seed=72)]
    w0 = synth.make_latents(size, B, seed=73, std=0.3).to(dev)
    beta = _beta(B, size, size, 74).to(dev)
    kw = {}
    if 'lpips' in terms:
        kw.update(lpips=LPIPSAlex({k: v.to(dev) for k, v in synth.lpips_state(0).items()}, min_max=(-1.0, 1.0)), lpips_weight=0.8)
    if 'ssim' in terms:
        kw.update(ssim_weight=0.5)
    inv = WPlusInverter(eng, use_plan=True, **kw)
    w1, l1 = inv.invert(target, w0, noises, steps=steps, loss_weight=beta)
    t1 = {k: None if v is None else v.clone() for k, v in inv.last_terms.items()}
    assert inv.last_plan['steps'] == [steps - 3] and inv.last_stats['rollbacks'] == [0]
    assert [k for k in ('lpips', 'ssim') if t1[k] is not None] == list(terms)
    inv2 = WPlusInverter(eng, use_plan=False, **kw)
    w2, l2 = inv2.invert(target, w0, noises, steps=steps, loss_weight=beta)
    assert torch.equal(w1, w2) and torch.equal(l1, l2)
    assert inv2.last_plan['steps'] == [0] and all(torch.equal(t1[k], inv2.last_terms[k]) for k in ('mse',) + tuple(terms))
    w3, l3 = inv.invert(target, w0, noises, steps=steps, streams=2, loss_weight=beta)
    rel = ((l3 - l1).abs() / l1.abs()).max().item()
    print(f'loss weight + {terms or "no term"}, 2 streams vs 1 at 256², B={B}: loss rel diff {rel:.2e}; plan {inv.last_plan}')
    assert rel < 5e-3 and inv.last_plan['steps'] == [steps - 3] * 2
    assert all(inv.last_terms[k].shape == (steps, B) for k in ('mse',) + tuple(terms))
    assert (l1[-1] < l1[0]).all()


# ------------------------------------------------------------------------------------------------------- refusals
def test_refusals(dev):
    from oodgan.engine import GeneratorEngine, WPlusInverter
    x, kw = _ood_inputs(dev, B=1)
    kw = dict(enc_lats=kw['enc_lats'][:1], enc_feats=[f[:1] for f in kw['enc_feats']], noise=[n[:1] for n in kw['noise']])
    for opts in (dict(enable_modulation=False), dict(blend_with_gen=False)):
        with pytest.raises(ValueError, match='blend'):
            _ood_model(dev, **opts).invert(x[:1], steps=2, loss_region='blend', **kw)
    m = _ood_model(dev)
    good = torch.full((1, 1, 256, 256), 0.5, device=dev)
    for bad in (torch.full((1, 3, 256, 256), 0.5, device=dev), torch.full((1, 1, 128, 128), 0.5, device=dev), good.double(), good.cpu(),
                good + 0.6, good - 0.6, good * float('nan')):
        with pytest.raises(ValueError):
            m.invert(x[:1], steps=2, loss_region=bad, **kw)
    with pytest.raises(ValueError):
        m.invert(x[:1], steps=2, loss_region='masked', **kw)
    with pytest.raises(NotImplementedError):
        m.invert(x[:1], steps=2, loss_region=good, use_graph=True, **kw)
    eng = GeneratorEngine({k: v.to(dev) for k, v in synth.generator_state(64, seed=5).items()}, 64)
    with pytest.raises(NotImplementedError):
        WPlusInverter(eng).invert(synth.make_images(64, 1, seed=1).to(dev), synth.make_latents(64, 1, seed=2).to(dev),
                                  [n.to(dev) for n in synth.make_noises(64, 1, seed=3)], steps=2, use_graph=True,
                                  loss_weight=torch.ones(1, 1, 64, 64, device=dev))
