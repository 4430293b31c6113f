"""The SSIM term of the W+ loss: L_b = MSE_b + lpips_weight LPIPS_b + ssim_weight (1 - SSIM_b).

The fused kernel (csrc/loss_ssim.hip) against the float64 yardstick of tests/ssim_ref.py; one W+ step's dL/dW+ against float64 autograd
through the oracle (plain, on the composite of a non-binary beta, and with LPIPS); a short run against the oracle's float64 Adam loop;
the term raises the SSIM the CLI reports; launch plans, streams, the range guard's rollback, the untouched default path, the refusals."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import lpips_cpu as LO  # noqa: E402
from oracle import ref_cpu as R  # noqa: E402
from oodgan import imgio, synth  # noqa: E402
from ssim_ref import ssim_loss, ssim_loss_and_grad  # noqa: E402
from wplus_grads import recover_grad  # noqa: E402


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


def _pair(kind, B, H, W, seed):
    """far: 0.6*normal clamped to +-1.3 (values outside [-1,1]); near: the target + 0.05*normal."""
    x = (0.6 * synth.normal('ssim.x', (B, 3, H, W), seed)).clamp(-1.3, 1.3)
    if kind == 'far':
        return (0.6 * synth.normal('ssim.img', (B, 3, H, W), seed + 1)).clamp(-1.3, 1.3).contiguous(), x.contiguous()
    return (x + 0.05 * synth.normal('ssim.img', (B, 3, H, W), seed + 1)).contiguous(), x.contiguous()


def _beta(B, H, W, seed):
    """A seeded, non-binary plane in [0, 1] with an exact-zero and an exact-one block (as tests/test_hip_wplus_masked.py)."""
    b = torch.sigmoid(2.0 * synth.normal('masked.beta', (B, 1, H, W), seed))
    b[:, :, : H // 4, : W // 4] = 0.0
    b[:, :, -(H // 4):, -(W // 4):] = 1.0
    return b.contiguous()


# ------------------------------------------------------------------------------------------------------------- kernel
@pytest.mark.parametrize('kind', ['far', 'near'])
@pytest.mark.parametrize('B', [1, 3, 8])
@pytest.mark.parametrize('H,W', [(256, 256), (64, 64), (37, 37), (64, 48), (11, 11)])
def test_ssim_kernel_vs_float64(dev, B, H, W, kind):
    """Bars: loss 1e-6 absolute, gradient 2e-5 of its maximum — about 4x what torch's own fp32 evaluation of the formula keeps
    (8e-8 and 4.5e-6 on these inputs)."""
    from oodgan import ops
    img, x = _pair(kind, B, H, W, 11)
    gmul = 64.0
    loss_ref, g_ref = ssim_loss_and_grad(img, x)
    a, t = img.to(dev), x.to(dev)
    z = torch.zeros_like(a)
    loss = ops.ssim_loss_grad(a, t, z, gmul)
    e_loss = (loss.double().cpu() - loss_ref).abs().max().item()
    e_g = (z.double().cpu() / gmul - g_ref).abs().max().item() / g_ref.abs().max().item()
    print(f'SSIM kernel {kind} B={B} {H}x{W}: 1-SSIM {loss_ref.min().item():.4f}..{loss_ref.max().item():.4f}, |loss err| {e_loss:.2e} (bar 1e-6), '
          f'gradient err {e_g:.2e} of max (bar 2e-5)')
    assert e_loss <= 1e-6
    assert e_g <= 2e-5
    # accumulated into, not overwritten: g = g0 + z up to one rounding of the sum
    g0 = synth.normal('ssim.g0', (B, 3, H, W), 13).to(dev) * z.abs().max()
    g = g0.clone()
    assert torch.equal(ops.ssim_loss_grad(a, t, g, gmul), loss)
    assert (g - (g0 + z)).abs().max().item() <= 1e-6 * (g0.abs().max().item() + z.abs().max().item())
    assert not torch.equal(g, z)
    # forward only: the same value bit for bit; two identical calls are bit-equal
    assert torch.equal(ops.ssim_loss_grad(a, t), loss)
    z2 = torch.zeros_like(z)
    assert torch.equal(ops.ssim_loss_grad(a, t, z2, gmul), loss) and torch.equal(z2, z)
    # the loss-table form writes row row_dev[0] (clamped to the table) and nothing else
    table = torch.full((4, B), -1.0, device=dev)
    for row in (2, 9):
        row_dev = torch.tensor([row], dtype=torch.int32, device=dev)
        z3 = torch.zeros_like(z)
        assert ops.ssim_loss_grad(a, t, z3, gmul, table=table, row_dev=row_dev) is None
        assert torch.equal(table[min(row, 3)], loss) and torch.equal(z3, z)
    assert torch.equal(table[:2], torch.full((2, B), -1.0, device=dev))


def test_ssim_kernel_refuses_small_images(dev):
    from oodgan import _lib, ops
    for shape in ((1, 3, 10, 64), (1, 3, 64, 10)):
        a = torch.zeros(shape, device=dev)
        with pytest.raises(RuntimeError, match='11'):
            ops.ssim_loss_grad(a, a)
    h = _lib.lib()
    assert h.oodgan_ssim_loss_fwd_bwd(None, None, None, None, None, 1, 3, 64, 64, 1.0, None) == -1 and b'ssim' in h.oodgan_last_error()


# ------------------------------------------------------------------------------------------------------- W+ step gradients
def _step_grads(inv, target, w0, noises, beta=None):
    """One step of the loop; its dL/dW+ recovered from Adam's first moment (tests/wplus_grads.py)."""
    caps = {}
    inv.on_step = lambda run: caps.__setitem__(run.t, run.m.clone())
    _, losses = inv.invert(target, w0, noises, steps=1, loss_weight=beta)
    torch.cuda.synchronize()
    assert inv.last_stats['rollbacks'] == [0]
    return recover_grad(torch.zeros_like(caps[1]).cpu(), caps[1].cpu(), inv.betas[0]), losses


@pytest.mark.parametrize('masked', [False, True])
@pytest.mark.parametrize('prec,bar', [('f16s', 1e-4), ('f16s-g2', 3e-4)])
def test_wplus_step_256_vs_float64_autograd(dev, prec, bar, masked):
    """dL/dW+ of the first W+ step at 256² with L = MSE + 0.5 (1 - SSIM), plain and on the composite of a non-binary beta (the bars of
    tests/test_hip_wplus_masked.py)."""
    from oodgan import _lib
    from oodgan.engine import GeneratorEngine, WPlusInverter
    size, B, lam = 256, 2, 0.5
    P = synth.generator_state(size, seed=0)
    target = synth.make_images(size, B, seed=61)
    noises = synth.make_noises(size, B, seed=62)
    w0 = synth.make_latents(size, B, seed=63, std=0.3)
    beta = _beta(B, size, size, 64) if masked else None
    w = w0.double().clone().requires_grad_(True)
    img = R.generator_forward({k: v.double() for k, v in P.items()}, w, [n.double() for n in noises], size)
    c = img if beta is None else target.double() + beta.double() * (img - target.double())
    mse_ref, ss_ref = ((c - target.double()) ** 2).mean(dim=(1, 2, 3)), ssim_loss(c, target.double())
    loss_ref = mse_ref + lam * ss_ref
    loss_ref.sum().backward()
    eng = GeneratorEngine({k: v.to(dev) for k, v in P.items()}, size, precision=prec)
    _lib.dispatch_reset()
    inv = WPlusInverter(eng, ssim_weight=lam)
    g, losses = _step_grads(inv, target.to(dev), w0.to(dev), [n.to(dev) for n in noises], None if beta is None else beta.to(dev))
    assert _lib.dispatch_count('ssim') == 1
    rel = (g - w.grad).abs().max().item() / w.grad.abs().max().item()
    e_loss = ((losses[0].double().cpu() - loss_ref.detach()).abs() / loss_ref.detach()).max().item()
    e_ss = (inv.last_terms['ssim'][0].double().cpu() - ss_ref.detach()).abs().max().item()
    print(f'W+ step 256² + SSIM {prec} masked={masked}: dL/dW+ rel {rel:.2e} (bar {bar:g}), loss rel {e_loss:.2e}, |1-SSIM err| {e_ss:.2e}; '
          f'terms mse {mse_ref.tolist()} 1-ssim {ss_ref.tolist()}')
    assert rel < bar and e_loss < 1e-5
    assert inv.last_terms['lpips'] is None and inv.last_terms['ssim'].shape == (1, B)


@pytest.mark.parametrize('prec,bar', [('f16s', 1e-4), ('f16s-g2', 3e-4)])
def test_wplus_step_64_mse_lpips_ssim_vs_float64_autograd(dev, prec, bar):
    """All three terms together (LPIPS on seeded weights).  A ReLU or max-pool decision within rounding flips between fp32 and float64
    (test_hip_lpips.py): as in test_hip_wplus_masked.py the bar is also met against the oracle's own fp32 autograd where that is closer, and
    is never looser than 3x the oracle's fp32-vs-float64 distance."""
    from oodgan.engine import GeneratorEngine, WPlusInverter
    from oodgan.lpips import LPIPSAlex
    size, B, lam, lam_s = 64, 2, 0.8, 0.5
    P, PL = synth.generator_state(size, seed=5), synth.lpips_state(0)
    target = synth.make_images(size, B, seed=9)
    noises = synth.make_noises(size, B, seed=7)
    w0 = synth.make_latents(size, B, seed=14)

    def oracle(dt):
        w = w0.to(dt).clone().requires_grad_(True)
        img = R.generator_forward({k: v.to(dt) for k, v in P.items()}, w, [n.to(dt) for n in noises], size)
        mse = ((img - target.to(dt)) ** 2).mean(dim=(1, 2, 3))
        _, lp = LO.lpips_loss({k: v.to(dt) for k, v in PL.items()}, img, target.to(dt), min_max=(-1.0, 1.0), reduction='none')
        tot = mse + lam * lp + lam_s * ssim_loss(img, target.to(dt))
        tot.sum().backward()
        return w.grad.double(), tot.detach().double()

    g64, l64 = oracle(torch.float64)
    g32, _ = oracle(torch.float32)
    eng = GeneratorEngine({k: v.to(dev) for k, v in P.items()}, size, precision=prec)
    net = LPIPSAlex({k: v.to(dev) for k, v in PL.items()}, min_max=(-1.0, 1.0))
    inv = WPlusInverter(eng, lpips=net, lpips_weight=lam, ssim_weight=lam_s)
    g, losses = _step_grads(inv, target.to(dev), w0.to(dev), [n.to(dev) for n in noises])
    scale = g64.abs().max().item()
    rel, rel32, e_self = ((g - g64).abs().max().item() / scale, (g - g32).abs().max().item() / scale, (g32 - g64).abs().max().item() / scale)
    e_loss = ((losses[0].double().cpu() - l64).abs() / l64).max().item()
    print(f'W+ step 64² MSE + LPIPS + SSIM {prec}: dL/dW+ rel {rel:.2e} vs f64, {rel32:.2e} vs the f32 oracle (oracle f32 vs f64 {e_self:.2e}; '
          f'bar {bar:g}), loss rel {e_loss:.2e}')
    assert min(rel, rel32) < max(bar, 3 * e_self) and e_loss < 1e-4
    t = inv.last_terms
    assert torch.equal(losses, t['mse'] + lam * t['lpips'] + lam_s * t['ssim'])


# ------------------------------------------------------------------------------------------------------- short runs
_RUN = dict(size=64, B=2, steps=20)
_ORACLE = {}


def _oracle_run(dt, lam):
    """The oracle's autograd + torch.optim.Adam loop with L = MSE + lam (1 - SSIM) in dtype ``dt``: (total losses[steps,B], 1 - SSIM
    tables, SSIM of G(w_final) against the target by imgio.calculate_ssim on the float images)."""
    key = (dt, lam)
    if key not in _ORACLE:
        size, B, steps = _RUN['size'], _RUN['B'], _RUN['steps']
        P = {k: v.to(dt) for k, v in synth.generator_state(size, seed=5).items()}
        x = synth.make_images(size, B, seed=9).to(dt)
        noises = [n.to(dt) for n in synth.make_noises(size, B, seed=7)]
        w = synth.make_latents(size, B, seed=14).to(dt).requires_grad_(True)
        opt = torch.optim.Adam([w], lr=0.01, betas=(0.9, 0.999), eps=1e-8)
        tot, ss = [], []
        for _ in range(steps):
            opt.zero_grad(set_to_none=True)
            img = R.generator_forward(P, w, noises, size)
            s = ssim_loss(img, x)
            t = ((img - x) ** 2).mean(dim=(1, 2, 3)) + (lam * s if lam else 0.0)
            t.sum().backward()
            tot.append(t.detach().clone())
            ss.append(s.detach().clone())
            opt.step()
        with torch.no_grad():
            img = R.generator_forward(P, w, noises, size)
        _ORACLE[key] = (torch.stack(tot).double(), torch.stack(ss).double(), _reported_ssim(img, x))
    return _ORACLE[key]


def _reported_ssim(img, x):
    """imgio.calculate_ssim per image on the float [0,255] images (no clamp, no rounding)."""
    f = lambda t: (127.5 * (t.detach().double().cpu() + 1.0)).permute(1, 2, 0).numpy()
    return [imgio.calculate_ssim(f(img[b]), f(x[b]), crop_border=0, test_y_channel=False) for b in range(img.shape[0])]


def _hip_run(dev, lam, **kw):
    from oodgan.engine import GeneratorEngine, WPlusInverter
    size, B, steps = _RUN['size'], _RUN['B'], _RUN['steps']
    eng = GeneratorEngine({k: v.to(dev) for k, v in synth.generator_state(size, seed=5).items()}, size)
    x = synth.make_images(size, B, seed=9).to(dev)
    noises = [n.to(dev) for n in synth.make_noises(size, B, seed=7)]
    inv = WPlusInverter(eng, ssim_weight=lam, **kw)
    w, losses = inv.invert(x, synth.make_latents(size, B, seed=14).to(dev), noises, steps=steps)
    return inv, w, losses, _reported_ssim(eng.forward(w, noises), x)


def test_short_run_vs_the_oracle_loop(dev):
    """20 steps at 64² with ssim_weight 0.5: the total-loss curve within max(1e-3, 3x the oracle's own fp32-vs-float64 distance)."""
    lam = 0.5
    l64, s64, _ = _oracle_run(torch.float64, lam)
    l32, _, _ = _oracle_run(torch.float32, lam)
    e_self = ((l32 - l64).abs() / l64).max().item()
    inv, w, losses, _ = _hip_run(dev, lam)
    e_curve = ((losses.double().cpu() - l64).abs() / l64).max().item()
    t = inv.last_terms
    e_terms = (t['ssim'].double() - (losses.double() - t['mse'].double()) / lam).abs().max().item()
    e_ss = (t['ssim'].double().cpu() - s64).abs().max().item()
    print(f'20 steps 64² MSE + 0.5 (1 - SSIM): loss curve rel {e_curve:.2e} vs the float64 oracle loop (its own fp32 loop: {e_self:.2e}); '
          f'|1-SSIM table - oracle| {e_ss:.2e}; (losses - mse)/lam vs the ssim table {e_terms:.2e}; stats {inv.last_stats}')
    assert e_curve < max(1e-3, 3 * e_self)
    assert e_terms < 1e-5                       # fp32 rounding of the total at |loss| <~ 8
    assert inv.last_stats == {'steps_run': [_RUN['steps']], 'rollbacks': [0]}
    assert not inv.engine.bwd_scale_violated() and not inv.engine.fwd_range_violated()
    assert (losses[-1] < losses[0]).all()


def test_the_term_raises_the_reported_ssim(dev):
    """Same start, noise and steps, ssim_weight 2 against 0: the SSIM of G(w) against the target that the CLI would report
    (imgio.calculate_ssim) is higher with the term — in the float64 oracle loop alone first (measured on the CPU: 0.00843 / 0.01105 with
    the term, 0.00621 / 0.00919 without, on these seeded noise-like images), then for the HIP loop."""
    lam = 2.0
    _, _, with64 = _oracle_run(torch.float64, lam)
    _, _, without64 = _oracle_run(torch.float64, 0.0)
    print(f'oracle float64, 20 steps: SSIM with the term {with64}, without {without64}')
    assert all(a > b for a, b in zip(with64, without64))
    _, _, _, with_hip = _hip_run(dev, lam)
    _, _, _, without_hip = _hip_run(dev, 0.0)
    print(f'HIP, 20 steps: SSIM with the term {with_hip}, without {without_hip}')
    assert all(a > b for a, b in zip(with_hip, without_hip))


# ------------------------------------------------------------------------------------------------------- plumbing
def test_plans_and_streams(dev):
    from oodgan.engine import GeneratorEngine, WPlusInverter
    size, B, steps, lam = 256, 4, 30, 0.5
    eng = GeneratorEngine({k: v.to(dev) for k, v in synth.generator_state(size, seed=0).items()}, size)
    target = synth.make_images(size, B, seed=71).to(dev)
    noises = [n.to(dev) for n in synth.make_noises(size, B, seed=72)]
    w0 = synth.make_latents(size, B, seed=73, std=0.3).to(dev)
    inv = WPlusInverter(eng, use_plan=True, ssim_weight=lam)
    w1, l1 = inv.invert(target, w0, noises, steps=steps)
    s1 = inv.last_terms['ssim'].clone()
    assert inv.last_plan['steps'] == [steps - 3] and inv.last_stats['rollbacks'] == [0]
    inv2 = WPlusInverter(eng, use_plan=False, ssim_weight=lam)
    w2, l2 = inv2.invert(target, w0, noises, steps=steps)
    assert torch.equal(w1, w2) and torch.equal(l1, l2) and torch.equal(s1, inv2.last_terms['ssim'])
    w3, l3 = inv.invert(target, w0, noises, steps=steps, streams=2)
    rel = ((l3 - l1).abs() / l1.abs()).max().item()
    print(f'SSIM term, 2 streams vs 1 at 256², B={B}: loss rel diff {rel:.2e}; plan {inv.last_plan}')
    assert rel < 5e-3 and inv.last_plan['steps'] == [steps - 3] * 2
    s3 = inv.last_terms['ssim']
    assert s3.shape == (steps, B) and ((s3 - s1).abs() / s1).max().item() < 5e-3
    assert (l1[-1] < l1[0]).all()


@pytest.mark.parametrize('use_plan', [True, False])
def test_rollback_leaves_a_complete_ssim_table(dev, use_plan):
    """A forward scale sabotaged after step 15 of 40 (as tests/test_hip_wplus_long.py): the window is repeated with exact scales and its rows
    of the third table are simply rewritten."""
    from oodgan.engine import GeneratorEngine, WPlusInverter
    size, B, steps, lam = 32, 2, 40, 0.5
    eng = GeneratorEngine({k: v.to(dev) for k, v in synth.generator_state(size, seed=5).items()}, size)
    target = synth.make_images(size, B, seed=9).to(dev)
    noises = [n.to(dev) for n in synth.make_noises(size, B, seed=7)]
    w0 = synth.make_latents(size, B, seed=14).to(dev)
    inv = WPlusInverter(eng, use_plan=use_plan, ssim_weight=lam)
    w_ref, l_ref = inv.invert(target, w0, noises, steps=steps)
    s_ref = inv.last_terms['ssim'].clone()
    assert inv.last_stats == {'steps_run': [steps], 'rollbacks': [0]}
    done = {'n': 0}

    def sabotage(run):
        if run.steps_run == 15 and not done['n']:
            done['n'] = 1
            eng.fwd_range.q[3].mul_(2.0 ** 12)
    inv.on_step = sabotage
    w, l = inv.invert(target, w0, noises, steps=steps)
    inv.on_step = None
    s = inv.last_terms['ssim']
    print(f'forward scale sabotaged after step 15 of {steps} with the SSIM term (plans {use_plan}): {inv.last_stats}; '
          f'|ssim table - undisturbed| {(s - s_ref).abs().max().item():.2e}')
    assert inv.last_stats['rollbacks'] == [1] and inv.last_stats['steps_run'][0] == steps + inv.check_every + inv.check_lag
    # complete: the table starts as zeros and 1 - SSIM > 0 here, so a row the repeated window or the re-recorded plan skipped would read 0
    assert s.shape == (steps, B) and (s > 0).all() and torch.isfinite(s).all()
    # the rows before the clean snapshot (step 10) were never rewritten: bit-identical to the undisturbed run
    assert torch.equal(s[:inv.check_every], s_ref[:inv.check_every]) and torch.equal(l[:inv.check_every], l_ref[:inv.check_every])
    # from there on ten steps ran with exact instead of carried scales — rounding-level differences that Adam amplifies (test_hip_wplus_long.py
    # accepts |dw| up to 5e-3 for this): the runs agree as two runs whose arithmetic differs by rounding do (1e-3 relative on the losses, the
    # bar of oodgan.arch's invert() for sub-batch / stream changes), not bit for bit
    assert ((s - s_ref).abs() / s_ref).max().item() < 1e-3
    assert ((l - l_ref).abs() / l_ref).max().item() < 1e-3
    assert torch.equal(l, inv.last_terms['mse'] + lam * s)


def _ood_model(dev, size=256):
    from oodgan.arch import ood_faceGAN_e4e
    m = ood_faceGAN_e4e(out_size=size, style_dim=512, encoder='E4E', enable_modulation=True, warp_scale=0.08, cycle_align=2, blend_with_gen=True,
                        ModSize=256, build_encoder=False)
    res = m.load_state_dict(synth.ood_state(size, seed=41), strict=False)
    assert not res.missing_keys and not res.unexpected_keys, res
    return m.to(dev).eval()


def test_model_invert_default_is_untouched_and_refusals(dev):
    from oodgan import _lib
    size, B = 256, 2
    m = _ood_model(dev, size)
    x = synth.make_images(size, B, seed=44).to(dev)
    kw = dict(enc_lats=synth.make_latents(size, B, seed=42, std=0.3).to(dev), enc_feats=[f.to(dev) for f in synth.make_encoder_feats(B, seed=43)],
              noise=[n.to(dev) for n in synth.make_noises(size, B, seed=45)])
    _lib.dispatch_reset()
    out0, lats0, l0 = m.invert(x, steps=6, **kw)
    plan0 = m.last_invert_plan
    assert m.last_loss_terms['ssim'] is None
    out1, lats1, l1 = m.invert(x, steps=6, ssim_weight=0.0, **kw)
    assert torch.equal(l0, l1) and torch.equal(lats0, lats1) and torch.equal(out0, out1)
    assert m.last_invert_plan['launches'] == plan0['launches'] and m.last_loss_terms['ssim'] is None
    assert _lib.dispatch_count('ssim') == 0
    out2, lats2, l2 = m.invert(x, steps=6, ssim_weight=0.5, **kw)
    t = m.last_loss_terms
    assert t['ssim'].shape == (6, B) and (t['ssim'] > 0).all() and torch.equal(l2, t['mse'] + 0.5 * t['ssim'])
    assert _lib.dispatch_count('ssim') >= 1 and m.last_invert_plan['launches'][0] == plan0['launches'][0] + 2      # the fused kernel + its finish
    # with a region the term runs on the composite (checked against float64 in test_wplus_step_256_vs_float64_autograd[masked])
    out3, _, l3 = m.invert(x, steps=6, ssim_weight=0.5, loss_region='blend', **kw)
    assert m.last_loss_terms['ssim'].shape == (6, B) and torch.isfinite(l3).all()
    for bad in (-1.0, float('nan'), float('inf')):
        with pytest.raises(ValueError, match='ssim_weight'):
            m.invert(x, steps=2, ssim_weight=bad, **kw)
    with pytest.raises(NotImplementedError):
        m.invert(x, steps=2, ssim_weight=0.5, use_graph=True, **kw)


def test_one_step_at_1024(dev):
    """One 1024² step at B=2: the table's 1 - SSIM against the float64 yardstick evaluated on the HIP image of that step."""
    from oodgan.engine import GeneratorEngine, WPlusInverter
    size, B, lam = 1024, 2, 0.5
    eng = GeneratorEngine({k: v.to(dev) for k, v in synth.generator_state(size, seed=0).items()}, size)
    target = synth.make_images(size, B, seed=81).to(dev)
    noises = [n.to(dev) for n in synth.make_noises(size, B, seed=82)]
    w0 = synth.make_latents(size, B, seed=83, std=0.3).to(dev)
    inv = WPlusInverter(eng, ssim_weight=lam)
    w, losses = inv.invert(target, w0, noises, steps=1)
    torch.cuda.synchronize()
    assert inv.last_stats == {'steps_run': [1], 'rollbacks': [0]} and torch.isfinite(w).all() and torch.isfinite(losses).all()
    eng.reset_bwd_state()
    eng.reset_fwd_state()
    img = eng.forward(w0, noises, save=True, range_mode='carry')          # the step's own forward: first step of a run, exact scales
    eng.saved = None
    ref = ssim_loss(img.double().cpu(), target.double().cpu())
    err = (inv.last_terms['ssim'][0].double().cpu() - ref).abs().max().item()
    print(f'1024² B={B} step: 1 - SSIM {inv.last_terms["ssim"][0].tolist()}, |err| vs float64 on the HIP image {err:.2e}')
    assert err < 1e-6
    assert torch.equal(losses, inv.last_terms['mse'] + lam * inv.last_terms['ssim'])
