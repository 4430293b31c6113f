"""The LPIPS term of the W+ loss on an area-pooled view (``lpips_size``): pool -> LPIPS at the small size -> the pool's adjoint.

The oracle is the composed function in float64: oracle.lpips_cpu.lpips_loss(avg_pool2d(pred), avg_pool2d(target)) with autograd down to the
full-resolution image or, in the loop, through oracle.ref_cpu's generator down to the latents.  PARITY UNPINNED as in test_hip_lpips.py: both
sides run the published algorithm on the same seeded weights.

The loop tests weigh LPIPS with lambda = 1000.  At the lambda = 0.8 of test_hip_lpips.py the pooled LPIPS gradient is under 0.3 % of the step's
gradient at these seeds (|dMSE/dw| ~ 9.6 and 4.2, |dLPIPS/dw| ~ 0.0057 and 0.0145 per image), so a wrong pooled gradient would pass a 1e-4 bar
unseen; the oracle asserts lambda |dLPIPS/dw| >= 0.3 |dMSE/dw| for every image at step 1."""
import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import wplus_grads as WG  # noqa: E402
from oracle import lpips_cpu as LO  # noqa: E402
from oracle import ref_cpu as R  # noqa: E402
from oodgan import synth  # noqa: E402

MM = (-1.0, 1.0)
LAM = 1000.0
SIZE, POOLED, NB, STEPS = 128, 64, 2, 6


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


def _rel(a, b):
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


def _net(dev):
    from oodgan.lpips import LPIPSAlex
    return LPIPSAlex({k: v.to(dev) for k, v in synth.lpips_state(0).items()}, min_max=MM)


# ------------------------------------------------------------------------------------------------------- value and image gradient
@pytest.mark.parametrize('size,f,B', [(128, 2, 2), (256, 4, 1)])
def test_pooled_lpips_value_and_image_gradient_vs_oracle(dev, size, f, B):
    """area_pool -> loss_and_grad(xs, gs, grad_mul=4) -> area_pool_bwd_add into a non-zero gimg0, against float64 autograd of the composed
    function; the acceptance rule of test_lpips_value_and_image_gradient_vs_oracle, no pixel excluded."""
    from oodgan import ops
    P = synth.lpips_state(0)
    P64 = {k: v.double() for k, v in P.items()}
    pred, target = synth.make_images(size, B, seed=11), synth.make_images(size, B, seed=12)

    def oracle(dt, state):
        p = pred.to(dt).requires_grad_(True)
        per = LO.lpips_loss(state, F.avg_pool2d(p, f), F.avg_pool2d(target.to(dt), f), min_max=MM, reduction='none')[1]
        per.sum().backward()
        return per.detach().double(), p.grad.double()

    per_ref, g64 = oracle(torch.float64, P64)
    _, g32 = oracle(torch.float32, P)
    net = _net(dev)
    pd, td = pred.to(dev), target.to(dev)
    net.set_target(ops.area_pool(td, f))
    gimg0 = synth.normal('lpp.g0', (B, 3, size, size), 5, 1e-3).to(dev)
    gimg = gimg0.clone()
    xs, gs = ops.area_pool(pd, f, grad_buffer=True)
    per = net.loss_and_grad(xs, gs, grad_mul=4.0)
    ops.area_pool_bwd_add(gs, gimg, f)
    e_l = _rel(per.double().cpu(), per_ref)
    gmine = (gimg - gimg0).double().cpu() / 4.0
    gmax = g64.abs().max()
    e_g, e_g32 = float((gmine - g64).abs().max() / gmax), float((gmine - g32).abs().max() / gmax)
    e_self = float((g32 - g64).abs().max() / gmax)
    print(f'pooled LPIPS {size}² -> {size // f}² B={B}: values {per.tolist()} (oracle {per_ref.tolist()}), rel {e_l:.2e}; d/dimage rel {e_g:.2e} vs the '
          f'f64 oracle, {e_g32:.2e} vs the f32 oracle; oracle f32 vs f64: {e_self:.2e}')
    assert e_l < 1e-4
    assert min(e_g, e_g32) < max(1e-3, 3 * e_self), (e_g, e_g32, e_self)


# ------------------------------------------------------------------------------------------------------- the loop
@functools.lru_cache(maxsize=None)
def _loop_inputs():
    return (synth.generator_state(SIZE, seed=5), synth.lpips_state(0), synth.make_images(SIZE, NB, seed=9), synth.make_noises(SIZE, NB, seed=7),
            synth.make_latents(SIZE, NB, seed=14))


def _beta():
    """A seeded plane in [0, 1] with a block of exact zeros."""
    b = torch.sigmoid(2.0 * synth.normal('lpp.beta', (NB, 1, SIZE, SIZE), 21))
    b[:, :, 40:72, 24:88] = 0.0
    return b.contiguous()


_ORACLE = {}


def _oracle_step(k, w_row, dt, beta=None, parts=False):
    """Image k at the latents ``w_row``: (dL/dw, pooled LPIPS value) of L = MSE + LAM * LPIPS(avg_pool2d(c), avg_pool2d(x)) in ``dt``, c = G(w) or,
    with ``beta``, the composite x + beta (G(w) - x) (the pixel term is then mean (c - x)^2).  ``parts``: (dMSE/dw, dLPIPS/dw) instead.
    Computed once per (image, latents, dtype, weight) and shared: the configurations start from the same latents."""
    key = (k, w_row.detach().cpu().double().numpy().tobytes(), dt, beta is not None, parts)
    if key not in _ORACLE:
        _ORACLE[key] = _oracle_step_once(k, w_row, dt, beta, parts)
    return _ORACLE[key]


def _oracle_step_once(k, w_row, dt, beta, parts):
    P, PL, target, noises, _ = _loop_inputs()
    Pd, PLd = {n: v.to(dt) for n, v in P.items()}, {n: v.to(dt) for n, v in PL.items()}
    f = SIZE // POOLED
    w = w_row.detach().cpu().to(dt).reshape(1, -1, w_row.shape[-1]).clone().requires_grad_(True)
    x = target[k:k + 1].to(dt)
    img = R.generator_forward(Pd, w, [n[k:k + 1].to(dt) for n in noises], SIZE)
    c = img if beta is None else x + beta[k:k + 1].to(dt) * (img - x)
    mse = ((c - x) ** 2).mean()
    lp = LO.lpips_loss(PLd, F.avg_pool2d(c, f), F.avg_pool2d(x, f), min_max=MM, reduction='none')[1].sum()
    if parts:
        g_mse, = torch.autograd.grad(mse, w, retain_graph=True)
        g_lp, = torch.autograd.grad(lp, w)
        return g_mse[0].double(), g_lp[0].double()
    (mse + LAM * lp).backward()
    return w.grad[0].double(), float(lp.detach())


@functools.lru_cache(maxsize=None)
def _lambda_is_large_enough():
    """In the oracle at the start latents: lambda |dLPIPS/dw| >= 0.3 |dMSE/dw| (2-norms) for every image, so the pooled gradient is seen."""
    w0 = _loop_inputs()[4]
    out = []
    for k in range(NB):
        g_mse, g_lp = _oracle_step(k, w0[k], torch.float64, parts=True)
        out.append((float(g_mse.norm()), float(g_lp.norm())))
    return out


def _lpips_launches(net, B, size, dev):
    """Launches of one loss_and_grad call into a loss table at (B,3,size,size), counted by recording it (the plan is never run)."""
    from oodgan import ops
    x = synth.make_images(size, B, seed=31).to(dev)
    g, table, row = torch.zeros_like(x), torch.zeros(2, B, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)
    taps = net.target_taps(synth.make_images(size, B, seed=32).to(dev))
    plan = ops.LaunchPlan()
    with plan.recording():
        net.loss_and_grad(x, g, 1.0, table=table, row_dev=row, target_taps=taps)
    torch.cuda.synchronize()
    return plan.size


@pytest.mark.parametrize('streams,use_plan', [(1, False), (1, True), (2, True)])
def test_wplus_step_gradients_with_pooled_lpips_vs_float64(dev, streams, use_plan):
    """dL/dW+ of step 1 and of step 5 (replayed from the plan where one is used), recovered from Adam's first moment, against float64 autograd
    of MSE + 1000 * LPIPS(avg_pool2d(G(w)), avg_pool2d(x)) at the captured latents; bar max(1e-4, 3 x the oracle's own fp32-vs-float64)."""
    from oodgan import _lib
    from oodgan.engine import GeneratorEngine, WPlusInverter
    P, PL, target, noises, w0 = _loop_inputs()
    for g_mse, g_lp in _lambda_is_large_enough():
        print(f'oracle at step 1: |dMSE/dw| {g_mse:.3g}, |dLPIPS/dw| {g_lp:.3g}, lambda |dLPIPS/dw| / |dMSE/dw| = {LAM * g_lp / g_mse:.2f}')
        assert LAM * g_lp >= 0.3 * g_mse
    eng = GeneratorEngine({k: v.to(dev) for k, v in P.items()}, SIZE)
    net = _net(dev)
    args = (target.to(dev), w0.to(dev), [n.to(dev) for n in noises])
    inv = WPlusInverter(eng, lpips=net, lpips_weight=LAM, lpips_size=POOLED, use_plan=use_plan)
    cap = WG.capture(inv)
    before = _lib.dispatch_count('area_pool')
    _, losses = inv.invert(*args, steps=STEPS, streams=streams)
    torch.cuda.synchronize()
    assert inv.last_stats == {'steps_run': [STEPS] * streams, 'rollbacks': [0] * streams}, inv.last_stats
    assert inv.last_plan['steps'] == ([STEPS - 3] * streams if use_plan else [0] * streams)
    # host-side counter: the target's pool once per run, two calls per step that was driven from Python (replayed steps do not count)
    eager = STEPS - inv.last_plan['steps'][0]
    assert _lib.dispatch_count('area_pool') == before + streams * (1 + 2 * eager)
    lp_rows = inv.last_terms['lpips'].double().cpu()
    assert torch.isfinite(losses).all()
    fails = []
    for k in range(NB):
        for t in (1, 5):
            g = cap.grad(k, t, inv.betas[0])
            w_prev = cap.w(k, t - 1)
            g64, lp64 = _oracle_step(k, w_prev, torch.float64)
            g32, _ = _oracle_step(k, w_prev, torch.float32)
            e_self = float((g32 - g64).abs().max() / g64.abs().max())
            rel = float((g - g64).abs().max() / g64.abs().max())
            e_lp = abs(float(lp_rows[t - 1, k]) - lp64) / lp64
            bar = max(1e-4, 3 * e_self)
            print(f'pooled LPIPS W+ (streams {streams}, plan {use_plan}) image {k} step {t}: dL/dw rel {rel:.2e} (bar {bar:.2e}; oracle f32 vs f64 '
                  f'{e_self:.2e}), lpips row rel {e_lp:.2e}')
            if not rel < bar:
                fails.append(f'image {k} step {t}: dL/dw {rel:.2e} >= {bar:.2e}')
            if not e_lp < 1e-3:
                fails.append(f'image {k} step {t}: lpips row {e_lp:.2e}')
    assert not fails, '; '.join(fails)
    if use_plan:
        # the recorded step against the same run at full resolution: the two pool launches more, and the LPIPS stack's own launches at the
        # pooled size in place of those at the image size (both counted by recording the call alone at the sub-batch's size)
        full = WPlusInverter(eng, lpips=net, lpips_weight=LAM, use_plan=True)
        full.invert(*args, steps=STEPS, streams=streams)
        n_full, n_pooled = _lpips_launches(net, NB // streams, SIZE, dev), _lpips_launches(net, NB // streams, POOLED, dev)
        print(f'launches per recorded step: pooled {inv.last_plan["launches"]}, full resolution {full.last_plan["launches"]}; one LPIPS call: '
              f'{n_full} at {SIZE}², {n_pooled} at {POOLED}²')
        assert inv.last_plan['launches'] == [n - n_full + n_pooled + 2 for n in full.last_plan['launches']]


def test_wplus_step_gradient_on_the_composite_vs_float64(dev):
    """Step 1 with a loss weight beta (a block of zeros in it): LPIPS on avg_pool2d(c), c = x + beta (G - x); the gradient to G carries beta once."""
    from oodgan.engine import GeneratorEngine, WPlusInverter
    P, PL, target, noises, w0 = _loop_inputs()
    beta = _beta()
    eng = GeneratorEngine({k: v.to(dev) for k, v in P.items()}, SIZE)
    inv = WPlusInverter(eng, lpips=_net(dev), lpips_weight=LAM, lpips_size=POOLED, use_plan=False)
    caps = {}
    inv.on_step = lambda run: caps.__setitem__(run.t, run.m.clone())
    inv.invert(target.to(dev), w0.to(dev), [n.to(dev) for n in noises], steps=1, loss_weight=beta.to(dev))
    torch.cuda.synchronize()
    assert inv.last_stats['rollbacks'] == [0]
    g = WG.recover_grad(torch.zeros_like(caps[1]).cpu(), caps[1].cpu(), inv.betas[0])
    lp_row = inv.last_terms['lpips'].double().cpu()
    for k in range(NB):
        g64, lp64 = _oracle_step(k, w0[k], torch.float64, beta)
        g32, _ = _oracle_step(k, w0[k], torch.float32, beta)
        g_plain, _ = _oracle_step(k, w0[k], torch.float64)
        e_self = float((g32 - g64).abs().max() / g64.abs().max())
        rel = float((g[k] - g64).abs().max() / g64.abs().max())
        off = float((g_plain - g64).abs().max() / g64.abs().max())
        e_lp = abs(float(lp_row[0, k]) - lp64) / lp64
        print(f'pooled LPIPS on the composite, image {k}: dL/dw rel {rel:.2e} (bar max(1e-4, 3 x {e_self:.2e})), lpips row rel {e_lp:.2e}; '
              f'the oracle without beta is {off:.2e} away')
        assert off > 1e-2                                            # the weight matters at these seeds
        assert rel < max(1e-4, 3 * e_self) and e_lp < 1e-3


# ------------------------------------------------------------------------------------------------------- the default, plans
def test_the_default_path_is_unchanged(dev):
    """At 64², lambda = 0.8: lpips_size=None, lpips_size=64 (the image size) and the constructor's default give the same bits, the same launch
    list, and no pool launch."""
    from oodgan import _lib
    from oodgan.engine import GeneratorEngine, WPlusInverter
    size, B, steps = 64, 2, 6
    eng = GeneratorEngine({k: v.to(dev) for k, v in synth.generator_state(size, seed=5).items()}, size)
    net = _net(dev)
    args = (synth.make_images(size, B, seed=9).to(dev), synth.make_latents(size, B, seed=14).to(dev), [n.to(dev) for n in synth.make_noises(size, B, seed=7)])
    before = _lib.dispatch_count('area_pool')
    runs = []
    for kw in ({}, {'lpips_size': None}, {'lpips_size': 64}):
        inv = WPlusInverter(eng, lpips=net, lpips_weight=0.8, **kw)
        w, losses = inv.invert(*args, steps=steps)
        runs.append((w, losses, inv.last_terms['lpips'].clone(), inv.last_terms['mse'].clone(), inv.last_plan))
    for r in runs[1:]:
        assert all(torch.equal(a, b) for a, b in zip(r[:4], runs[0][:4])) and r[4] == runs[0][4]
    assert runs[0][4]['steps'] == [steps - 3]
    assert _lib.dispatch_count('area_pool') == before


def test_plan_replay_is_bit_identical_to_the_python_driven_loop(dev):
    """lpips_size=64 at 128²: a buffer born inside the recording that the replay then misses would show here."""
    from oodgan.engine import GeneratorEngine, WPlusInverter
    P, PL, target, noises, w0 = _loop_inputs()
    eng = GeneratorEngine({k: v.to(dev) for k, v in P.items()}, SIZE)
    net = _net(dev)
    args = (target.to(dev), w0.to(dev), [n.to(dev) for n in noises])
    out = []
    for use_plan in (True, False):
        inv = WPlusInverter(eng, lpips=net, lpips_weight=0.8, lpips_size=POOLED, use_plan=use_plan)
        w, losses = inv.invert(*args, steps=8)
        assert inv.last_plan['steps'] == ([5] if use_plan else [0]) and inv.last_stats['rollbacks'] == [0]
        out.append((w, losses, inv.last_terms['lpips'].clone(), inv.last_terms['mse'].clone()))
    assert all(torch.equal(a, b) for a, b in zip(*out))
    assert (out[0][1][-1] < out[0][1][0]).all()


# ------------------------------------------------------------------------------------------------------- model level
def _ood_model(dev, size=256):
    from oodgan.arch import ood_faceGAN_e4e
    m = ood_faceGAN_e4e(out_size=size, style_dim=512, encoder='E4E', enable_modulation=True, warp_scale=0.08, cycle_align=2, blend_with_gen=True,
                        ModSize=256, build_encoder=False)
    res = m.load_state_dict(synth.ood_state(size, seed=41), strict=False)
    assert not res.missing_keys and not res.unexpected_keys, res
    return m.to(dev).eval()


def test_model_invert_takes_lpips_size(dev):
    from oodgan import _lib
    size, B = 256, 2
    m = _ood_model(dev, size)
    x = synth.make_images(size, B, seed=44).to(dev)
    kw = dict(enc_lats=synth.make_latents(size, B, seed=42, std=0.3).to(dev), enc_feats=[f.to(dev) for f in synth.make_encoder_feats(B, seed=43)],
              noise=[n.to(dev) for n in synth.make_noises(size, B, seed=45)])
    _lib.dispatch_reset()
    for bad in (96, 100, 32, 8, 512, True, 64.0, '64'):
        with pytest.raises(ValueError, match='lpips_size'):
            m.invert(x, steps=4, lpips_weight=0.8, lpips_size=bad, **kw)
    assert all(_lib.dispatch_count(name) == 0 for name in ('area_pool', 's1big', 's1v2', 'tiny', 'stripx', 'strip'))       # nothing was launched
    out, lats, losses = m.invert(x, steps=4, lpips_weight=0.8, lpips_size=64, **kw)
    lp = m.last_loss_terms['lpips']
    assert lp is not None and lp.shape == (4, B) and torch.isfinite(lp).all() and (lp > 0).all()
    assert torch.isfinite(losses).all() and torch.isfinite(out).all()
    assert _lib.dispatch_count('area_pool') >= 1 + 2
    _, _, losses_full = m.invert(x, steps=4, lpips_weight=0.8, **kw)
    assert not torch.equal(m.last_loss_terms['lpips'], lp)           # another function of the image than the full-resolution term
