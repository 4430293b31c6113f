"""The fitted out-of-domain mask of the W+ loop: ``invert(loss_region='fit')`` fits, beside the latents, the logits of a
low-resolution mask under the reference's mask objective and weights the loss with its bilinear enlargement.

The three entries of csrc/loss_maskfit.hip against the float64 yardstick (tests/mask_fit_ref.py) and bit for bit against themselves; dL/dW+
and dL/dl of the running loop — read back from Adam's first moments as tests/wplus_grads.py does — against float64 autograd through the
oracle; the loop against the reference's own autograd + torch.optim.Adam with its MaskLoss (tests/golden/wplus_maskfit_64.npz); where the mask
goes; the run forms (launch plan, Python-driven, rollback, two streams); the model-level outputs and refusals; and the 'full' and 'blend'
regions against the commit before (tests/golden/wplus_maskfit_parent.npz)."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import ref_cpu as R  # noqa: E402
from oodgan import synth  # noqa: E402
from oodgan.ops import lr_multiplier  # noqa: E402
import mask_fit_ref as MR  # noqa: E402
import mask_fit_parent_cases as PC  # noqa: E402
import ssim_ref  # noqa: E402
from sspace_ref import SLOPE_BAND, given_slopes  # noqa: E402
import wplus_grads as WG  # noqa: E402

AREA, WA, WB = MR.DEFAULTS['area'], MR.DEFAULTS['area_weight'], MR.DEFAULTS['binary_weight']
# (S, m): F = 2, 4, 16 (edge cells dominate at m = 4), and 16 at 256² (four blocks of pixel columns per row group)
SHAPES = [(64, 32), (64, 16), (64, 4), (256, 16)]


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


def _i32(v, dev):
    return torch.tensor([v], dtype=torch.int32, device=dev)


def _logits(B, m, want_mean=None, seed=0):
    """Logits (B,1,m,m), float32: N(0, 1.5^2) with +-20 at the first two cells and the last one (a corner cell) — a on both sides of 1/2.
    ``want_mean``: every image shifted (bisection in float64) so that mean(1 - sigmoid(l)) of its float32 logits is that value within 1e-4."""
    l = synth.normal(f'mf.l{m}', (B, 1, m, m), 70 + seed, 1.5)
    l.view(B, -1)[:, 0], l.view(B, -1)[:, 1], l.view(B, -1)[:, -1] = 20.0, -20.0, 20.0
    if want_mean is not None:
        for b in range(B):
            lo, hi = -30.0, 30.0
            for _ in range(60):
                mid = 0.5 * (lo + hi)
                if (1 - torch.sigmoid((l[b] + mid).double())).mean().item() > want_mean:
                    lo = mid
                else:
                    hi = mid
            l[b] += 0.5 * (lo + hi)
            assert abs((1 - torch.sigmoid(l[b].double())).mean().item() - want_mean) < 1e-4
    return l.contiguous()


def _share(got, want):
    """max |got - want| as a share of max |want|, in float64 on the CPU."""
    want = want.detach().double().cpu()
    return (got.detach().double().cpu() - want).abs().max().item() / want.abs().max().item()


# ------------------------------------------------------------------------------------------------------------- expand
@pytest.mark.parametrize('B', [1, 3])
@pytest.mark.parametrize('S,m', SHAPES)
def test_expand_vs_float64(dev, S, m, B):
    """a = sigmoid(l) and beta = U(a) against float64 torch (F.interpolate, bilinear, align_corners=False), logits +-20 included: both within
    1e-6 absolute — values in [0, 1]; the bar the composite kernels are held to in tests/test_hip_wplus_masked.py.  Buffers handed in are
    written in place; shapes the kernels are not built for are refused."""
    from oodgan import ops
    l = _logits(B, m)
    a, beta = ops.maskfit_expand(l.to(dev), S)
    a64 = torch.sigmoid(l.double())
    b64 = MR.upsample(a64, S)
    e_a, e_b = (a.double().cpu() - a64).abs().max().item(), (beta.double().cpu() - b64).abs().max().item()
    print(f'expand S {S} m {m} B {B}: |a - float64| {e_a:.2e}, |beta - float64| {e_b:.2e} (bars 1e-6)')
    assert a.shape == (B, 1, m, m) and beta.shape == (B, 1, S, S)
    assert e_a <= 1e-6 and e_b <= 1e-6
    assert a.view(B, -1)[:, 0].min() > 1 - 1e-6 and a.view(B, -1)[:, 1].max() < 1e-6
    a2, b2 = torch.full_like(a, -7.0), torch.full_like(beta, -7.0)
    ra, rb = ops.maskfit_expand(l.to(dev), S, a=a2, beta=b2)
    assert ra is a2 and rb is b2 and torch.equal(a2, a) and torch.equal(b2, beta)
    if B == 1:
        with pytest.raises(RuntimeError, match='maskfit_expand'):
            ops.maskfit_expand(l.to(dev), m)                                        # F = 1
        with pytest.raises(RuntimeError, match='maskfit_expand'):
            ops.maskfit_expand(torch.zeros(1, 1, 3, 3, device=dev), 48)             # no powers of two


# ------------------------------------------------------------------------------------------------------------- chain + step
CASES = {'open': (AREA + 0.05, WA, WB), 'shut': (AREA - 0.05, WA, WB), 'no_area': (AREA + 0.05, 0.0, WB), 'no_binary': (AREA + 0.05, WA, 0.0)}


def _device_step(ops, dev, l, gen, x, t0, total, up, down, lr, wa, wb, state=None, tables=None):
    """One mask-side step on the device from logits ``l`` (a device tensor, updated in place): expand, the composite pixel term w.r.t. c,
    chain, step.  Returns (gimg, e, g written back, a, beta, gmul)."""
    B, _, S, _ = gen.shape
    gmul = ops.loss_scale_for(3 * S * S)
    a, beta = ops.maskfit_expand(l, S)
    _, gimg, c = ops.pixel_loss_grad(gen, x, 'mse', None, beta, gmul, wrt='composite', composite=False)
    assert c is None
    gimg, e = ops.maskfit_chain(gimg, gen, x, beta)
    if state is None:
        state = (torch.zeros_like(l), torch.zeros_like(l))
    g = torch.full_like(l, -7.0)
    ta, tb = tables if tables is not None else (None, None)
    ops.maskfit_step(l, g, state[0], state[1], a, e, _i32(t0, dev), total, up, down, lr, grad_div=gmul, area=AREA, area_weight=wa,
                     binary_weight=wb, area_table=ta, binary_table=tb)
    return gimg, e, g, a, beta, gmul


@pytest.mark.parametrize('case', list(CASES))
@pytest.mark.parametrize('B', [1, 3])
@pytest.mark.parametrize('S,m', SHAPES)
def test_chain_and_step_vs_float64_autograd(dev, S, m, B, case):
    """beta (.) dL/dc, e = dL/dbeta, dL/dl and the two table rows against float64 autograd of the whole L_b (tests/mask_fit_ref.objective):
    gradients as a share of their maximum, table rows absolute, bars 1e-6.  The hinge open and shut (mean(1 - a) - A = +-0.05 by a shift of
    the logits, away from the tie), a on both sides of 1/2, logits +-20, either weight zero."""
    from oodgan import ops
    mean, wa, wb = CASES[case]
    l0 = _logits(B, m, want_mean=mean, seed=1)
    gen, x = synth.normal(f'mf.g{S}', (B, 3, S, S), 71), synth.make_images(S, B, seed=72)
    ld = l0.clone().to(dev)
    ta, tb = torch.full((3, B), -1.0, device=dev), torch.full((3, B), -1.0, device=dev)
    gimg, e, g, a, beta, gmul = _device_step(ops, dev, ld, gen.to(dev), x.to(dev), 1, 8, 0.0, 0.0, 0.1, wa, wb, tables=(ta, tb))
    l64, g64 = l0.double().requires_grad_(True), gen.double().requires_grad_(True)
    tot, pix, hinge, binary, b64 = MR.objective(l64, g64, x.double(), AREA, wa, wb)
    b64.retain_grad()
    tot.sum().backward()
    assert ((hinge > 0).all() if case != 'shut' else (hinge == 0).all()) and (torch.sigmoid(l0) > 0.5).any() and (torch.sigmoid(l0) < 0.5).any()
    e_g, e_e, e_l = _share(gimg / gmul, g64.grad), _share(e / gmul, b64.grad), _share(g, l64.grad)
    e_h = (ta[1].double().cpu() - hinge.detach()).abs().max().item()
    e_b = (tb[1].double().cpu() - binary.detach()).abs().max().item()
    print(f'chain + step S {S} m {m} B {B} {case}: beta*dL/dc {e_g:.2e}, e {e_e:.2e}, dL/dl {e_l:.2e} of max; hinge row {e_h:.2e}, binary row {e_b:.2e} '
          f'(bars 1e-6); max |dL/dl| {l64.grad.abs().max().item():.3e}')
    assert e_g <= 1e-6 and e_e <= 1e-6 and e_l <= 1e-6 and e_h <= 1e-6 and e_b <= 1e-6
    assert not torch.equal(ld.cpu(), l0)                        # Adam moved the logits


@pytest.mark.parametrize('S,m,B', [(64, 16, 3), (256, 16, 1), (64, 4, 2)])
def test_mask_adam_vs_float64(dev, S, m, B):
    """Five consecutive steps of Adam on l from counter value 2 with the ramps on (0.5 / 0.5 of 8: factors 0.5, 0.75, 1, 0.854, 0.5) on frozen G and x,
    the device recomputing expand, pixel term, chain and step each time, against float64 autograd + ``adam_step`` (torch.optim.Adam written
    out): l within 1e-6 * max(1, max |l|) after every step.  The call leaves the counter alone."""
    from oodgan import ops
    total, up, down, lr, t0 = 8, 0.5, 0.5, 0.1, 2
    l0 = _logits(B, m, want_mean=AREA + 0.05, seed=2)
    gen, x = synth.normal(f'mf.g{S}', (B, 3, S, S), 73), synth.make_images(S, B, seed=74)
    gd, xd, ld = gen.to(dev), x.to(dev), l0.clone().to(dev)
    state = (torch.zeros_like(ld), torch.zeros_like(ld))
    l64, m64, v64 = l0.double(), torch.zeros_like(l0, dtype=torch.float64), torch.zeros_like(l0, dtype=torch.float64)
    for i in range(t0, t0 + 5):
        leaf = l64.clone().requires_grad_(True)
        MR.objective(leaf, gen.double(), x.double(), AREA, WA, WB)[0].sum().backward()
        l64, m64, v64 = MR.adam_step(l64, leaf.grad, m64, v64, i + 1, lr * lr_multiplier(i, total, up, down))
        t = _i32(i, dev)
        _device_step(ops, dev, ld, gd, xd, i, total, up, down, lr, WA, WB, state=state)
        err = (ld.double().cpu() - l64).abs().max().item() / max(1.0, l64.abs().max().item())
        print(f'mask Adam S {S} m {m} B {B} step {i + 1}: l err {err:.2e} (bar 1e-6); lr factor {lr_multiplier(i, total, up, down):.3f}')
        assert err <= 1e-6
    assert (ld.cpu() - l0).abs().max() > 0.05


def test_table_form_writes_the_clamped_row_only(dev):
    from oodgan import ops
    S, m, B = 64, 16, 2
    l0 = _logits(B, m, want_mean=AREA + 0.05, seed=3)
    gen, x = synth.normal('mf.g64', (B, 3, S, S), 75).to(dev), synth.make_images(S, B, seed=76).to(dev)
    for t0, row in ((0, 0), (1, 1), (2, 2), (7, 2)):
        ta, tb = torch.full((3, B), -7.0, device=dev), torch.full((3, B), -7.0, device=dev)
        ld = l0.clone().to(dev)
        t = _i32(t0, dev)
        a, beta = ops.maskfit_expand(ld, S)
        e = torch.zeros(B, 1, S, S, device=dev)
        st = (torch.zeros_like(ld), torch.zeros_like(ld), torch.zeros_like(ld))
        ops.maskfit_step(ld, st[0], st[1], st[2], a, e, t, 8, area_table=ta, binary_table=tb)
        assert int(t.item()) == t0                                  # read, not incremented
        for tab in (ta, tb):
            assert (tab[row] >= 0).all() and (tab[[r for r in range(3) if r != row]] == -7.0).all(), (t0, tab)
        assert abs(ta[row, 0].item() - 0.05) < 2e-4
    # one table, or none
    ops.maskfit_step(l0.clone().to(dev), st[0], st[1], st[2], a, e, _i32(0, dev), 8, binary_table=tb)
    ops.maskfit_step(l0.clone().to(dev), st[0], st[1], st[2], a, e, _i32(0, dev), 8)


def test_two_runs_give_identical_bits(dev):
    from oodgan import ops
    for S, m, B in ((64, 4, 3), (256, 16, 2)):
        l0 = _logits(B, m, want_mean=AREA + 0.05, seed=4)
        gen, x = synth.normal(f'mf.g{S}', (B, 3, S, S), 77).to(dev), synth.make_images(S, B, seed=78).to(dev)
        outs = []
        for _ in range(2):
            ld = l0.clone().to(dev)
            ta, tb = torch.zeros(3, B, device=dev), torch.zeros(3, B, device=dev)
            gimg, e, g, a, beta, _ = _device_step(ops, dev, ld, gen, x, 1, 8, 0.05, 0.25, 0.1, WA, WB, tables=(ta, tb))
            outs.append((ld, gimg, e, g, a, beta, ta, tb))
        assert all(torch.equal(p, q) for p, q in zip(*outs)), (S, m, B)


# ------------------------------------------------------------------------------------------------------------- gradients in the running loop
_STATE = {}


def _state(size, seed=0):
    if (size, seed) not in _STATE:
        P = synth.generator_state(size, seed=seed)
        _STATE.clear()
        _STATE[(size, seed)] = (P, {k: v.double() for k, v in P.items()})
    return _STATE[(size, seed)]


GRAD_BAR_W = {'f16s': 1e-4, 'f16s-g2': 3e-4}          # the project's bars for dL/dW+
GRAD_BAR_L = 1e-4                                      # dL/dl depends on the forward image only, fp32-class in both precisions
GRAD_CASES = {'b2-f16s': (2, 'f16s', 0.0), 'b2-f16s-g2': (2, 'f16s-g2', 0.0), 'b1-ssim': (1, 'f16s', 0.5)}
# Points whose dL/dW+ is not held to the bar against the PLAIN float64 oracle, by name, as tests/test_hip_fspace.py names its LeakyReLU kinks
# (the same image of the same recipe is named there): (case, image) -> the measured reason.  They stay held to it against the float64 oracle
# that takes, for the pre-activations float32 cannot tell from 0 (within 2^-20 of their layer's maximum), the side the kernels took.
KINK_POINTS = {
    ('b2-f16s', 1): 'dL/dW+ 4.26e-4 against the plain oracle at step 1 (the same figure in both precisions: not a rounding of the gradient path)',
    ('b2-f16s-g2', 1): 'dL/dW+ 4.24e-4 against the plain oracle at step 1',
}
ADOPTED_MAX = lambda n_elements: 4 * SLOPE_BAND * n_elements + 8          # as tests/test_hip_fspace.py


@pytest.mark.parametrize('case', list(GRAD_CASES))
def test_step_gradients_vs_float64(dev, case):
    """256², m = 64, one step of the loop from random logits: dL/dW+ and dL/dl — recovered from the first moments of the latents' and the
    logits' Adam through ``on_step`` — against float64 autograd of the whole objective through ``oracle.ref_cpu.generator_forward``, per image as
    a share of the gradient's maximum.  dL/dW+ is held to the project's bars (1e-4 for f16s, 3e-4 for f16s-g2), dL/dl to 1e-4 for both.  The
    B = 1 case adds ssim_weight = 0.5: the chain then sums dL/dc of two terms.

    Every image is compared twice, as the step-1 points of tests/test_hip_sspace.py and tests/test_hip_fspace.py are: with the plain oracle, and
    with the oracle taking the LeakyReLU side of the pre-activations within 2^-20 of their layer's maximum from the loop's own forward
    (``sspace_ref.given_slopes``: no slope outside the band may differ, the number taken stays within ``ADOPTED_MAX``).  The bars hold against
    the second for every image and against the first for every image not named in ``KINK_POINTS``; dL/dl is held to its bar against both."""
    from oodgan.engine import GeneratorEngine, WPlusInverter
    size, m = 256, 64
    B, prec, ssw = GRAD_CASES[case]
    P, P64 = _state(size, 0)
    target, w0, noises = WG.recipe(size, list(range(B)))
    l0 = (synth.normal('mf.grad.l', (B, 1, m, m), 79, 1.0) + 1.5).contiguous()
    eng = GeneratorEngine({k: v.to(dev) for k, v in P.items()}, size, precision=prec)
    inv = WPlusInverter(eng, mask_size=m, ssim_weight=ssw)
    cap, slopes_of = {}, []
    styled = ['conv1'] + [f'convs.{j}' for j in range(2 * (eng.log_size - 2))]

    def on_step(run):
        cap[run.t] = (run.m.clone(), run.mm.clone(), run.mg.clone())
        # the side of zero every pre-activation of the loop's own forward lies on, per styled conv: the sign of its saved output
        acts = [run.eng.saved['acts'][nm] for nm in styled]
        slopes_of[:] = [((a.to_nchw() if hasattr(a, 'to_nchw') else a) > 0).cpu() for a in acts]
    inv.on_step = on_step
    w, losses = inv.invert(target.to(dev), w0.to(dev), [n.to(dev) for n in noises], steps=1, mask_logits=l0.to(dev))
    torch.cuda.synchronize()
    assert inv.last_stats == {'steps_run': [1], 'rollbacks': [0]}
    fails = []
    for k in range(B):
        gw = WG.recover_grad(torch.zeros_like(w0[k]), cap[1][0][k].cpu(), inv.betas[0])
        gl = WG.recover_grad(torch.zeros_like(l0[k]), cap[1][1][k].cpu(), inv.betas[0])
        extra = (lambda c, x: ssw * ssim_ref.ssim_loss(c, x)) if ssw else None

        def oracle():
            wl = w0[k:k + 1].double().clone().requires_grad_(True)
            ll = l0[k:k + 1].double().clone().requires_grad_(True)
            img = R.generator_forward(P64, wl, [n[k:k + 1].double() for n in noises], size)
            tot = MR.objective(ll, img, target[k:k + 1].double(), AREA, WA, WB, extra)[0]
            tot.sum().backward()
            return tot.item(), wl.grad[0], ll.grad[0]
        tot, gw64, gl64 = oracle()
        with given_slopes([s_[k:k + 1] for s_ in slopes_of]) as gs_:
            _, gw64s, gl64s = oracle()
        n_el, taken, outside = sum(s_[k:k + 1].numel() for s_ in slopes_of), sum(gs_.adopted), sum(gs_.outside)
        e_w, e_l, e_g = _share(gw, gw64), _share(gl, gl64), _share(cap[1][2][k], gl64)
        es_w, es_l = _share(gw, gw64s), _share(gl, gl64s)
        e_loss = abs(losses[0, k].item() - tot) / tot
        kept = (case, k) not in KINK_POINTS
        print(f'[{case}] image {k}: dL/dW+ {e_w:.2e} of max (bar {GRAD_BAR_W[prec]:.0e}), dL/dl {e_l:.2e} recovered, {e_g:.2e} as written back (bar '
              f'{GRAD_BAR_L:.0e}), total loss rel {e_loss:.2e}; max |dL/dl| {gl64.abs().max().item():.3e}' + ('' if kept else '  [named in KINK_POINTS]'))
        print(f'[{case}] image {k}, slopes within 2^-20 of the layer maximum as the engine took them: dL/dW+ {es_w:.2e}, dL/dl {es_l:.2e}; {taken} of '
              f'{n_el} slopes taken (at most {ADOPTED_MAX(n_el):.0f}), {outside} differ outside the band')
        if outside != 0 or not taken <= ADOPTED_MAX(n_el):
            fails.append(f'image {k}: {outside} slopes differ outside the band, {taken} taken')
        if not es_w <= GRAD_BAR_W[prec] or (kept and not e_w <= GRAD_BAR_W[prec]):
            fails.append(f'image {k}: dL/dW+ {e_w:.2e} plain, {es_w:.2e} given slopes')
        if not (e_l <= GRAD_BAR_L and e_g <= GRAD_BAR_L and es_l <= GRAD_BAR_L):
            fails.append(f'image {k}: dL/dl {e_l:.2e} / {e_g:.2e} / {es_l:.2e}')
        if not e_loss <= 1e-5:
            fails.append(f'image {k}: loss {e_loss:.2e}')
    assert not fails, f'[{case}] ' + '; '.join(fails)


# ------------------------------------------------------------------------------------------------------------- the loop against the reference
def _fixture_run(g, dev, **ctor):
    """(engine, inverter, x, w0, noises, start logits, steps, m) of tests/golden/make_wplus_maskfit.py's case."""
    from oodgan.engine import GeneratorEngine, WPlusInverter, mask_logits
    size, m, B, steps = (int(v) for v in g['meta'])
    sw, sn, s_w, s_start = (int(v) for v in g['seeds'])
    area, wa, wb, lr, mlr, init = (float(v) for v in g['settings'])
    eng = GeneratorEngine({k: v.to(dev) for k, v in synth.generator_state(size, seed=sw).items()}, size)
    w_star = synth.make_latents(size, B, seed=s_w, std=0.3)
    w0 = (w_star + 0.1 * synth.normal('maskfit.start', tuple(w_star.shape), s_start)).to(dev)
    noises = [n.to(dev) for n in synth.make_noises(size, B, seed=sn)]
    inv = WPlusInverter(eng, lr=lr, mask_size=m, mask_lr=mlr, mask_area=area, mask_area_weight=wa, mask_binary_weight=wb, **ctor)
    ml0 = mask_logits(torch.full((B, 1, m, m), init, device=dev))
    return eng, inv, g['target'].to(dev), w0, noises, ml0, steps, m


@pytest.fixture(scope='module')
def fixture_result(dev, golden):
    """The fixture's case run once through the default loop (launch plan), shared by the tests below; left unchanged."""
    g = golden('wplus_maskfit_64.npz')
    eng, inv, x, w0, noises, ml0, steps, m = _fixture_run(g, dev)
    w, losses = inv.invert(x, w0, noises, steps=steps, mask_logits=ml0)
    torch.cuda.synchronize()
    return dict(g=g, w=w, losses=losses, terms=dict(inv.last_terms), a=inv.last_fitted_mask, beta=inv.last_loss_weight, l=inv.last_mask_logits,
                stats=inv.last_stats, plan=inv.last_plan, steps=steps)


def test_loop_vs_reference(fixture_result):
    """30 steps at 64², m = 16, against the reference's float64 loop (its Generator, its MaskLoss, torch.optim.Adam with two groups).  Every
    statistic of the loss curve — total, pixel term, lambda_a * hinge, lambda_b * binarisation mean — within max(1e-3, 3 x the fixture's own
    fp32-vs-float64 distance on that statistic), relative (1e-3: the project's bar for loss curves; the factor 3 covers Adam's sign choice for
    ~0 coordinates, as in the robust-loss tests); the fixture's distances are 4.0e-5 (total), 6.9e-5 (pixel), 0 (area: the run stays under its
    budget, both precisions) and 3.3e-6 (binary), so the floor 1e-3 decides.  a_T: max |a_T - a_T^f64| within 3 x the fixture's own distance,
    no floor: the fixture measures 3.42e-5, the band is 1.03e-4."""
    r, g = fixture_result, fixture_result['g']
    wa, wb = float(g['settings'][1]), float(g['settings'][2])
    assert r['stats'] == {'steps_run': [r['steps']], 'rollbacks': [0]} and r['plan']['steps'] == [r['steps'] - 3]
    t = r['terms']
    mine = dict(total=r['losses'], pixel=t['pixel'], ml_area=wa * t['mask_area'], ml_binary=wb * t['mask_binary'])
    assert torch.equal(r['losses'], t['pixel'] + wa * t['mask_area'] + wb * t['mask_binary'])
    fails = []
    for k, v in mine.items():
        f64, f32 = g[f'{k}_f64'].double(), g[f'{k}_f32'].double()
        rel = lambda p, q: ((p - q).abs() / q.abs().clamp_min(1e-30)).max().item()
        own = rel(f32, f64)
        bar = max(1e-3, 3 * own)
        err = rel(v.double().cpu(), f64)
        print(f'loop vs reference, {k}: rel {err:.2e} (bar {bar:.2e}; the fixture fp32 vs float64 {own:.2e}); {v[0].tolist()} -> {v[-1].tolist()}')
        if not err <= bar:
            fails.append(f'{k}: {err:.2e} > {bar:.2e}')
    own_a = (g['a_T_f32'] - g['a_T_f64']).abs().max().item()
    err_a = (r['a'].double().cpu() - g['a_T_f64']).abs().max().item()
    err_w = (r['w'].double().cpu() - g['w_T_f64']).abs().max().item()
    print(f'loop vs reference, a_T: max |a_T - float64| {err_a:.2e} (band {3 * own_a:.2e} = 3 x the fixture fp32 vs float64 {own_a:.2e}); '
          f'w_T max diff {err_w:.2e} (the fixture {(g["w_T_f32"].double() - g["w_T_f64"]).abs().max().item():.2e})')
    if not err_a <= 3 * own_a:
        fails.append(f'a_T: {err_a:.2e} > {3 * own_a:.2e}')
    assert not fails, '; '.join(fails)


def test_the_mask_goes_where_the_occluder_is(fixture_result):
    """On the fixture's occluder (rows 4-23, columns 20-43 at the image's maximum) mean(beta_T) outside the rectangle minus inside is at least
    half the float64 fixture's own gap per image, and the mask keeps its budget: mean(1 - a_T) <= A + 0.05."""
    r, g = fixture_result, fixture_result['g']
    r0, r1, c0, c1 = (int(v) for v in g['rect'])
    beta = r['beta'][:, 0].double().cpu()
    inside = torch.zeros(beta.shape[-2:], dtype=torch.bool)
    inside[r0:r1, c0:c1] = True
    assert (r['beta'].cpu() - MR.upsample(r['a'].cpu(), beta.shape[-1])).abs().max() <= 1e-6        # last_loss_weight is U(last_fitted_mask)
    for b in range(beta.shape[0]):
        gap, want = (beta[b][~inside].mean() - beta[b][inside].mean()).item(), (g['beta_out_f64'][b] - g['beta_in_f64'][b]).item()
        spent = (1 - r['a'][b]).mean().item()
        print(f'image {b}: beta outside - inside {gap:.3f} (the float64 fixture {want:.3f}); mean(1 - a_T) {spent:.3f} (budget {float(g["settings"][0]):.2f})')
        assert want > 0.2 and gap >= 0.5 * want
        assert spent <= float(g['settings'][0]) + 0.05


# ------------------------------------------------------------------------------------------------------------- run forms
def test_plan_and_python_loop_agree_bit_for_bit(dev, fixture_result):
    r = fixture_result
    eng, inv, x, w0, noises, ml0, steps, m = _fixture_run(r['g'], dev, use_plan=False)
    w, losses = inv.invert(x, w0, noises, steps=steps, mask_logits=ml0)
    assert inv.last_plan['steps'] == [0] and r['plan']['steps'] == [steps - 3] and r['plan']['launches'][0] > 0
    assert torch.equal(losses, r['losses']) and torch.equal(w, r['w']) and torch.equal(inv.last_mask_logits, r['l'])
    assert torch.equal(inv.last_terms['mask_area'], r['terms']['mask_area']) and torch.equal(inv.last_terms['mask_binary'], r['terms']['mask_binary'])
    assert torch.equal(inv.last_fitted_mask, r['a']) and torch.equal(inv.last_loss_weight, r['beta'])


@pytest.mark.parametrize('use_plan', [True, False])
def test_rollback_restores_the_logits_and_their_moments(dev, fixture_result, use_plan):
    """The noise maps scaled by 2^30 for one step (after step 15 of 30, as tests/test_hip_generator.py provokes the forward flag): the carried
    scales are off, the guard flags the window, and the run goes back to its last clean snapshot — (l, its m, its v) with (w, m, v) — repeats
    the window with exact scales and ends where the undisturbed run ends: losses within 1e-3 relative (the bar of the other rollback tests),
    the logits within 1e-3.  Logits or moments left at what the scaled step made of them would not come back."""
    r = fixture_result
    eng, inv, x, w0, noises, ml0, steps, m = _fixture_run(r['g'], dev, use_plan=use_plan)
    seen = []

    def scale(run):
        if run.steps_run == 15 and not seen:
            seen.append(1)
            for n in run.noises:
                n.mul_(2.0 ** 30)
        elif run.steps_run == 16 and len(seen) == 1:
            seen.append(2)
            for n in run.noises:
                n.mul_(2.0 ** -30)
    inv.on_step = scale
    w, losses = inv.invert(x, w0, noises, steps=steps, mask_logits=ml0)
    inv.on_step = None
    rel = ((losses - r['losses']).abs() / r['losses']).max().item()
    dl = (inv.last_mask_logits - r['l']).abs().max().item()
    print(f'noise maps x 2^30 for step 16 of {steps} (plans {use_plan}): {inv.last_stats}; loss rel diff {rel:.2e} (bar 1e-3), |l - undisturbed| {dl:.2e} '
          f'(bar 1e-3), |w - undisturbed| {(w - r["w"]).abs().max().item():.2e}')
    assert seen == [1, 2] and inv.last_stats['rollbacks'] == [1] and inv.last_stats['steps_run'][0] == steps + inv.check_every + inv.check_lag
    assert torch.isfinite(losses).all() and torch.isfinite(inv.last_mask_logits).all() and torch.isfinite(w).all()
    assert torch.equal(losses[:inv.check_every], r['losses'][:inv.check_every])
    assert rel < 1e-3 and dl < 1e-3


def test_two_streams_stay_within_half_a_percent(dev, fixture_result):
    r = fixture_result
    eng, inv, x, w0, noises, ml0, steps, m = _fixture_run(r['g'], dev)
    w, losses = inv.invert(x, w0, noises, steps=steps, streams=2, mask_logits=ml0)
    rel = ((losses - r['losses']).abs() / r['losses']).max().item()
    print(f'two streams vs one: loss rel diff {rel:.2e} (bar 5e-3); plan {inv.last_plan}')
    assert rel <= 5e-3 and inv.last_plan['steps'] == [steps - 3] * 2 and inv.last_stats['rollbacks'] == [0, 0]
    assert inv.last_fitted_mask.shape == r['a'].shape and inv.last_loss_weight.shape == r['beta'].shape
    assert inv.last_terms['mask_area'].shape == (steps, 2) and (inv.last_fitted_mask - r['a']).abs().max() < 1e-2


def test_composition(dev, fixture_result):
    """The fitted mask beside the other options of the loop: latent_space 'w', layer_lr, delta_reg, the schedule, a robust pixel term, SSIM and
    LPIPS on a pooled view — every run finite, without a rollback, with a mask that moved."""
    from oodgan.engine import GeneratorEngine, WPlusInverter
    from oodgan.lpips import LPIPSAlex
    r = fixture_result
    lp = LPIPSAlex({k: v.to(dev) for k, v in synth.lpips_state(0).items()}, min_max=(-1.0, 1.0))
    for ctor in (dict(latent_space='w'), dict(layer_lr=[1.0] * 5 + [0.5] * 5, delta_reg=0.1),
                 dict(lr_rampup=0.05, lr_rampdown=0.25, latent_noise=0.05), dict(pixel_loss='charbonnier', ssim_weight=0.3),
                 dict(lpips=lp, lpips_weight=0.8)):
        eng, inv, x, w0, noises, ml0, steps, m = _fixture_run(r['g'], dev, **ctor)
        w, losses = inv.invert(x, w0, noises, steps=6, mask_logits=ml0)
        print(f'{sorted(ctor)}: loss {losses[0].tolist()} -> {losses[-1].tolist()}, plan {inv.last_plan}')
        assert inv.last_stats == {'steps_run': [6], 'rollbacks': [0]} and inv.last_plan['steps'] == [3]
        assert torch.isfinite(losses).all() and torch.isfinite(w).all() and (inv.last_mask_logits != ml0).any()


# ------------------------------------------------------------------------------------------------------------- model level
def _model_64(dev):
    import test_hip_wplus_sched as S
    return S._model_64(dev)


def _kw64(dev, B):
    return dict(enc_lats=synth.make_latents(64, B, seed=42, std=0.3).to(dev), noise=[n.to(dev) for n in synth.make_noises(64, B, seed=45)])


def test_model_outputs_without_modulation_at_64(dev):
    """``enable_modulation=False``: fit_blend=True returns exactly blend(x, G(last_refined_lats), 1 - last_loss_weight); fit_blend=False the bits
    of the model's own forward at the refined latents; the options reach the loop; the attributes are set and cleared."""
    size, B, steps, m = 64, 2, 6, 16
    md = _model_64(dev)
    x, kw = synth.make_images(size, B, seed=44).to(dev), _kw64(dev, B)
    out, lats, losses = md.invert(x, steps=steps, loss_region='fit', mask_size=m, fit_blend=True, **kw)
    a, beta, t = md.last_fitted_mask, md.last_loss_weight, md.last_loss_terms
    assert a.shape == (B, 1, m, m) and beta.shape == (B, 1, size, size) and torch.equal(lats, md.last_refined_lats)
    assert t['mask_area'].shape == (steps, B) and t['mask_binary'].shape == (steps, B)
    assert torch.equal(losses, t['pixel'] + 5.0 * t['mask_area'] + 0.2 * t['mask_binary'])
    assert abs(t['mask_binary'][0, 0].item() - 0.12) < 1e-6 and t['mask_area'][0].abs().max() == 0         # the start: a = 0.88 everywhere
    gen, _ = md.generator(md.last_refined_lats, input_is_tensor=True, input_is_latent=True, noise=kw['noise'])
    assert torch.equal(out, md.blend(x, gen, alpha_scale=1 - beta))
    out2, lats2, losses2 = md.invert(x, steps=steps, loss_region='fit', mask_size=m, **kw)
    assert torch.equal(losses2, losses) and torch.equal(lats2, lats) and torch.equal(md.last_fitted_mask, a)
    assert torch.equal(out2, md(x, lats=lats2, **kw)[0]) and not torch.equal(out2, out)
    # a tensor start and other settings reach the loop
    a0 = torch.full((B, 1, m, m), 0.6, device=dev)
    a0[:, :, :4] = 0.0
    md.invert(x, steps=2, loss_region='fit', mask_size=m, mask_init=a0, mask_lr=0.05, mask_area=0.1, mask_area_weight=2.0, mask_binary_weight=0.0, **kw)
    t = md.last_loss_terms
    want = (1 - a0.clamp(1e-3, 1 - 1e-3)).mean().item() - 0.1
    assert abs(t['mask_area'][0, 0].item() - want) < 1e-5
    # edit: added after the fit, the blend taken at the edited latents
    e = synth.normal('mf.edit', tuple(lats.shape[1:]), 46, 0.1).to(dev)
    out_e, lats_e, losses_e = md.invert(x, steps=steps, loss_region='fit', mask_size=m, fit_blend=True, edit=e, **kw)
    assert torch.equal(losses_e, losses) and torch.equal(lats_e, (lats + e).contiguous())
    gen_e, _ = md.generator(lats_e, input_is_tensor=True, input_is_latent=True, noise=kw['noise'])
    assert torch.equal(out_e, md.blend(x, gen_e, alpha_scale=1 - md.last_loss_weight))
    # without the option nothing is left behind
    md.invert(x, steps=2, **kw)
    assert md.last_fitted_mask is None and md.last_loss_weight is None and md.last_loss_terms['mask_area'] is None


def test_model_refusals_at_64(dev):
    from oodgan import _lib
    size, B, m = 64, 2, 16
    md = _model_64(dev)
    x, kw = synth.make_images(size, B, seed=44).to(dev), _kw64(dev, B)
    md.generator.engine()
    _lib.dispatch_reset()
    fit = dict(loss_region='fit', mask_size=m)
    for bad, name in ((dict(use_graph=True), 'use_graph'), (dict(pixel_size=32), 'pixel_size'), (dict(pixel_size=32, pixel_filter='bicubic'), 'pixel_'),
                      (dict(pixel_target=torch.zeros(B, 3, 32, 32, device=dev)), 'pixel_'), (dict(latent_space='s'), 'latent_space'),
                      (dict(feature_layer=5), 'feature_layer')):
        with pytest.raises(NotImplementedError, match=name):
            md.invert(x, steps=2, **fit, **bad, **kw)
    for bad, name in ((dict(mask_size=64), 'mask_size'), (dict(mask_size=8), 'mask_size'), (dict(mask_size=24), 'mask_size'),
                      (dict(mask_area_weight=-1.0), 'mask_area_weight'), (dict(mask_binary_weight=float('nan')), 'mask_binary_weight'),
                      (dict(mask_lr=0.0), 'mask_lr'), (dict(mask_lr=float('inf')), 'mask_lr'), (dict(mask_area=1.5), 'mask_area'),
                      (dict(mask_init=1.0), 'mask_init'), (dict(mask_init=0.0), 'mask_init'), (dict(mask_init='blend'), 'mask_init'),
                      (dict(mask_init=torch.full((B, 1, m, m), 0.5)), 'mask_init'),
                      (dict(mask_init=torch.full((B, 1, 8, 8), 0.5, device=dev)), 'mask_init'),
                      (dict(mask_init=torch.full((B, 1, m, m), 0.5, device=dev, dtype=torch.float64)), 'mask_init'),
                      (dict(mask_init=torch.full((B, 1, m, m), 1.5, device=dev)), 'mask_init')):
        with pytest.raises(ValueError, match=name):
            md.invert(x, steps=2, **{**fit, **bad}, **kw)
    with pytest.raises(ValueError, match='fit_blend'):
        md.invert(x, steps=2, fit_blend=True, **kw)
    assert all(_lib.dispatch_count(c) == 0 for c in ('s1big', 's1v2', 'tiny', 'composite_mse'))      # nothing of the loop was launched
    # the padded (narrow) generator, and the inverter's own checks
    from oodgan.engine import GeneratorEngine, WPlusInverter, mask_logits
    P = synth.generator_state(256, seed=5, narrow=0.1875)
    eng = GeneratorEngine({k: v.to(dev) for k, v in P.items()}, 256, narrow=0.1875)
    assert eng.padded
    w = synth.make_latents(256, 1, seed=14).to(dev)
    nz = [n.to(dev) for n in synth.make_noises(256, 1, seed=7)]
    xt = synth.make_images(256, 1, seed=9).to(dev)
    ml = mask_logits(torch.full((1, 1, 64, 64), 0.88, device=dev))
    with pytest.raises(NotImplementedError, match='zero-padded'):
        WPlusInverter(eng, mask_size=64).invert(xt, w, nz, steps=2, mask_logits=ml)
    eng64 = md.generator.engine()
    w64 = kw['enc_lats']
    inv = WPlusInverter(eng64, mask_size=m)
    ml64 = mask_logits(torch.full((B, 1, m, m), 0.88, device=dev))
    with pytest.raises(ValueError, match='mask_logits'):
        inv.invert(x, w64, kw['noise'], steps=2)
    with pytest.raises(ValueError, match='mask_logits'):
        inv.invert(x, w64, kw['noise'], steps=2, mask_logits=ml64[:1])
    with pytest.raises(ValueError, match='loss weight'):
        inv.invert(x, w64, kw['noise'], steps=2, mask_logits=ml64, loss_weight=torch.ones(B, 1, size, size, device=dev))
    with pytest.raises(ValueError, match='mask_logits'):
        WPlusInverter(eng64).invert(x, w64, kw['noise'], steps=2, mask_logits=ml64)
    with pytest.raises(ValueError, match='mask_size'):
        WPlusInverter(eng64, mask_size=64).invert(x, w64, kw['noise'], steps=2, mask_logits=torch.zeros(B, 1, 64, 64, device=dev))


def test_model_with_modulation_at_256(dev):
    """With the SAMM blocks: mask_init='blend' starts from the area-pooled beta of loss_region='blend'; fit_blend=True replaces the SAMM blend by
    the fitted one, exactly; fit_blend=False returns the model's own forward at the refined latents."""
    from oodgan import ops
    m = 64
    md = PC.model(dev)
    x, kw = PC.inputs(dev)
    out, lats, losses = md.invert(x, steps=4, loss_region='fit', mask_size=m, mask_init='blend', fit_blend=True, **kw)
    beta = md.last_loss_weight
    gen, _ = md.generator(lats, input_is_tensor=True, input_is_latent=True, noise=kw['noise'])
    assert torch.equal(out, md.blend(x, gen, alpha_scale=1 - beta)) and torch.isfinite(losses).all()
    md.invert(x, steps=0, loss_region='blend', **kw)
    a0 = ops.area_pool(md.last_loss_weight, 256 // m).clamp(1e-3, 1 - 1e-3)
    md.invert(x, steps=0, loss_region='fit', mask_size=m, mask_init='blend', **kw)
    assert (md.last_fitted_mask - a0).abs().max() <= 1e-6                        # sigmoid(logit(a0))
    out2, lats2, losses2 = md.invert(x, steps=4, loss_region='fit', mask_size=m, mask_init='blend', **kw)
    assert torch.equal(losses2, losses) and torch.equal(lats2, lats)
    assert torch.equal(out2, md(x, lats=lats2, **kw)[0])


# ------------------------------------------------------------------------------------------------------------- the regions of the commit before
@pytest.fixture(scope='module')
def golden_parent(dev):
    md = PC.model(dev)
    x, kw = PC.inputs(dev)
    return dict(model=md, x=x, kw=kw, npz=np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'wplus_maskfit_parent.npz')))


@pytest.mark.parametrize('name', list(PC.CASES))
def test_full_and_blend_keep_the_bits_and_launches_of_the_parent_commit(golden_parent, name):
    """``loss_region='full'`` and ``'blend'`` (alone, and with a second term, where ``scale_by_plane`` runs): equal loss bits, equal SHA-256 of
    the latents and of the output, equal launch count of the recorded step, equal dispatch counters as on the commit before the fitted mask."""
    parent = golden_parent['npz']
    assert tuple(str(c) for c in parent['counter_names']) == PC.COUNTERS
    rec = PC.record(golden_parent['model'], golden_parent['x'], golden_parent['kw'], name)
    bad = []
    for k, v in rec.items():
        want = parent[f'{name}/{k}']
        same = v.shape == want.shape and np.array_equal(v, want)
        print(f'{name} {k}: {"equal" if same else f"{v.tolist()} != parent {want.tolist()}"}')
        if not same:
            bad.append(k)
    assert not bad, bad
