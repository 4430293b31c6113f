"""The similarity alignment of the target beside the latents of the W+ loop: ``WPlusInverter(align='similarity')`` fits, per
image, theta = (log-scale, rotation, tx, ty) and compares G(w) with the target warped by it.

The two entries of csrc/loss_align.hip against the float64 yardstick (tests/align_ref.py), with the same formula in torch-CPU float32 as the
measure of what float32 can deliver (the rule of §20 and §23: per case the kernel's error is at most 4 x the float32 formula's own), and bit for
bit against themselves; theta recovered by the kernels alone; dL/dW+ and dL/dtheta of one step of the running loop against float64 autograd
through the oracle; the loop against the reference's own autograd + torch.optim.Adam on [w, theta] (tests/golden/wplus_align_64.npz); the run
forms (launch plan, Python-driven, two streams, ``align_lr`` 0 against the run without the option); the model-level outputs."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from oracle import ref_cpu as R  # noqa: E402
from oodgan import synth  # noqa: E402
import align_ref as AR  # noqa: E402
import robust_ref  # noqa: E402
from sspace_ref import SLOPE_BAND, given_slopes  # noqa: E402
import wplus_grads as WG  # noqa: E402

SHAPES = [(32, 32), (32, 64), (37, 53), (128, 128)]        # 128²: 16 blocks per image; 37x53: two, the second partly empty
NAN, INF = float('nan'), float('inf')


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


def _thetas(W):
    """name -> the theta of image 0, 1, 2 (float32 values)."""
    base = {'identity': [0.0, 0.0, 0.0, 0.0], 'whole-pixel': [0.0, 0.0, 2.0 / W, 0.0], 'sub-pixel': [0.0, 0.0, 0.7 / W, -0.9 / W],
            'general': [0.1, 0.3, 0.2, -0.1], 'off-image': [-0.2, -0.5, 3.0, 0.4]}
    out = {k: [v, v, v] for k, v in base.items()}
    out['per-image'] = [base['general'], base['sub-pixel'], [-0.05, 0.1, -0.3, 0.25]]
    return out


def _i32(v, dev):
    return torch.tensor([v], dtype=torch.int32, device=dev)


def _grad(gimg, x, th, dev, grad_div=1.0, reg=0.0, **sink):
    """dL/dtheta as ``align_grad_step`` writes it back, with a rate of 0 (theta stays)."""
    from oodgan import ops
    B = x.shape[0]
    g, m, v = (torch.zeros(B, 4, device=dev) for _ in range(3))
    th_d = th.to(dev).clone()
    ops.align_grad_step(gimg, x, th_d, g, m, v, _i32(0, dev), 1, lr=0.0, grad_div=grad_div, align_reg=reg, **sink)
    assert torch.equal(th_d.cpu(), th)
    return g


@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: f'{s[0]}x{s[1]}')
def test_kernels_vs_float64(dev, shape):
    """The warp and dL/dtheta for B in {1, 3} x C in {1, 3} x six thetas: max |kernel - float64| at most 4 x max |float32 formula - float64|
    per case (both zero at the identity and for the warp of a whole-pixel shift, where every weight is exactly 0 or 1); the identity returns
    the source's bits; a second call and the table sink give the same bits."""
    from oodgan import ops
    H, W = shape
    gd = 1024.0
    fails, worst = [], [0.0, 0.0]
    for B in (1, 3):
        for C in (1, 3):
            gen = torch.Generator().manual_seed(1000 * H + 10 * W + 3 * B + C)
            x = torch.randn(B, C, H, W, generator=gen)
            gimg = torch.randn(B, C, H, W, generator=gen) * gd / (C * H * W)
            xd, gimgd = x.to(dev), gimg.to(dev)
            for name, rows in _thetas(W).items():
                th = torch.tensor(rows[:B], dtype=torch.float32)
                y = ops.similarity_warp(xd, th.to(dev))
                y64, y32 = AR.warp(x.double(), th), AR.warp(x, th, torch.float32)
                e_k, e_y = (y.cpu().double() - y64).abs().max().item(), (y32.double() - y64).abs().max().item()
                g = _grad(gimgd, xd, th, dev, gd)
                go = -gimg.double() / gd
                g64, g32 = AR.theta_grad(x.double(), th, go), AR.theta_grad(x, th, go, torch.float32)
                eg_k, eg_y = (g.cpu().double() - g64).abs().max().item(), (g32.double() - g64).abs().max().item()
                print(f'{H}x{W} B={B} C={C} {name}: warp {e_k:.2e} (float32 formula {e_y:.2e}), dL/dtheta {eg_k:.2e} ({eg_y:.2e}; max |g| '
                      f'{g64.abs().max().item():.2e})')
                worst = [max(worst[0], e_k / max(e_y, 1e-300)), max(worst[1], eg_k / max(eg_y, 1e-300))]
                if not e_k <= 4 * e_y:
                    fails.append(f'B={B} C={C} {name}: warp {e_k:.2e} > 4 x {e_y:.2e}')
                if not eg_k <= 4 * eg_y:
                    fails.append(f'B={B} C={C} {name}: dL/dtheta {eg_k:.2e} > 4 x {eg_y:.2e}')
                if name == 'identity' and not torch.equal(y, xd):
                    fails.append(f'B={B} C={C}: the identity does not return the source bit for bit')
                # equal inputs, equal bits; the table row is the plain sink's value
                if not (torch.equal(ops.similarity_warp(xd, th.to(dev)), y) and torch.equal(_grad(gimgd, xd, th, dev, gd), g)):
                    fails.append(f'B={B} C={C} {name}: a second call gives other bits')
                lo, tb = torch.full((B,), -1.0, device=dev), torch.full((3, B), -1.0, device=dev)
                g_lo = _grad(gimgd, xd, th, dev, gd, reg=0.25, loss_out=lo)
                g_tb = _grad(gimgd, xd, th, dev, gd, reg=0.25, table=tb)
                r64 = (th.double() ** 2).sum(1)
                if not (torch.equal(g_lo, g_tb) and torch.equal(tb[0], lo) and (tb[1:] == -1).all()):
                    fails.append(f'B={B} C={C} {name}: the table sink differs from the plain one')
                if not ((lo.cpu().double() - r64).abs() <= 1e-6 * r64.clamp_min(1e-30)).all():
                    fails.append(f'B={B} C={C} {name}: sum theta^2 {lo.tolist()} vs {r64.tolist()}')
                if not ((g_lo.cpu().double() - (g64 + 0.5 * th.double())).abs().max().item() <= 4 * eg_y + 1e-7 * th.abs().max().item()):
                    fails.append(f'B={B} C={C} {name}: the regulariser\'s gradient')
    print(f'{H}x{W}: worst kernel / float32-formula error ratio: warp {worst[0]:.2f}, dL/dtheta {worst[1]:.2f} (bar 4)')
    assert not fails, '; '.join(fails)


@pytest.mark.parametrize('shape', [(32, 32), (37, 53)], ids=lambda s: f'{s[0]}x{s[1]}')
def test_non_finite_theta_keeps_every_index_in_the_image(dev, shape):
    """NaN and inf in any position of theta: every offset is clamped before it becomes an index, so both entries run to their end; values
    are not compared.  A finite image beside them in the batch keeps its bits."""
    from oodgan import ops
    H, W = shape
    gen = torch.Generator().manual_seed(7)
    x = torch.randn(3, 3, H, W, generator=gen).to(dev)
    gimg = torch.randn(3, 3, H, W, generator=gen).to(dev)
    good = [0.1, 0.3, 0.2, -0.1]
    want = ops.similarity_warp(x, torch.tensor([good] * 3, device=dev))
    for bad in ([NAN, 0.0, 0.0, 0.0], [0.0, NAN, 0.0, 0.0], [0.0, 0.0, NAN, NAN], [INF, 0.0, 0.0, 0.0], [-INF, 0.3, 0.0, 0.0], [0.0, INF, 0.0, 0.0],
                [0.0, 0.0, INF, -INF], [80.0, 1.0, 1e30, -1e30], [NAN, INF, -INF, NAN]):
        th = torch.tensor([good, bad, good], dtype=torch.float32)
        y = ops.similarity_warp(x, th.to(dev))
        th_d, (gg, m, v) = th.to(dev), (torch.zeros(3, 4, device=dev) for _ in range(3))
        ops.align_grad_step(gimg, x, th_d, gg, m, v, _i32(0, dev), 1, lr=0.0)
        torch.cuda.synchronize()
        assert torch.equal(y[0], want[0]) and torch.equal(y[2], want[2]) and torch.equal(th_d[[0, 2]].cpu(), th[[0, 2]])


def test_bad_arguments_launch_nothing(dev):
    from oodgan import _lib, ops
    L = _lib.lib()
    x = torch.zeros(1, 1, 8, 8, device=dev)
    th, g, m, v = (torch.zeros(1, 4, device=dev) for _ in range(4))
    part, t = ops.align_grad_parts(1, 8, 8, dev), _i32(0, dev)
    p = ops._p
    n0 = _lib.dispatch_count('align')
    assert L.oodgan_similarity_warp(None, p(th), p(g), 1, 1, 8, 8, None) == -1 and b'similarity_warp' in L.oodgan_last_error()
    for B, C, H, W in ((0, 1, 8, 8), (1, 0, 8, 8), (1, -1, 8, 8), (1, 1, 3, 8), (1, 1, 8, 3)):
        assert L.oodgan_similarity_warp(p(x), p(th), p(g), B, C, H, W, None) == -1
    step = lambda gi=x, B=1, H=8, lr=0.001, reg=0.0, gd=1.0, pt=part: L.oodgan_align_grad_step(  # noqa: E731
        p(gi), p(x), p(th), p(g), p(m), p(v), B, 1, H, 8, lr, 0.9, 0.999, 1e-8, p(t), 10, 0.0, 0.0, gd, reg, None, 0, p(pt), None)
    assert step(gi=None) == -1 and step(pt=None) == -1 and step(B=0) == -1 and step(H=3) == -1 and step(lr=-0.001) == -1
    assert step(lr=NAN) == -1 and step(reg=-1.0) == -1 and step(gd=0.0) == -1
    assert _lib.dispatch_count('align') == n0 and L.oodgan_align_grad_nparts(3, 8) == 0 and L.oodgan_align_grad_nparts(128, 128) == 16
    assert step() == 0 and _lib.dispatch_count('align') == n0 + 1
    with pytest.raises(ValueError):
        ops.similarity_warp(x, torch.zeros(2, 4, device=dev))
    torch.cuda.synchronize()


THETA_STAR = [[0.03, 0.05, 0.04, -0.03], [-0.04, -0.03, -0.05, 0.02], [0.0, 0.0, 0.06, 0.06]]


def test_the_kernels_recover_a_known_alignment(dev):
    """A smooth 64² image (six seeded sinusoids per channel), G = warp(x, theta*) for three theta*; 200 steps of warp -> MSE ->
    ``align_grad_step`` from theta = 0 at rate 0.005: |theta - theta*| <= 1e-4 and the last loss <= 1e-6 of the first, per image.  Every sign
    and every axis flip of the gradient shows here."""
    from oodgan import ops
    S, B, steps = 64, 3, 200
    x = AR.smooth_image(B, 3, S, seed=11).float()
    star = torch.tensor(THETA_STAR, dtype=torch.float32)
    G = AR.warp(x.double(), star).float().to(dev)
    xd = x.to(dev)
    gmul = ops.loss_scale_for(3 * S * S)
    th, g, m, v = (torch.zeros(B, 4, device=dev) for _ in range(4))
    xt, part, t = torch.empty_like(xd), ops.align_grad_parts(B, S, S, dev), _i32(0, dev)
    losses = torch.empty(steps, B, device=dev)
    for i in range(steps):
        ops.similarity_warp(xd, th, out=xt)
        _, gimg = ops.mse_loss_grad(G, xt, grad_mul=gmul, table=losses, row_dev=t)
        ops.align_grad_step(gimg, xd, th, g, m, v, t, steps, lr=0.005, grad_div=gmul, part=part)
        t += 1
    err = (th.cpu() - star).abs().max(1).values
    ratio = (losses[-1] / losses[0]).cpu()
    print(f'recovery: |theta - theta*| {err.tolist()} (bar 1e-4); last / first loss {ratio.tolist()} (bar 1e-6); first loss {losses[0].tolist()}')
    assert (err <= 1e-4).all() and (ratio <= 1e-6).all()


# ------------------------------------------------------------------------------------------------------------- one step of the loop
_STATE = {}


def _state(size, seed=0):
    if (size, seed) not in _STATE:
        P = synth.generator_state(size, seed=seed)
        _STATE.clear()
        _STATE[(size, seed)] = (P, {k: v.double() for k, v in P.items()})
    return _STATE[(size, seed)]


def _share(got, want):
    return (got.double().cpu() - want.double()).abs().max().item() / want.double().abs().max().item()


def _pixel_term(img, xt, kind, s, f):
    """Per-image pixel term of the step in the dtype of ``img``: the mean of rho over the residual, on the view area-pooled by f."""
    r = img - xt
    if f > 1:
        r = F.avg_pool2d(r, f)
    if kind == 'mse':
        return (r * r).mean(dim=(1, 2, 3))
    return robust_ref.rho(r, kind, robust_ref.scale32(s)).mean(dim=(1, 2, 3))


STEP_CASES = {'mse': ('mse', 1), 'huber': ('huber', 1), 'charbonnier-pool2': ('charbonnier', 2), 'geman_mcclure': ('geman_mcclure', 1)}
W_BAR = {'mse': 1e-4, 'huber': 3e-4, 'charbonnier': 3e-4, 'geman_mcclure': 3e-4}          # the project's bars for dL/dW+
INIT = [[0.04, -0.06, 0.05, -0.03], [-0.03, 0.05, -0.04, 0.06]]
# Points whose dL/dW+ is not held to the bar against the PLAIN float64 oracle, by name, as tests/test_hip_fspace.py and
# tests/test_hip_mask_fit.py name their LeakyReLU kinks (image 1 of this recipe is named there as well): (case, image) -> the measured reason.
# They stay held to it against the float64 oracle that takes, for the pre-activations float32 cannot tell from 0 (within 2^-20 of their
# layer's maximum), the side the kernels took.  dL/dW+ does not pass through the code of the alignment: the image gradient it starts from is
# G - x_theta with x_theta the float32 formula's bits.
KINK_POINTS = {
    ('mse', 1): 'dL/dW+ 1.84e-4 against the plain oracle (bar 1e-4)',
    ('geman_mcclure', 1): 'dL/dW+ 5.65e-4 against the plain oracle (bar 3e-4)',
}
ADOPTED_MAX = lambda n_elements: 4 * SLOPE_BAND * n_elements + 8          # noqa: E731  (as tests/test_hip_fspace.py)


@pytest.mark.parametrize('case', list(STEP_CASES))
def test_step_gradients_vs_float64(dev, case):
    """64², B = 2, one step from a non-zero ``align_init``: dL/dW+ (recovered from Adam's first moment) against float64 autograd through the
    oracle generator and the yardstick's warp, per image as a share of the gradient's maximum, held to the project's bars (1e-4 for the square,
    3e-4 for the robust kinds); dL/dtheta (as the step writes it back) held to 4 x the error of the oracle's own float32 autograd, per image.
    dL/dW+ is compared twice, as the step-1 points of tests/test_hip_fspace.py and tests/test_hip_mask_fit.py are: with the plain oracle, and
    with the oracle taking the LeakyReLU side of the pre-activations within 2^-20 of their layer's maximum from the loop's own forward
    (``sspace_ref.given_slopes``: no slope outside the band may differ, the number taken stays within ``ADOPTED_MAX``).  The bar holds against
    the second for every image and against the first for every image not named in ``KINK_POINTS``."""
    from oodgan.engine import GeneratorEngine, WPlusInverter
    size, B = 64, 2
    kind, f = STEP_CASES[case]
    scale = 0.1
    P, P64 = _state(size, 0)
    target, w0, noises = WG.recipe(size, list(range(B)))
    th0 = torch.tensor(INIT, dtype=torch.float32)
    eng = GeneratorEngine({k: v.to(dev) for k, v in P.items()}, size)
    inv = WPlusInverter(eng, align='similarity', align_lr=0.001, align_reg=0.3, pixel_loss=kind, pixel_scale=scale, pixel_size=size // f if f > 1 else None)
    cap, slopes_of = {}, []
    styled = ['conv1'] + [f'convs.{j}' for j in range(2 * (eng.log_size - 2))]

    def on_step(run):
        cap.update(m=run.m.clone(), g=run.thg.clone())
        acts = [run.eng.saved['acts'][nm] for nm in styled]     # the side of zero every pre-activation of the loop's own forward lies on
        slopes_of[:] = [((a.to_nchw() if hasattr(a, 'to_nchw') else a) > 0).cpu() for a in acts]
    inv.on_step = on_step
    w, losses = inv.invert(target.to(dev), w0.to(dev), [n.to(dev) for n in noises], steps=1, align_init=th0.to(dev))
    torch.cuda.synchronize()
    assert inv.last_stats == {'steps_run': [1], 'rollbacks': [0]}
    assert torch.equal(losses, inv.last_terms['pixel'] + 0.3 * inv.last_terms['align'])
    fails = []
    for k in range(B):
        gw = WG.recover_grad(torch.zeros_like(w0[k]), cap['m'][k].cpu(), inv.betas[0])

        def oracle(dt, state):
            wl = w0[k:k + 1].to(dt).clone().requires_grad_(True)
            tl = th0[k:k + 1].to(dt).clone().requires_grad_(True)
            img = R.generator_forward(state, wl, [n[k:k + 1].to(dt) for n in noises], size)
            tot = _pixel_term(img, AR.warp(target[k:k + 1], tl, dt), kind, scale, f).sum() + 0.3 * (tl.to(dt) ** 2).sum()
            tot.backward()
            return tot.item(), wl.grad[0], tl.grad[0]
        tot, gw64, gt64 = oracle(torch.float64, P64)
        _, _, gt32 = oracle(torch.float32, P)
        with given_slopes([s_[k:k + 1] for s_ in slopes_of]) as gs_:
            _, gw64s, _ = oracle(torch.float64, P64)
        n_el, taken, outside = sum(s_[k:k + 1].numel() for s_ in slopes_of), sum(gs_.adopted), sum(gs_.outside)
        es_w, kept = _share(gw, gw64s), (case, k) not in KINK_POINTS
        print(f'[{case}] image {k}, slopes within 2^-20 of the layer maximum as the engine took them: dL/dW+ {es_w:.2e}; {taken} of {n_el} slopes '
              f'taken (at most {ADOPTED_MAX(n_el):.0f}), {outside} differ outside the band' + ('' if kept else '  [named in KINK_POINTS]'))
        if outside != 0 or not taken <= ADOPTED_MAX(n_el):
            fails.append(f'image {k}: {outside} slopes differ outside the band, {taken} taken')
        e_w, e_loss = _share(gw, gw64), abs(losses[0, k].item() - tot) / tot
        e_t, e_y = (cap['g'][k].cpu().double() - gt64).abs().max().item(), (gt32.double() - gt64).abs().max().item()
        print(f'[{case}] image {k}: dL/dW+ {e_w:.2e} of max (bar {W_BAR[kind]:.0e}); dL/dtheta {e_t:.2e} (the oracle in float32 {e_y:.2e}, bar 4 x; '
              f'dL/dtheta {gt64.tolist()}); loss rel {e_loss:.2e}')
        if not es_w <= W_BAR[kind] or (kept and not e_w <= W_BAR[kind]):
            fails.append(f'image {k}: dL/dW+ {e_w:.2e} plain, {es_w:.2e} given slopes')
        if not e_t <= 4 * e_y:
            fails.append(f'image {k}: dL/dtheta {e_t:.2e} > 4 x {e_y:.2e}')
        if not e_loss <= 1e-5:
            fails.append(f'image {k}: loss {e_loss:.2e}')
    assert not fails, f'[{case}] ' + '; '.join(fails)


# ------------------------------------------------------------------------------------------------------------- the loop against the reference
def _fixture_run(g, dev, **ctor):
    from oodgan.engine import GeneratorEngine, WPlusInverter
    size, B, steps = (int(v) for v in g['meta'])
    sw, sn, s_w, s_start = (int(v) for v in g['seeds'])
    lr, alr = (float(v) for v in g['settings'])
    eng = GeneratorEngine({k: v.to(dev) for k, v in synth.generator_state(size, seed=sw).items()}, size)
    w_star = synth.make_latents(size, B, seed=s_w, std=0.3)
    w0 = (w_star + 0.1 * synth.normal('align.start', tuple(w_star.shape), s_start)).to(dev)
    noises = [n.to(dev) for n in synth.make_noises(size, B, seed=sn)]
    kw = dict(lr=lr, align='similarity', align_lr=alr)
    kw.update(ctor)
    return eng, WPlusInverter(eng, **kw), g['target'].to(dev), w0, noises, steps


@pytest.fixture(scope='module')
def fixture_result(dev, golden):
    """The fixture's case run once through the default loop (launch plan), theta after every step captured; shared, left unchanged."""
    g = golden('wplus_align_64.npz')
    eng, inv, x, w0, noises, steps = _fixture_run(g, dev)
    thetas = {}
    inv.on_step = lambda run: thetas.__setitem__(run.t, run.th.clone())
    w, losses = inv.invert(x, w0, noises, steps=steps)
    torch.cuda.synchronize()
    return dict(g=g, w=w, losses=losses, theta=inv.last_alignment, xa=inv.last_aligned_target, thetas=torch.stack([thetas[t] for t in range(1, steps + 1)]),
                stats=inv.last_stats, plan=inv.last_plan, steps=steps, x=x)


def test_loop_vs_reference(fixture_result):
    """20 steps at 64², B = 2, against the reference Generator's autograd + torch.optim.Adam on [w, theta] with torch's own grid_sample: the loss
    curve within 1e-3 relative of the float64 run (the project's bar for loop curves), theta after every step within 4 x the fixture's own
    float32-against-float64 distance (3.65e-7: the band is 1.46e-6)."""
    from oodgan import ops
    r, g = fixture_result, fixture_result['g']
    assert r['stats'] == {'steps_run': [r['steps']], 'rollbacks': [0]} and r['plan']['steps'] == [r['steps'] - 3]
    rel = lambda p, q: ((p - q).abs() / q.abs()).max().item()     # noqa: E731
    own_l, err_l = rel(g['losses_f32'].double(), g['losses_f64']), rel(r['losses'].double().cpu(), g['losses_f64'])
    own_t = (g['theta_f32'] - g['theta_f64']).abs().max().item()
    err_t = (r['thetas'].double().cpu() - g['theta_f64']).abs().max().item()
    err_w = (r['w'].double().cpu() - g['w_T_f64']).abs().max().item()
    print(f'loop vs reference: loss curve rel {err_l:.2e} (bar 1e-3; the fixture fp32 vs float64 {own_l:.2e}); theta {err_t:.2e} (band {4 * own_t:.2e} = '
          f'4 x the fixture\'s {own_t:.2e}); w_T max diff {err_w:.2e} (the fixture {(g["w_T_f32"].double() - g["w_T_f64"]).abs().max().item():.2e}); '
          f'theta_T {r["theta"].tolist()}; loss {r["losses"][0].tolist()} -> {r["losses"][-1].tolist()}')
    assert own_l <= 2.5e-4          # the fixture's own gap stays under a quarter of the bar
    assert torch.equal(r['thetas'][-1], r['theta']) and torch.equal(r['xa'], ops.similarity_warp(r['x'], r['theta']))
    assert err_l <= 1e-3
    assert err_t <= 4 * own_t


# ------------------------------------------------------------------------------------------------------------- run forms and identities
def test_plan_and_python_loop_agree_bit_for_bit(dev, fixture_result):
    r = fixture_result
    eng, inv, x, w0, noises, steps = _fixture_run(r['g'], dev, use_plan=False)
    w, losses = inv.invert(x, w0, noises, steps=steps)
    assert inv.last_plan['steps'] == [0] and r['plan']['launches'][0] > 0
    assert torch.equal(losses, r['losses']) and torch.equal(w, r['w']) and torch.equal(inv.last_alignment, r['theta'])


@pytest.mark.parametrize('pixel_size', [None, 32])
def test_rate_zero_is_the_run_without_the_option(dev, fixture_result, pixel_size):
    """``align_lr=0`` from the identity: x_theta is the target's bits at every step, so losses and latents are those of the run without the
    option, bit for bit (plan and Python-driven alike), and the recorded step is the default's plus the documented extras: the warp, the two
    launches of the step and, with ``pixel_size``, the pool of x_theta.  Without ``align`` the counter "align" does not move."""
    from oodgan import _lib
    r = fixture_result
    extra = dict(pixel_size=pixel_size, pixel_loss='huber') if pixel_size else {}
    eng, inv, x, w0, noises, steps = _fixture_run(r['g'], dev, align=None, **extra)
    n0 = _lib.dispatch_count('align')
    w_b, l_b = inv.invert(x, w0, noises, steps=steps)
    assert _lib.dispatch_count('align') == n0 and inv.last_alignment is None and inv.last_terms['align'] is None
    launches = inv.last_plan['launches'][0]
    for use_plan in (True, False):
        eng, inv0, x, w0, noises, steps = _fixture_run(r['g'], dev, align_lr=0.0, use_plan=use_plan, **extra)
        w, losses = inv0.invert(x, w0, noises, steps=steps)
        assert torch.equal(w, w_b) and torch.equal(losses, l_b) and (inv0.last_alignment == 0).all() and torch.equal(inv0.last_aligned_target, x)
        if use_plan:
            assert inv0.last_plan['launches'][0] == launches + 3 + (1 if pixel_size else 0), (inv0.last_plan, launches)
            assert _lib.dispatch_count('align') > n0
    # ... and with a rate the option moves the run, the pooled view included
    eng, inv1, x, w0, noises, steps = _fixture_run(r['g'], dev, **extra)
    w1, l1 = inv1.invert(x, w0, noises, steps=steps)
    assert torch.isfinite(l1).all() and (inv1.last_alignment != 0).all() and not torch.equal(l1, l_b) and inv1.last_stats['rollbacks'] == [0]
    print(f'pixel_size {pixel_size}: loss {l_b[-1].tolist()} without, {l1[-1].tolist()} with align; theta_T {inv1.last_alignment.tolist()}')


def test_two_streams_stay_within_half_a_percent(dev, fixture_result):
    r = fixture_result
    eng, inv, x, w0, noises, steps = _fixture_run(r['g'], dev)
    w, losses = inv.invert(x, w0, noises, steps=steps, streams=2)
    rel = ((losses - r['losses']).abs() / r['losses']).max().item()
    dth = (inv.last_alignment - r['theta']).abs().max().item()
    print(f'two streams vs one: loss rel diff {rel:.2e} (bar 5e-3), theta diff {dth:.2e}; plan {inv.last_plan}')
    assert rel <= 5e-3 and inv.last_plan['steps'] == [steps - 3] * 2 and inv.last_stats['rollbacks'] == [0, 0]
    assert inv.last_alignment.shape == (2, 4) and inv.last_aligned_target.shape == x.shape
    assert dth <= 5e-3 * 0.002 * steps          # the same share of the farthest theta can travel, rate x steps


def test_rollback_restores_theta_and_its_moments(dev, fixture_result):
    """The noise maps scaled by 2^30 for one step (after step 10 of 20): the guard flags the window, the run goes back to its last clean
    snapshot — (theta, its m, its v) with (w, m, v) — repeats it with exact scales and ends where the undisturbed run ends."""
    r = fixture_result
    eng, inv, x, w0, noises, steps = _fixture_run(r['g'], dev)
    seen = []

    def scale(run):
        if run.steps_run == 10 and not seen:
            seen.append(1)
            for n in run.noises:
                n.mul_(2.0 ** 30)
        elif run.steps_run == 11 and len(seen) == 1:
            seen.append(2)
            for n in run.noises:
                n.mul_(2.0 ** -30)
    inv.on_step = scale
    w, losses = inv.invert(x, w0, noises, steps=steps)
    rel = ((losses - r['losses']).abs() / r['losses']).max().item()
    dth = (inv.last_alignment - r['theta']).abs().max().item()
    print(f'noise maps x 2^30 for step 11 of {steps}: {inv.last_stats}; loss rel diff {rel:.2e} (bar 1e-3), |theta - undisturbed| {dth:.2e} (bar 1e-4)')
    assert seen == [1, 2] and inv.last_stats['rollbacks'] == [1]
    assert torch.isfinite(losses).all() and rel < 1e-3 and dth < 1e-4


def test_composition_and_refusals(dev, fixture_result):
    """The alignment beside the other options of the loop — latent_space 'w', layer_lr + delta_reg, the schedule, align_reg — every run finite,
    without a rollback, with a theta that moved; and what it does not go with, refused before anything is launched."""
    from oodgan import _lib
    from oodgan.engine import WPlusInverter
    r = fixture_result
    for ctor in (dict(latent_space='w'), dict(layer_lr=[1.0] * 5 + [0.5] * 5, delta_reg=0.1), dict(lr_rampup=0.05, lr_rampdown=0.25, latent_noise=0.05),
                 dict(align_reg=0.5, pixel_loss='geman_mcclure')):
        eng, inv, x, w0, noises, steps = _fixture_run(r['g'], dev, **ctor)
        w, losses = inv.invert(x, w0, noises, steps=6)
        print(f'{sorted(ctor)}: loss {losses[0].tolist()} -> {losses[-1].tolist()}, theta {inv.last_alignment.tolist()}')
        assert inv.last_stats == {'steps_run': [6], 'rollbacks': [0]} and inv.last_plan['steps'] == [3]
        assert torch.isfinite(losses).all() and torch.isfinite(w).all() and (inv.last_alignment != 0).all()
        assert (inv.last_terms['align'] is not None) == ('align_reg' in ctor)
    eng, inv, x, w0, noises, steps = _fixture_run(r['g'], dev)
    n0 = _lib.dispatch_count('align')
    with pytest.raises(NotImplementedError, match='use_graph'):
        inv.invert(x, w0, noises, steps=4, use_graph=True)
    with pytest.raises(NotImplementedError, match='loss_region'):
        inv.invert(x, w0, noises, steps=4, loss_weight=torch.ones(2, 1, 64, 64, device=dev))
    for ctor, what in ((dict(ssim_weight=0.5), 'SSIM'), (dict(pixel_size=32, pixel_filter='bicubic'), 'pixel_filter'), (dict(latent_space='s'), 'latent_space'),
                       (dict(feature_layer=5), 'feature_layer'), (dict(mask_size=16), 'loss_region')):
        with pytest.raises(NotImplementedError, match=what):
            kw = dict(mask_logits=torch.zeros(2, 1, 16, 16, device=dev)) if 'mask_size' in ctor else {}
            WPlusInverter(eng, align='similarity', **ctor).invert(x, w0, noises, steps=4, **kw)
    for init in (torch.zeros(3, 4, device=dev), torch.zeros(2, 4), torch.zeros(2, 4, device=dev, dtype=torch.float64),
                 torch.full((2, 4), NAN, device=dev)):
        with pytest.raises(ValueError, match='align_init'):
            inv.invert(x, w0, noises, steps=4, align_init=init)
    with pytest.raises(ValueError, match='align_init'):
        WPlusInverter(eng).invert(x, w0, noises, steps=4, align_init=torch.zeros(2, 4, device=dev))
    assert _lib.dispatch_count('align') == n0


# ------------------------------------------------------------------------------------------------------------- model level
def test_model_outputs_at_64(dev):
    """``invert(align=)`` sets ``last_alignment`` and ``last_aligned_input``; its output is the model's own forward on x_a at the refined
    latents; ``align_init`` and the rates reach the loop; without the option both attributes are None; a warp and its inverse return the
    interior of a smooth image."""
    import test_hip_wplus_sched as S
    from oodgan import ops
    size, B, steps = 64, 2, 6
    md = S._model_64(dev)
    x = synth.make_images(size, B, seed=44).to(dev)
    kw = dict(enc_lats=synth.make_latents(size, B, seed=42, std=0.3).to(dev), noise=[n.to(dev) for n in synth.make_noises(size, B, seed=45)])
    th0 = torch.tensor(INIT, device=dev)
    out, lats, losses = md.invert(x, steps=steps, align='similarity', align_lr=0.002, align_reg=0.1, align_init=th0, **kw)
    th, xa = md.last_alignment, md.last_aligned_input
    assert th.shape == (B, 4) and xa.shape == x.shape and (th != th0).all() and torch.equal(xa, ops.similarity_warp(x, th))
    assert torch.equal(lats, md.last_refined_lats) and md.last_loss_terms['align'].shape == (steps, B)
    assert torch.equal(losses, md.last_loss_terms['pixel'] + 0.1 * md.last_loss_terms['align'])
    assert abs(md.last_loss_terms['align'][0, 0].item() - sum(v * v for v in INIT[0])) < 1e-7
    assert torch.equal(out, md(xa, lats=lats, **kw)[0])
    out0, lats0, _ = md.invert(x, steps=steps, **kw)
    assert md.last_alignment is None and md.last_aligned_input is None and md.last_loss_terms['align'] is None
    with pytest.raises(ValueError, match='align'):
        md.invert(x, steps=steps, align='affine', **kw)
    with pytest.raises(NotImplementedError, match='SSIM'):
        md.invert(x, steps=steps, align='similarity', ssim_weight=0.5, **kw)
    # the public resampler and its inverse
    s = AR.smooth_image(B, 3, size, seed=5).float().to(dev)
    ti = ops.similarity_inverse(th0)
    back = ops.similarity_warp(ops.similarity_warp(s, th0), ti)
    back64 = AR.warp(AR.warp(s.cpu().double(), th0.cpu()), ti.cpu())
    e, e64 = (back - s)[:, :, 8:-8, 8:-8].abs().max().item(), (back.cpu().double() - back64).abs().max().item()
    print(f'warp and inverse warp of a smooth image: interior max diff to the image {e:.2e} (two bicubic resamplings of sinusoids of up to three '
          f'periods; bar 0.05), to the float64 yardstick\'s round trip {e64:.2e} (bar 1e-5)')
    assert e <= 0.05 and e64 <= 1e-5


class _EncoderStub(torch.nn.Module):
    """An encoder whose outputs depend on its input: fixed latents, and the seeded feature pyramid scaled by the local brightness of the
    256² image it is shown — features of x_a differ from features of x."""

    def __init__(self, lats, feats):
        super().__init__()
        self.lats, self.feats = lats, feats

    def forward(self, x256, return_feats=False):
        lum = x256.mean(1, keepdim=True)
        feats = [f * (1.0 + 0.5 * F.interpolate(lum, size=f.shape[-2:], mode='bilinear', align_corners=False)) for f in self.feats]
        return (self.lats, feats) if return_feats else self.lats


def test_model_with_modulation_takes_its_features_from_the_aligned_input(dev):
    """256², the model with its modulation blocks and blend: the encoder features of the final OOD forward are those of x_a — from the
    attached encoder, or from ``enc_feats`` given as a callable — and the forward and the blend run on x_a: the output is the model's own
    forward on x_a at the refined latents, bit for bit, and not the one on x.  Features handed in as tensors (those of x), or no source of
    features at all, are refused before anything of the option is launched."""
    from oodgan import _lib
    from oodgan.arch import _MissingEncoder, ood_faceGAN_e4e
    size, B, steps = 256, 2, 4
    md = ood_faceGAN_e4e(out_size=size, style_dim=512, encoder='E4E', enable_modulation=True, warp_scale=0.08, cycle_align=2, blend_with_gen=True,
                         ModSize=256, build_encoder=False)
    res = md.load_state_dict(synth.ood_state(size, seed=41), strict=False)
    assert not res.missing_keys and not res.unexpected_keys, res
    md = md.to(dev).eval()
    x = synth.make_images(size, B, seed=44).to(dev)
    enc_lats = synth.make_latents(size, B, seed=42, std=0.3).to(dev)
    base = [f.to(dev) for f in synth.make_encoder_feats(B, seed=43)]
    noise = [n.to(dev) for n in synth.make_noises(size, B, seed=45)]
    th0 = torch.tensor(INIT, device=dev)
    stub = _EncoderStub(enc_lats, base).to(dev).eval()
    # an attached encoder
    md.encoder = stub
    out, lats, losses = md.invert(x, steps=steps, align='similarity', align_lr=0.002, align_init=th0, noise=noise)
    xa, th = md.last_aligned_input, md.last_alignment
    assert torch.isfinite(out).all() and (th != th0).all() and not torch.equal(xa, x)
    want = md(xa, lats=lats, noise=noise)[0]
    other = md(x, lats=lats, noise=noise)[0]
    print(f'modulation model at {size}²: |out - forward on x_a| {(out - want).abs().max().item():.1e}, |out - forward on x| {(out - other).abs().max().item():.2e}')
    assert torch.equal(out, want) and not torch.equal(out, other)
    # no encoder, the features as a callable of the aligned input
    md.encoder = _MissingEncoder()
    seen = []

    def feats_of(img):
        seen.append(img)
        return stub(torch.nn.functional.interpolate(img, size=(256, 256), mode='bilinear', align_corners=False), return_feats=True)[1]
    out2, lats2, losses2 = md.invert(x, steps=steps, align='similarity', align_lr=0.002, align_init=th0, noise=noise, enc_lats=enc_lats, enc_feats=feats_of)
    assert len(seen) == 1 and torch.equal(seen[0], md.last_aligned_input) and torch.equal(losses2, losses) and torch.equal(lats2, lats)
    assert torch.equal(out2, md(md.last_aligned_input, lats=lats2, noise=noise, enc_lats=enc_lats, enc_feats=feats_of(md.last_aligned_input))[0])
    # features of x as tensors, or none: refused before the loop
    n0 = _lib.dispatch_count('align')
    with pytest.raises(ValueError, match='enc_feats'):
        md.invert(x, steps=steps, align='similarity', noise=noise, enc_lats=enc_lats, enc_feats=base)
    with pytest.raises(ValueError, match='encoder'):
        md.invert(x, steps=steps, align='similarity', noise=noise, enc_lats=enc_lats)
    assert _lib.dispatch_count('align') == n0
    # without the option tensors stay what they were
    out3, _, _ = md.invert(x, steps=steps, noise=noise, enc_lats=enc_lats, enc_feats=base)
    assert md.last_alignment is None and torch.isfinite(out3).all()
