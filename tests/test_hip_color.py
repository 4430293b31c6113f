"""The colour map of the generator image beside the latents of the W+ loop: ``WPlusInverter(color='gain' | 'affine')`` fits,
per image, theta = (M, b) and takes the pixel term on M G + b.

The entries of csrc/loss_color.hip against the float64 yardstick (tests/color_ref.py) — loss and image gradient at the bars of
tests/test_hip_robust_loss.py, dL/dtheta at 4 x the error of the same formula's torch-CPU float32 autograd (the rule of §25) with the one
rounding of the result as floor —, bit for bit against the plain pixel kernels at the identity and against themselves; theta recovered by
the kernels alone; dL/dW+ and dL/dtheta of one step of the running loop against float64 autograd through the oracle; the loop against the
reference's own autograd + torch.optim.Adam on [w, theta] (tests/golden/wplus_color_64.npz); the run forms (launch plan, Python-driven, two
streams, rollback, ``color_lr`` 0 against the run without the option); the model-level outputs."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from oracle import ref_cpu as R  # noqa: E402
from oodgan import synth  # noqa: E402
import color_ref as CR  # noqa: E402
from sspace_ref import SLOPE_BAND, given_slopes  # noqa: E402
import wplus_grads as WG  # noqa: E402

# 16²: less than one block's span; 37x53: odd HW, the scalar form; 64²: two blocks per image; 128²: HW = kMseChunk; 128x256: two of them
SHAPES = [(16, 16), (37, 53), (64, 64), (128, 128), (128, 256)]
NAN, INF = float('nan'), float('inf')
THIRD = (0.9, -0.1, 0.2, 0.05, 1.1, -0.15, 0.1, 0.0, 0.95, 0.1, -0.08, 0.03)


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


def _i32(v, dev):
    return torch.tensor([v], dtype=torch.int32, device=dev)


def _thetas():
    """name -> the theta of image 0, 1, 2."""
    s0, s1 = CR.THETA_STAR
    return {'identity': [CR.IDENTITY] * 3, 'gain*': [s0] * 3, 'affine*': [s1] * 3, 'per-image': [s1, s0, THIRD]}


def _beta(B, H, W, gen):
    """A seeded, non-binary plane in [0, 1] with an exact-zero and an exact-one block."""
    b = torch.rand(B, 1, H, W, generator=gen)
    b[:, :, : H // 4, : W // 4] = 0.0
    b[:, :, -(H // 4):, -(W // 4):] = 1.0
    return b.contiguous()


def _theta_grad(parts, th, dev, grad_div, kind='affine', reg=0.0, **sink):
    """dL/dtheta as ``color_step`` writes it back, with a rate of 0 (theta stays)."""
    from oodgan import ops
    B = th.shape[0]
    g, m, v = (torch.zeros(B, 12, device=dev) for _ in range(3))
    th_d = th.to(dev).clone()
    ops.color_step(th_d, g, m, v, parts[1], _i32(0, dev), 1, lr=0.0, grad_div=grad_div, kind=kind, color_reg=reg, **sink)
    assert torch.equal(th_d.cpu(), th)
    return g


@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: f'{s[0]}x{s[1]}')
def test_kernels_vs_float64(dev, shape):
    """The fused term, dL/dtheta and ``color_apply`` for B in {1, 3} x four kinds x s in {1e-6, 0.5} x with and without a loss weight x four
    thetas, images and targets N(0,1): loss <= 1e-6 relative, gimg <= 1e-6 of its maximum, dL/dtheta <= max(4 x the error of the formula's
    torch-CPU float32 autograd, 1e-6 max |dL/dtheta|), each against the float64 yardstick.  At the identity gimg is the plain kernels'
    gradient and ``color_apply`` the source, bit for bit.  The table sink, and a second call, give the same bits."""
    from oodgan import ops
    H, W = shape
    gmul = ops.loss_scale_for(3 * H * W)
    fails, worst = [], dict(loss=0.0, gimg=0.0, dth=0.0, apply=0.0)
    for B in (1, 3):
        gen = torch.Generator().manual_seed(1000 * H + 10 * W + B)
        img, x = torch.randn(B, 3, H, W, generator=gen), torch.randn(B, 3, H, W, generator=gen)
        beta = _beta(B, H, W, gen)
        a, t, w = img.to(dev), x.to(dev), beta.to(dev)
        for name, rows in _thetas().items():
            th = torch.tensor(rows[:B], dtype=torch.float32)
            thd = th.to(dev)
            y = ops.color_apply(a, thd)
            y64 = CR.apply(img.double(), th.double())
            e_y = (y.double().cpu() - y64).abs().max().item() / y64.abs().max().item()
            worst['apply'] = max(worst['apply'], e_y)
            if not e_y <= 1e-6:
                fails.append(f'B={B} {name}: color_apply {e_y:.2e}')
            if name == 'identity' and not torch.equal(y, a):
                fails.append(f'B={B}: color_apply at the identity does not return the source bit for bit')
            if not torch.equal(ops.color_apply(a.clone(), thd), y):
                fails.append(f'B={B} {name}: a second color_apply gives other bits')
            for kind in CR.KINDS:
                for s in (1e-6, 0.5):
                    for bt, btd in ((None, None), (beta, w)):
                        tag = f'B={B} {name} {kind} s={s:g} beta={bt is not None}'
                        l64, g64, d64, _ = CR.term(img, x, th, kind, s, bt, grad_mul=gmul, grad_div=gmul)
                        _, _, d32 = CR.autograd_term(img, x, th, kind, s, bt, dtype=torch.float32)
                        loss, gimg, parts = ops.color_pixel_loss_grad(a, t, thd, kind, s, btd, gmul)
                        dth = _theta_grad(parts, th, dev, gmul)
                        e_l = ((loss.double().cpu() - l64).abs() / l64).max().item()
                        e_g = (gimg.double().cpu() - g64).abs().max().item() / g64.abs().max().item()
                        e_t, e_32 = (dth.double().cpu() - d64).abs().max().item(), (d32.double() - d64).abs().max().item()
                        bar_t = max(4 * e_32, 1e-6 * d64.abs().max().item())
                        print(f'{H}x{W} {tag}: loss rel {e_l:.2e}, gimg {e_g:.2e} of max (bars 1e-6); dL/dtheta {e_t:.2e} (bar {bar_t:.2e}: float32 '
                              f'autograd {e_32:.2e}, max |dL/dtheta| {d64.abs().max().item():.2e})')
                        worst.update(loss=max(worst['loss'], e_l), gimg=max(worst['gimg'], e_g), dth=max(worst['dth'], e_t / bar_t))
                        if not e_l <= 1e-6:
                            fails.append(f'{tag}: loss {e_l:.2e}')
                        if not e_g <= 1e-6:
                            fails.append(f'{tag}: gimg {e_g:.2e}')
                        if not e_t <= bar_t:
                            fails.append(f'{tag}: dL/dtheta {e_t:.2e} > {bar_t:.2e}')
                        if name == 'identity':
                            lp, gp, _ = ops.pixel_loss_grad(a, t, kind, s, btd, gmul, wrt='gen')
                            if not torch.equal(gimg, gp):
                                fails.append(f'{tag}: gimg is not the plain kernel\'s gradient bit for bit')
                            if not ((loss - lp).abs() <= 1e-6 * lp.abs()).all():
                                fails.append(f'{tag}: loss {loss.tolist()} vs the plain kernel\'s {lp.tolist()}')
                        # equal inputs, equal bits; the table row is the plain sink's value
                        loss2, gimg2, parts2 = ops.color_pixel_loss_grad(a, t, thd, kind, s, btd, gmul)
                        if not (torch.equal(loss2, loss) and torch.equal(gimg2, gimg) and torch.equal(parts2[1], parts[1])
                                and torch.equal(_theta_grad(parts2, th, dev, gmul), dth)):
                            fails.append(f'{tag}: a second call gives other bits')
                        tb = torch.full((3, B), -1.0, device=dev)
                        none, gimg3, parts3 = ops.color_pixel_loss_grad(a, t, thd, kind, s, btd, gmul, table=tb, row_dev=_i32(1, dev))
                        if not (none is None and torch.equal(tb[1], loss) and (tb[[0, 2]] == -1).all() and torch.equal(gimg3, gimg)
                                and torch.equal(parts3[1], parts[1])):
                            fails.append(f'{tag}: the table sink differs from the plain one')
    print(f'{H}x{W}: worst loss rel {worst["loss"]:.2e}, gimg {worst["gimg"]:.2e}, color_apply {worst["apply"]:.2e} (bars 1e-6); dL/dtheta at '
          f'{worst["dth"]:.2f} of its bar')
    assert not fails, '; '.join(fails[:12]) + f' ({len(fails)} in all)'


def test_color_step_vs_float64_adam(dev):
    """Three steps on seeded partial sums against Adam in float64 (the loop's betas as float32 numbers, its ramp factor), 'affine' and 'gain',
    with the regulariser: theta within 1e-6 max(1, max |theta|), the g written back, m and v within 1e-6 of their maxima (the bars of
    tests/test_hip_latent_controls.py for ``oodgan_latent_step``); 'gain' leaves its six fixed numbers at their start bits (m, v = 0,
    g = 0); the regulariser's row within 1e-6 relative; the counter is read, not incremented."""
    from oodgan import ops
    B, nparts, total, lr, reg, gd = 3, 70, 20, 0.01, 0.3, 64.0
    up, down = 0.1, 0.25
    for kind in ('affine', 'gain'):
        gen = torch.Generator().manual_seed(17)
        th0 = torch.tensor(_thetas()['per-image'], dtype=torch.float32)
        th, (g, m, v) = th0.to(dev).clone(), (torch.zeros(B, 12, device=dev) for _ in range(3))
        r_th, r_m, r_v = th0.double(), torch.zeros(B, 12, dtype=torch.float64), torch.zeros(B, 12, dtype=torch.float64)
        table, t = torch.full((total, B), -1.0, device=dev), _i32(4, dev)
        free = CR.free_mask(kind)
        for i in range(3):
            dpart = torch.randn(B, nparts, 12, generator=gen, dtype=torch.float64) * 10.0 ** (-i)
            th_before = th.clone()
            ops.color_step(th, g, m, v, dpart.to(dev), t, total, up, down, lr, grad_div=gd, kind=kind, color_reg=reg, table=table)
            off = th_before.double().cpu() - CR.identity(B, torch.float64)
            g_ref = (dpart.sum(1) / gd + 2.0 * reg * off) * free
            r_th, r_m, r_v = CR.adam(r_th, g_ref, r_m, r_v, 5 + i, lr, free=kind, total_steps=total, rampup=up, rampdown=down)
            e = dict(theta=(th.double().cpu() - r_th).abs().max().item() / max(1.0, r_th.abs().max().item()),
                     g=(g.double().cpu() - g_ref).abs().max().item() / g_ref.abs().max().item(),
                     m=(m.double().cpu() - r_m).abs().max().item() / r_m.abs().max().item(),
                     v=(v.double().cpu() - r_v).abs().max().item() / r_v.abs().max().item(),
                     reg=((table[4 + i].double().cpu() - (off * off).sum(1)).abs() / (off * off).sum(1)).max().item())
            print(f'color_step {kind} step {i}: ' + ', '.join(f'{k} {x:.2e}' for k, x in e.items()) + ' (bars 1e-6)')
            assert max(e.values()) <= 1e-6 and int(t.item()) == 4 + i
            assert (table[:4] == -1).all() and (table[5 + i:] == -1).all()
            r_th = th.double().cpu()            # the next step starts from the kernel's float32 theta, as the loop's does
            t += 1
        if kind == 'gain':
            fixed = [1, 2, 3, 5, 6, 7]
            assert torch.equal(th[:, fixed].cpu(), th0[:, fixed]) and (g[:, fixed] == 0).all() and (m[:, fixed] == 0).all() and (v[:, fixed] == 0).all()
            assert (th[:, [0, 4, 8, 9, 10, 11]].cpu() != th0[:, [0, 4, 8, 9, 10, 11]]).all()
        # a rate of 0 leaves theta as it is
        keep = th.clone()
        ops.color_step(th, g, m, v, dpart.to(dev), t, total, lr=0.0, grad_div=gd, kind=kind)
        assert torch.equal(th, keep)


@pytest.mark.parametrize('shape', [(16, 16), (37, 53)], ids=lambda s: f'{s[0]}x{s[1]}')
def test_non_finite_theta_runs_to_its_end(dev, shape):
    """NaN or inf in any place of one image's theta: every entry runs to its end; values of that image are not compared.  The finite
    images beside it in the batch keep their bits."""
    from oodgan import ops
    H, W = shape
    gen = torch.Generator().manual_seed(7)
    a, t = torch.randn(3, 3, H, W, generator=gen).to(dev), torch.randn(3, 3, H, W, generator=gen).to(dev)
    good = list(CR.THETA_STAR[1])

    def run(rows):
        th = torch.tensor(rows, dtype=torch.float32, device=dev)
        y = ops.color_apply(a, th)
        loss, gimg, parts = ops.color_pixel_loss_grad(a, t, th, 'huber', 0.5, grad_mul=64.0)
        g, m, v = (torch.zeros(3, 12, device=dev) for _ in range(3))
        ops.color_step(th, g, m, v, parts[1], _i32(0, dev), 10, lr=0.01, grad_div=64.0, color_reg=0.1)
        torch.cuda.synchronize()
        return y, loss, gimg, th, g
    want = run([good] * 3)
    for k in range(12):
        for bad_v in (NAN, INF, -INF):
            bad = list(good)
            bad[k] = bad_v
            got = run([good, bad, good])
            for p, q in zip(got, want):
                assert torch.equal(p[0], q[0]) and torch.equal(p[2], q[2]), (k, bad_v)
    got = run([good, [NAN] * 12, good])
    assert all(torch.equal(p[[0, 2]], q[[0, 2]]) for p, q in zip(got, want))


def test_bad_arguments_launch_nothing(dev):
    from oodgan import _lib, ops
    L = _lib.lib()
    p = ops._p
    a, x, gi = (torch.zeros(1, 3, 8, 8, device=dev) for _ in range(3))
    w = torch.ones(1, 1, 8, 8, device=dev)
    th, g, m, v = (ops.color_identity(1, dev) for _ in range(4))
    part, dpart = ops.color_parts(1, 8, 8, dev)
    loss, t = torch.zeros(1, device=dev), _i32(0, dev)
    n0 = _lib.dispatch_count('color')

    def term(img=a, tg=x, th_=th, go=gi, pt=part, dp=dpart, lo=loss, B=1, H=8, W=8, kind=0, s=0.0, gm=1.0, beta=None):
        return L.oodgan_color_pixel_loss_fwd_bwd(p(img), p(tg), p(beta), p(th_), p(go), p(pt), p(dp), p(lo), B, H, W, kind, s, gm, None)

    def row(lo=loss, rd=t, nrows=1, kind=0, s=0.0):
        return L.oodgan_color_pixel_loss_fwd_bwd_row(p(a), p(x), None, p(th), p(gi), p(part), p(dpart), p(lo), p(rd), nrows, 1, 8, 8, kind, s, 1.0, None)

    def step(th_=th, dp=dpart, B=1, nparts=1, mask=0xfff, lr=0.001, reg=0.0, gd=1.0, td=t, total=10):
        return L.oodgan_color_step(p(th_), p(g), p(m), p(v), p(dp), B, nparts, mask, lr, 0.9, 0.999, 1e-8, p(td), total, 0.0, 0.0, gd, reg, None, 0, None)

    def apply(src=a, th_=th, out=gi, B=1, H=8, W=8):
        return L.oodgan_color_apply(p(src), p(th_), p(out), B, H, W, None)
    assert term(img=None) == -1 and b'color_pixel_loss' in L.oodgan_last_error()
    for kw in (dict(tg=None), dict(th_=None), dict(go=None), dict(pt=None), dict(dp=None), dict(lo=None), dict(B=0), dict(B=-1), dict(H=0), dict(W=0),
               dict(kind=4), dict(kind=-1), dict(kind=2, s=0.0), dict(kind=1, s=-0.5), dict(kind=3, s=NAN), dict(kind=1, s=INF), dict(kind=2, s=1e-30),
               dict(gm=NAN)):
        assert term(**kw) == -1, kw
    for kw in (dict(lo=None), dict(rd=None), dict(nrows=0), dict(kind=7), dict(kind=2, s=0.0)):
        assert row(**kw) == -1, kw
    for kw in (dict(th_=None), dict(dp=None), dict(td=None), dict(B=0), dict(nparts=0), dict(mask=0x1000), dict(mask=-1), dict(lr=-0.001), dict(lr=NAN),
               dict(reg=-1.0), dict(reg=NAN), dict(gd=0.0), dict(gd=-1.0), dict(gd=NAN), dict(total=0)):
        assert step(**kw) == -1, kw
    for kw in (dict(src=None), dict(th_=None), dict(out=None), dict(B=0), dict(H=0), dict(W=-3)):
        assert apply(**kw) == -1, kw
    assert _lib.dispatch_count('color') == n0
    assert L.oodgan_color_nparts(0, 8) == 0 and L.oodgan_color_nparts(64, 64) == 2 and L.oodgan_color_nparts(128, 256) == 16
    assert term() == 0 and term(beta=w) == 0 and row() == 0 and step() == 0 and apply() == 0 and _lib.dispatch_count('color') == n0 + 5
    with pytest.raises(ValueError):
        ops.color_apply(a, torch.zeros(2, 12, device=dev))
    with pytest.raises(ValueError):
        ops.color_apply(torch.zeros(1, 1, 8, 8, device=dev), th)
    torch.cuda.synchronize()


@pytest.mark.parametrize('kind', ['affine', 'gain'])
def test_the_kernels_recover_a_known_colour_map(dev, kind):
    """A smooth 64² image (six seeded sinusoids per channel), x = C_theta*(img): 300 steps of the fused term -> ``color_step`` from the
    identity at rate 0.01, MSE: |theta - theta*| <= 1e-4 and the last loss <= 1e-6 of the first, per image.  'affine': the gain/offset and
    the full matrix; 'gain': the gain/offset, which its six numbers can reach.  Every sign and every transposition of dL/dtheta shows here."""
    from oodgan import ops
    S, steps = 64, 300
    rows = list(CR.THETA_STAR) if kind == 'affine' else [CR.THETA_STAR[0]]
    B = len(rows)
    img = CR.smooth_image(B, 3, S, seed=11).float()
    star = torch.tensor(rows, dtype=torch.float32)
    x = CR.apply(img.double(), star.double()).float().to(dev)
    a = img.to(dev)
    gmul = ops.loss_scale_for(3 * S * S)
    th, (g, m, v) = ops.color_identity(B, dev), (torch.zeros(B, 12, device=dev) for _ in range(3))
    parts, gimg, t = ops.color_parts(B, S, S, dev), torch.empty_like(a), _i32(0, dev)
    losses = torch.empty(steps, B, device=dev)
    for i in range(steps):
        ops.color_pixel_loss_grad(a, x, th, 'mse', grad_mul=gmul, table=losses, row_dev=t, parts=parts, out=gimg)
        ops.color_step(th, g, m, v, parts[1], t, steps, lr=0.01, grad_div=gmul, kind=kind)
        t += 1
    err = (th.cpu() - star).abs().max(1).values
    ratio = (losses[-1] / losses[0]).cpu()
    print(f'recovery {kind}: |theta - theta*| {err.tolist()} (bar 1e-4); last / first loss {ratio.tolist()} (bar 1e-6); first loss {losses[0].tolist()}')
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


STEP_CASES = {'mse': ('mse', False, 'affine'), 'huber-beta': ('huber', True, 'affine'), 'charbonnier': ('charbonnier', False, 'affine'),
              'geman_mcclure-gain': ('geman_mcclure', False, 'gain')}
W_BAR = {'mse': 1e-4, 'huber': 3e-4, 'charbonnier': 3e-4, 'geman_mcclure': 3e-4}          # the project's bars for dL/dW+
INIT = [[1.05, 0.03, -0.02, 0.02, 0.95, 0.04, -0.03, 0.01, 1.08, 0.03, -0.02, 0.04],
        [0.92, -0.04, 0.03, 0.05, 1.04, -0.02, 0.02, -0.03, 0.9, -0.05, 0.02, 0.01]]
# Points whose dL/dW+ is not held to the bar against the PLAIN float64 oracle, by name, as tests/test_hip_align.py names the LeakyReLU kinks
# of this recipe: (case, image) -> the measured reason.  They stay held to it against the float64 oracle that takes, for the pre-activations
# float32 cannot tell from 0 (within 2^-20 of their layer's maximum), the side the kernels took.
KINK_POINTS = {
    ('mse', 1): 'dL/dW+ 1.65e-4 against the plain oracle (bar 1e-4), 4.71e-6 with the slopes the kernels took',
    ('geman_mcclure-gain', 1): 'dL/dW+ 4.25e-4 against the plain oracle (bar 3e-4), 5.28e-5 with the slopes the kernels took',
}
ADOPTED_MAX = lambda n_elements: 4 * SLOPE_BAND * n_elements + 8          # noqa: E731  (as tests/test_hip_fspace.py)


@pytest.mark.parametrize('case', list(STEP_CASES))
def test_step_gradients_vs_float64(dev, case):
    """64², B = 2, one step from a non-identity ``color_init`` with ``color_reg`` 0.3: dL/dW+ (recovered from Adam's first moment) against
    float64 autograd through the oracle generator and the yardstick's formula, per image as a share of the gradient's maximum, held to the
    project's bars (1e-4 for the square, 3e-4 for the robust kinds) the way tests/test_hip_align.py holds them: against the oracle that takes
    the LeakyReLU side of the pre-activations within 2^-20 of their layer's maximum from the loop's own forward for every image, and against
    the plain oracle for every image not named in ``KINK_POINTS``.  dL/dtheta (as the step writes it back) within max(4 x the error of the
    oracle's own float32 autograd, 1e-6 of its maximum); the loss within 1e-6 relative."""
    from oodgan.engine import GeneratorEngine, WPlusInverter
    size, B = 64, 2
    kind, with_beta, ckind = STEP_CASES[case]
    scale, reg = 0.1, 0.3
    P, P64 = _state(size, 0)
    target, w0, noises = WG.recipe(size, list(range(B)))
    th0 = torch.tensor(INIT, dtype=torch.float32)
    beta = _beta(B, size, size, torch.Generator().manual_seed(3)) if with_beta else None
    free = CR.free_mask(ckind)
    eng = GeneratorEngine({k: v.to(dev) for k, v in P.items()}, size)
    inv = WPlusInverter(eng, color=ckind, color_lr=0.002, color_reg=reg, pixel_loss=kind, pixel_scale=scale)
    cap, slopes_of = {}, []
    styled = ['conv1'] + [f'convs.{j}' for j in range(2 * (eng.log_size - 2))]

    def on_step(run):
        cap.update(m=run.m.clone(), g=run.ctg.clone())
        acts = [run.eng.saved['acts'][nm] for nm in styled]     # the side of zero every pre-activation of the loop's own forward lies on
        slopes_of[:] = [((a.to_nchw() if hasattr(a, 'to_nchw') else a) > 0).cpu() for a in acts]
    inv.on_step = on_step
    w, losses = inv.invert(target.to(dev), w0.to(dev), [n.to(dev) for n in noises], steps=1, color_init=th0.to(dev),
                           loss_weight=None if beta is None else beta.to(dev))
    torch.cuda.synchronize()
    assert inv.last_stats == {'steps_run': [1], 'rollbacks': [0]}
    assert torch.equal(losses, inv.last_terms['pixel'] + reg * inv.last_terms['color'])
    fails = []
    for k in range(B):
        gw = WG.recover_grad(torch.zeros_like(w0[k]), cap['m'][k].cpu(), inv.betas[0])

        def oracle(dt, state):
            wl = w0[k:k + 1].to(dt).clone().requires_grad_(True)
            tl = th0[k:k + 1].to(dt).clone().requires_grad_(True)
            img = R.generator_forward(state, wl, [n[k:k + 1].to(dt) for n in noises], size)
            off = tl - CR.identity(1, dt)
            pix = CR.formula(img, target[k:k + 1].to(dt), tl, kind, scale, None if beta is None else beta[k:k + 1].to(dt)).sum()
            tot = pix + reg * (off * off).sum()
            tot.backward()
            return tot.item(), wl.grad[0], tl.grad[0] * free.to(dt)
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
        bar_t = max(4 * e_y, 1e-6 * gt64.abs().max().item())
        print(f'[{case}] image {k}: dL/dW+ {e_w:.2e} of max (bar {W_BAR[kind]:.0e}); dL/dtheta {e_t:.2e} (bar {bar_t:.2e}: the oracle in float32 '
              f'{e_y:.2e}, max |dL/dtheta| {gt64.abs().max().item():.2e}); loss rel {e_loss:.2e} (bar 1e-6)')
        if not es_w <= W_BAR[kind] or (kept and not e_w <= W_BAR[kind]):
            fails.append(f'image {k}: dL/dW+ {e_w:.2e} plain, {es_w:.2e} given slopes')
        if not e_t <= bar_t:
            fails.append(f'image {k}: dL/dtheta {e_t:.2e} > {bar_t:.2e}')
        if ckind == 'gain' and not (cap['g'][k][[1, 2, 3, 5, 6, 7]] == 0).all():
            fails.append(f'image {k}: a fixed number has a gradient')
        if not e_loss <= 1e-6:
            fails.append(f'image {k}: loss {e_loss:.2e}')
    assert not fails, f'[{case}] ' + '; '.join(fails)


# ------------------------------------------------------------------------------------------------------------- the loop against the reference
def _fixture_run(g, dev, kind='affine', **ctor):
    from oodgan.engine import GeneratorEngine, WPlusInverter
    size, B, steps = (int(v) for v in g['meta'])
    sw, sn, s_w, s_start = (int(v) for v in g['seeds'])
    lr, clr = (float(v) for v in g['settings'])
    eng = GeneratorEngine({k: v.to(dev) for k, v in synth.generator_state(size, seed=sw).items()}, size)
    w_star = synth.make_latents(size, B, seed=s_w, std=0.3)
    w0 = (w_star + 0.1 * synth.normal('color.start', tuple(w_star.shape), s_start)).to(dev)
    noises = [n.to(dev) for n in synth.make_noises(size, B, seed=sn)]
    kw = dict(lr=lr, color=kind, color_lr=clr)
    kw.update(ctor)
    return eng, WPlusInverter(eng, **kw), g['target'].to(dev), w0, noises, steps


_RESULTS = {}


def _fixture_result(dev, golden, kind):
    """The fixture's case run once through the default loop (launch plan), theta after every step captured; shared, left unchanged."""
    if kind not in _RESULTS:
        g = golden('wplus_color_64.npz')
        eng, inv, x, w0, noises, steps = _fixture_run(g, dev, kind)
        thetas = {}
        inv.on_step = lambda run: thetas.__setitem__(run.t, run.ct.clone())
        w, losses = inv.invert(x, w0, noises, steps=steps)
        torch.cuda.synchronize()
        _RESULTS[kind] = dict(g=g, w=w, losses=losses, theta=inv.last_color, thetas=torch.stack([thetas[t] for t in range(1, steps + 1)]),
                              stats=inv.last_stats, plan=inv.last_plan, steps=steps, x=x, kind=kind,
                              band=4 * (g[f'{kind}_theta_f32'] - g[f'{kind}_theta_f64']).abs().max().item())
    return _RESULTS[kind]


@pytest.fixture(scope='module')
def fixture_result(dev, golden):
    return _fixture_result(dev, golden, 'affine')


@pytest.mark.parametrize('kind', ['affine', 'gain'])
def test_loop_vs_reference(dev, golden, kind):
    """10 steps at 64², B = 2, against the reference Generator's autograd + torch.optim.Adam on [w, theta]: the loss curve within 1e-3 relative
    of the float64 run (the project's bar for loop curves), theta after every step within 4 x the fixture's own float32-against-float64
    distance, read from the fixture.  No gain in quality is asserted: on these seeded weights ten steps do not show one."""
    r = _fixture_result(dev, golden, kind)
    g = r['g']
    assert r['stats'] == {'steps_run': [r['steps']], 'rollbacks': [0]} and r['plan']['steps'] == [r['steps'] - 3]
    rel = lambda p, q: ((p - q).abs() / q.abs()).max().item()     # noqa: E731
    own_l, err_l = rel(g[f'{kind}_losses_f32'].double(), g[f'{kind}_losses_f64']), rel(r['losses'].double().cpu(), g[f'{kind}_losses_f64'])
    err_t = (r['thetas'].double().cpu() - g[f'{kind}_theta_f64']).abs().max().item()
    err_w = (r['w'].double().cpu() - g[f'{kind}_w_T_f64']).abs().max().item()
    print(f'loop vs reference [{kind}]: loss curve rel {err_l:.2e} (bar 1e-3; the fixture fp32 vs float64 {own_l:.2e}); theta {err_t:.2e} (band '
          f'{r["band"]:.2e} = 4 x the fixture\'s own); w_T max diff {err_w:.2e} (the fixture '
          f'{(g[f"{kind}_w_T_f32"].double() - g[f"{kind}_w_T_f64"]).abs().max().item():.2e}); theta_T {r["theta"].tolist()}; loss {r["losses"][0].tolist()} '
          f'-> {r["losses"][-1].tolist()}')
    assert own_l <= 2.5e-4          # the fixture's own gap stays under a quarter of the bar
    assert torch.equal(r['thetas'][-1], r['theta'])
    if kind == 'gain':
        assert torch.equal(r['theta'][:, [1, 2, 3, 5, 6, 7]].cpu(), CR.identity(2)[:, [1, 2, 3, 5, 6, 7]])
    assert err_l <= 1e-3
    assert err_t <= r['band']


# ------------------------------------------------------------------------------------------------------------- run forms and identities
def test_plan_and_python_loop_agree_bit_for_bit(dev, fixture_result):
    r = fixture_result
    eng, inv, x, w0, noises, steps = _fixture_run(r['g'], dev, use_plan=False)
    w, losses = inv.invert(x, w0, noises, steps=steps)
    assert inv.last_plan['steps'] == [0] and r['plan']['launches'][0] > 0
    assert torch.equal(losses, r['losses']) and torch.equal(w, r['w']) and torch.equal(inv.last_color, r['theta'])


@pytest.mark.parametrize('extra', ['mse', 'huber', 'loss-weight'])
def test_rate_zero_is_the_run_without_the_option(dev, fixture_result, extra):
    """``color_lr=0`` from the identity: c is G's bits and gimg the plain kernels' at every step, so the latents are those of the run without
    the option bit for bit (plan and Python-driven alike) and the losses within 1e-6 relative; the recorded step is the default's plus ONE
    launch, asserted against that run.  Without ``color`` the counter "color" does not move and ``last_color`` is None."""
    from oodgan import _lib
    r = fixture_result
    ctor = dict(pixel_loss='huber', pixel_scale=0.2) if extra == 'huber' else {}
    B, S = r['x'].shape[0], r['x'].shape[-1]
    call = dict(loss_weight=_beta(B, S, S, torch.Generator().manual_seed(5)).to(dev)) if extra == 'loss-weight' else {}
    eng, inv, x, w0, noises, steps = _fixture_run(r['g'], dev, None, **ctor)
    n0 = _lib.dispatch_count('color')
    w_b, l_b = inv.invert(x, w0, noises, steps=steps, **call)
    assert _lib.dispatch_count('color') == n0 and inv.last_color is None and inv.last_terms['color'] is None
    launches = inv.last_plan['launches'][0]
    for use_plan in (True, False):
        eng, inv0, x, w0, noises, steps = _fixture_run(r['g'], dev, color_lr=0.0, use_plan=use_plan, **ctor)
        w, losses = inv0.invert(x, w0, noises, steps=steps, **call)
        rel = ((losses - l_b).abs() / l_b.abs()).max().item()
        print(f'{extra}, plan {use_plan}: losses within {rel:.2e} of the run without the option (bar 1e-6)')
        assert torch.equal(w, w_b) and rel <= 1e-6 and torch.equal(inv0.last_color.cpu(), CR.identity(B))
        if use_plan:
            assert inv0.last_plan['launches'][0] == launches + 1, (inv0.last_plan, launches)
            assert _lib.dispatch_count('color') > n0
    # ... and with a rate the option moves the run
    eng, inv1, x, w0, noises, steps = _fixture_run(r['g'], dev, **ctor)
    w1, l1 = inv1.invert(x, w0, noises, steps=steps, **call)
    assert torch.isfinite(l1).all() and not torch.equal(inv1.last_color.cpu(), CR.identity(B)) and not torch.equal(w1, w_b)
    assert inv1.last_stats['rollbacks'] == [0]


def test_two_streams_stay_within_half_a_percent(dev, fixture_result):
    r = fixture_result
    eng, inv, x, w0, noises, steps = _fixture_run(r['g'], dev)
    w, losses = inv.invert(x, w0, noises, steps=steps, streams=2)
    rel = ((losses - r['losses']).abs() / r['losses']).max().item()
    dth = (inv.last_color - r['theta']).abs().max().item()
    print(f'two streams vs one: loss rel diff {rel:.2e} (bar 5e-3), theta diff {dth:.2e} (band {r["band"]:.2e}); plan {inv.last_plan}')
    assert rel <= 5e-3 and inv.last_plan['steps'] == [steps - 3] * 2 and inv.last_stats['rollbacks'] == [0, 0]
    assert inv.last_color.shape == (2, 12)
    assert dth <= r['band']


def test_rollback_restores_theta_and_its_moments(dev, fixture_result):
    """The noise maps scaled by 2^30 for one step (after step 5 of 10, checks every 5 steps): the guard flags the window, the run goes back
    to its last clean snapshot — (theta, its m, its v) with (w, m, v) — repeats it with exact scales and ends where the undisturbed run
    ends: the bars of tests/test_hip_align.py."""
    r = fixture_result
    eng, inv, x, w0, noises, steps = _fixture_run(r['g'], dev, check_every=5)
    seen = []

    def scale(run):
        if run.steps_run == 5 and not seen:
            seen.append(1)
            for n in run.noises:
                n.mul_(2.0 ** 30)
        elif run.steps_run == 6 and len(seen) == 1:
            seen.append(2)
            for n in run.noises:
                n.mul_(2.0 ** -30)
    inv.on_step = scale
    w, losses = inv.invert(x, w0, noises, steps=steps)
    rel = ((losses - r['losses']).abs() / r['losses']).max().item()
    dth = (inv.last_color - r['theta']).abs().max().item()
    print(f'noise maps x 2^30 for step 6 of {steps}: {inv.last_stats}; loss rel diff {rel:.2e} (bar 1e-3), |theta - undisturbed| {dth:.2e} (bar 1e-4)')
    assert seen == [1, 2] and inv.last_stats['rollbacks'] == [1]
    assert torch.isfinite(losses).all() and rel < 1e-3 and dth < 1e-4


def test_composition_and_refusals(dev, fixture_result):
    """The colour map beside the other options of the loop — latent_space 'w', layer_lr + delta_reg, the schedule, color_reg with a robust
    kind — every run finite, without a rollback, with a theta that moved; and what it does not go with, refused before anything is launched."""
    from oodgan import _lib
    from oodgan.engine import WPlusInverter
    r = fixture_result
    for ctor in (dict(latent_space='w'), dict(layer_lr=[1.0] * 5 + [0.5] * 5, delta_reg=0.1), dict(lr_rampup=0.05, lr_rampdown=0.25, latent_noise=0.05),
                 dict(color_reg=0.5, pixel_loss='geman_mcclure', kind='gain')):
        eng, inv, x, w0, noises, steps = _fixture_run(r['g'], dev, **ctor)
        w, losses = inv.invert(x, w0, noises, steps=6)
        print(f'{sorted(ctor)}: loss {losses[0].tolist()} -> {losses[-1].tolist()}, theta {inv.last_color.tolist()}')
        assert inv.last_stats == {'steps_run': [6], 'rollbacks': [0]} and inv.last_plan['steps'] == [3]
        assert torch.isfinite(losses).all() and torch.isfinite(w).all() and (inv.last_color[:, [0, 4, 8, 9, 10, 11]].cpu() != CR.identity(2)[:, [0, 4, 8, 9, 10, 11]]).all()
        assert (inv.last_terms['color'] is not None) == ('color_reg' in ctor)
        if 'color_reg' in ctor:
            assert torch.equal(losses, inv.last_terms['pixel'] + 0.5 * inv.last_terms['color']) and (inv.last_terms['color'][0] == 0).all()
    eng, inv, x, w0, noises, steps = _fixture_run(r['g'], dev)
    n0 = _lib.dispatch_count('color')
    with pytest.raises(NotImplementedError, match='use_graph'):
        inv.invert(x, w0, noises, steps=4, use_graph=True)
    with pytest.raises(NotImplementedError, match='pixel_target'):
        inv.invert(x, w0, noises, steps=4, pixel_target=torch.zeros(2, 3, 32, 32, device=dev))
    for ctor, what in ((dict(ssim_weight=0.5), 'SSIM'), (dict(pixel_size=32), 'pixel_size'), (dict(pixel_size=32, pixel_filter='bicubic'), 'pixel_size'),
                       (dict(latent_space='s'), 'latent_space'), (dict(feature_layer=5), 'feature_layer'), (dict(mask_size=16), 'loss_region'),
                       (dict(align='similarity'), 'align')):
        with pytest.raises(NotImplementedError, match=what):
            kw = dict(mask_logits=torch.zeros(2, 1, 16, 16, device=dev)) if 'mask_size' in ctor else {}
            WPlusInverter(eng, color='affine', **ctor).invert(x, w0, noises, steps=4, **kw)
    for init in (torch.zeros(3, 12, device=dev), torch.zeros(2, 12), torch.zeros(2, 12, device=dev, dtype=torch.float64),
                 torch.full((2, 12), NAN, device=dev), torch.zeros(2, 4, device=dev)):
        with pytest.raises(ValueError, match='color_init'):
            inv.invert(x, w0, noises, steps=4, color_init=init)
    with pytest.raises(ValueError, match='color_init'):
        WPlusInverter(eng).invert(x, w0, noises, steps=4, color_init=torch.zeros(2, 12, device=dev))
    assert _lib.dispatch_count('color') == n0


# ------------------------------------------------------------------------------------------------------------- model level
class _EncoderStub(torch.nn.Module):
    """The encoder stub of tests/test_hip_align.py: fixed latents, and the seeded feature pyramid scaled by the local brightness of the
    256² image it is shown."""

    def __init__(self, lats, feats):
        super().__init__()
        self.lats, self.feats = lats, feats

    def forward(self, x256, return_feats=False):
        lum = x256.mean(1, keepdim=True)
        feats = [f * (1.0 + 0.5 * F.interpolate(lum, size=f.shape[-2:], mode='bilinear', align_corners=False)) for f in self.feats]
        return (self.lats, feats) if return_feats else self.lats


def test_model_blends_the_mapped_image(dev):
    """256², the model with its modulation blocks and blend: the output of ``invert(color=)`` is blend(x, color_apply(G, theta)) bit for bit —
    the generator image mapped once, before the blend —, ``model(x, lats=, color=theta)`` replays it bit for bit, and
    ``color_apply(out, color_inverse(theta))`` is the blend of C^-1(x) with G to 1e-5 of the image range: an affine map commutes with the
    blend.  Without the option ``last_color`` is None."""
    from oodgan import _lib, ops
    from oodgan.arch import ood_faceGAN_e4e
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
    md.encoder = _EncoderStub(enc_lats, base).to(dev).eval()
    out, lats, losses = md.invert(x, steps=steps, color='affine', color_lr=0.004, color_reg=0.1, color_init=th0, loss_region='blend', noise=noise)
    th = md.last_color
    assert th.shape == (B, 12) and torch.isfinite(out).all() and (th != th0).all() and md.last_loss_terms['color'].shape == (steps, B)
    assert torch.equal(losses, md.last_loss_terms['pixel'] + 0.1 * md.last_loss_terms['color'])
    # the replay, and the output taken apart: G from the hooked pass, mapped once, then the blend
    again = md(x, lats=lats, noise=noise, color=th)[0]
    assert torch.equal(again, out)
    _, feats = md.encode(x)
    G = md._hooked_generate(lats, feats, noise)
    want = ops.color_apply(G.contiguous(), th)
    for _ in range(md.blend_cnt):
        want = md.blend(x, want)
    plain = md(x, lats=lats, noise=noise)[0]
    print(f'modulation model at {size}²: |out - blend(x, C(G))| {(out - want).abs().max().item():.1e}, |out - the output without the map| '
          f'{(out - plain).abs().max().item():.2e}')
    assert torch.equal(out, want) and not torch.equal(out, plain)
    # the colour-corrected picture: C^-1 of the output is the blend of C^-1(x) with G
    ti = ops.color_inverse(th)
    corrected = ops.color_apply(out, ti)
    other = G
    for _ in range(md.blend_cnt):
        other = md.blend(ops.color_apply(x, ti), other)
    rng = (other.max() - other.min()).item()
    e = (corrected - other).abs().max().item() / rng
    print(f'color_apply(out, color_inverse(theta)) against blend(C^-1(x), G): {e:.2e} of the image range {rng:.2f} (bar 1e-5)')
    assert e <= 1e-5
    # refusals before any device work, and the run without the option
    n0 = _lib.dispatch_count('color')
    with pytest.raises(ValueError, match='color'):
        md.invert(x, steps=steps, color='tone', noise=noise)
    with pytest.raises(NotImplementedError, match='SSIM'):
        md.invert(x, steps=steps, color='gain', ssim_weight=0.5, noise=noise)
    with pytest.raises(NotImplementedError, match='loss_region'):
        md.invert(x, steps=steps, color='gain', loss_region='fit', noise=noise)
    with pytest.raises(ValueError, match='color_init'):
        md.invert(x, steps=steps, color_init=th0, noise=noise)
    assert _lib.dispatch_count('color') == n0
    out0, _, _ = md.invert(x, steps=steps, noise=noise)
    assert md.last_color is None and md.last_loss_terms['color'] is None and _lib.dispatch_count('color') == n0
