"""StyleSpace inversion: ``invert(latent_space='s')`` fits an offset on the per-channel styles the modulated convs consume.

The two kernels against float64 (oodgan_style_affine_fwd_offset, oodgan_style_step) and bit for bit against the entries they extend
(oodgan_style_affine_fwd with a zero offset, oodgan_adam_step_dev_sched with every option off); the public layout of the style columns
against shifted modulation biases; dL/ds of the running loop — read back from
Adam's first moment as tests/wplus_grads.py does for dL/dW+ — against float64 autograd through the oracle (tests/sspace_ref.py), the first
direct pin of ``gs_all``; the loop against the reference's own autograd + Adam on offsets of its modulation biases
(tests/golden/wplus_sspace_256.npz); the model-level arguments."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import ref_cpu as R  # noqa: E402
from oodgan import synth  # noqa: E402
from oodgan.ops import lr_multiplier  # noqa: E402
import sspace_ref as SR  # noqa: E402
import wplus_grads as WG  # noqa: E402

U = 2.0 ** -24


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


def _i32(v, dev):
    return torch.tensor([v], dtype=torch.int32, device=dev)


def _grouped_rows(L, n, seed):
    """n row -> latent indices, random group sizes, ascending (rows grouped by latent, as the engine's are)."""
    g = torch.Generator().manual_seed(seed)
    return torch.sort(torch.randint(0, L, (n,), generator=g)).values.to(torch.int32)


# ------------------------------------------------------------------------------------------------------------- style affine + offset
@pytest.mark.parametrize('shape', [(1, 10, 512, 37 * 16), (3, 18, 512, 9088), (2, 4, 24, 40)], ids=['mfma-592', 'mfma-9088', 'scalar-40'])
def test_style_affine_offset_vs_float64(dev, shape):
    """s = scale W w + b + delta against float64.  Bar: a float32 dot product of S terms in any order, the bias and the offset added to it,
    is within (S + 3) 2^-24 of the sum of the absolute values of its terms.  With a zero offset the entry returns the existing entry's bits."""
    from oodgan import ops
    B, L, S, Rn = shape
    lat, w = synth.normal('ss.lat', (B, L, S), 1), synth.normal('ss.w', (Rn, S), 2)
    bias, off = synth.normal('ss.b', (Rn,), 3), synth.normal('ss.off', (B, Rn), 4, 0.3)
    rl = _grouped_rows(L, Rn, 5)
    if Rn % 16 == 0:
        rl = rl[(torch.arange(Rn) // 16) * 16].contiguous()         # the generator's case: every tile of 16 rows reads one latent
        rl[16:32] = torch.sort(torch.randint(0, L, (16,), generator=torch.Generator().manual_seed(6))).values.to(torch.int32)      # and one mixed tile
    scale = 1.0 / math.sqrt(S)
    latd, wd, bd, od, rld = lat.to(dev), w.to(dev), bias.to(dev), off.to(dev), rl.to(dev)
    got = ops.style_affine(latd, wd, bd, rld, offset=od)
    plain = ops.style_affine(latd, wd, bd, rld)
    zero = ops.style_affine(latd, wd, bd, rld, offset=torch.zeros_like(od))
    assert torch.equal(zero, plain)
    assert torch.equal(got, plain + od)                 # one more fp32 addition after the affine's own rounding
    terms = lat.double()[:, rl.long(), :] * w.double()[None]                    # (B, R, S)
    ref = terms.sum(-1) * scale + bias.double() + off.double()
    mag = terms.abs().sum(-1) * scale + bias.double().abs() + off.double().abs()
    ratio = ((got.double().cpu() - ref).abs() / ((S + 3) * U * mag)).max().item()
    print(f'style_affine_fwd_offset {shape}: max err / ((S + 3) 2^-24 sum|terms|) = {ratio:.3f} (bar 1)')
    assert ratio <= 1.0
    with pytest.raises(ValueError, match='offset'):
        ops.style_affine(latd, wd, bd, rld, offset=od[:, :-1].contiguous())
    from oodgan import _lib
    rc = _lib.lib().oodgan_style_affine_fwd_offset(ops._p(latd), ops._p(wd), ops._p(bd), ops._p(rld), None, ops._p(got), B, L, S, Rn, scale, 1.0,
                                                   ops._stream())
    assert rc == -1 and b'style_affine_fwd_offset' in _lib.lib().oodgan_last_error()


# ------------------------------------------------------------------------------------------------------------- the style step
_STEP = dict(total=8, up=0.05, down=0.25, lr=0.01, L=6)


def _step_rates():
    return [1.0, 0.5, 0.0, 1.5, 2.0, 0.25]         # one frozen latent


@pytest.mark.parametrize('grad_div', [1.0, 64.0])
@pytest.mark.parametrize('lam', [0.0, 0.5])
@pytest.mark.parametrize('shape', [(1, 37), (3, 1000), (8, 9088)])
def test_style_step_vs_float64(dev, shape, lam, grad_div):
    """Eight steps (ramps 0.05 / 0.25: t = 1 has step size 0, the middle full, the end on the cosine) against torch.optim.Adam in float64 with
    one parameter group per latent (lr * layer_lr) and lambda * mean delta^2 in the loss.  Every step is checked.  Bars, those of
    oodgan_latent_step for the same quantities (tests/test_hip_latent_controls.py — the same arithmetic): delta 1e-6 max(1, max|delta|),
    R 1e-6 relative, the g written back 1e-6 of its maximum.  Rows of a latent with factor 0 never move, their moments do."""
    from oodgan import ops
    B, Rn = shape
    total, up, down, lr, L = _STEP['total'], _STEP['up'], _STEP['down'], _STEP['lr'], _STEP['L']
    rates, rl = _step_rates(), _grouped_rows(_STEP['L'], Rn, 11)
    d0 = synth.normal('st.d', shape, 3, 0.1)
    groups = [(l, (rl == l).nonzero().flatten()) for l in range(L) if bool((rl == l).any())]
    leaves = [d0[:, idx].double().clone().requires_grad_(True) for _, idx in groups]
    opt = torch.optim.Adam([dict(params=[p]) for p in leaves], lr=lr, betas=(0.9, 0.999), eps=1e-8)

    def full():
        d = torch.zeros(shape, dtype=torch.float64)
        return torch.index_put(d, (torch.arange(B)[:, None], torch.cat([idx for _, idx in groups])[None]), torch.cat(leaves, 1))

    dd = d0.clone().to(dev)
    m, v, t = torch.zeros_like(dd), torch.zeros_like(dd), _i32(0, dev)
    rd, rld = torch.tensor(rates, dtype=torch.float32, device=dev), rl.to(dev)
    table = torch.full((total, B), -1.0, device=dev)
    frozen = torch.cat([idx for l, idx in groups if rates[l] == 0.0] or [torch.zeros(0, dtype=torch.long)])
    for i in range(total):
        gr = synth.normal(f'st.g{i}', shape, 4) * (10.0 ** (-(i % 3) - 1))
        for (l, _), grp in zip(groups, opt.param_groups):
            grp['lr'] = lr * lr_multiplier(i, total, up, down) * rates[l]
        opt.zero_grad(set_to_none=True)
        d = full()
        d.retain_grad()
        R_ref = (d ** 2).mean(dim=1)
        ((gr.double() * d).sum() + lam * R_ref.sum()).backward()
        g_ref = d.grad
        opt.step()
        gs = (gr * grad_div).to(dev)                     # a power of two: the division gives gr back exactly
        ops.style_step(dd, gs, m, v, t, total, up, down, lr, grad_div=grad_div, row_lat=rld, layer_lr=rd, style_reg=lam, table=table)
        d_ref = full().detach()
        e_d = (dd.double().cpu() - d_ref).abs().max().item() / max(1.0, d_ref.abs().max().item())
        e_g = (gs.double().cpu() - g_ref).abs().max().item() / g_ref.abs().max().item()
        e_R = ((table[i].double().cpu() - R_ref.detach()).abs() / R_ref.detach()).max().item()
        print(f'style step {shape} lambda {lam} grad_div {grad_div} step {i + 1}: delta err {e_d:.2e}, R rel err {e_R:.2e}, g err {e_g:.2e} of max (bars 1e-6)')
        assert e_d <= 1e-6 and e_R <= 1e-6 and e_g <= 1e-6
        assert int(t.item()) == i + 1
        if lam == 0.0:
            assert torch.equal(gs.cpu(), gr)             # gs / grad_div exactly, nothing added
        if len(frozen):
            assert torch.equal(dd[:, frozen.to(dev)].cpu(), d0[:, frozen]) and (m[:, frozen.to(dev)] != 0).any() and (v[:, frozen.to(dev)] != 0).any()
        if i == 0:                                      # r(0) = 0 with a ramp-up: the first step only fills the moments
            assert torch.equal(dd.cpu(), d0)
    assert (table >= 0).all() and not torch.equal(dd.cpu(), d0)


@pytest.mark.parametrize('shape', [(1, 37), (3, 1000), (8, 9088)])
def test_style_step_off_is_the_scheduled_adam(dev, shape):
    """The anchor: grad_div = 1, no factors, lambda = 0, no table -> delta, m, v, t bit for bit those of oodgan_adam_step_dev_sched on the same flat
    buffers, ramps on or off (both off: those of oodgan_adam_step_dev, tests/test_hip_wplus_sched.py); all factors 1.0 is the same."""
    from oodgan import ops
    total, up, down, lr = _STEP['total'], _STEP['up'], _STEP['down'], _STEP['lr']
    d0 = synth.normal('st.d', shape, 3, 0.1).to(dev)
    ones, rl = torch.ones(_STEP['L'], device=dev), _grouped_rows(_STEP['L'], shape[1], 11).to(dev)
    for ramps in ((up, down), (0.0, 0.0)):
        state = [[d0.clone(), torch.zeros_like(d0), torch.zeros_like(d0), _i32(0, dev)] for _ in range(3)]
        for i in range(total):
            gr = (synth.normal(f'st.g{i}', shape, 4) * (10.0 ** (-(i % 3) - 1))).to(dev)
            (wa, ma, va, ta), (wb, mb, vb, tb), (wc, mc, vc, tc) = state
            ops.adam_step_dev_sched(wa.view(-1), gr.view(-1), ma.view(-1), va.view(-1), ta, total, ramps[0], ramps[1], lr)
            gb, gc = gr.clone(), gr.clone()
            ops.style_step(wb, gb, mb, vb, tb, total, ramps[0], ramps[1], lr)
            ops.style_step(wc, gc, mc, vc, tc, total, ramps[0], ramps[1], lr, row_lat=rl, layer_lr=ones)
            for got in (state[1], state[2]):
                assert all(torch.equal(a, b) for a, b in zip(state[0], got)), (shape, ramps, i)
            assert torch.equal(gb, gr) and torch.equal(gc, gr)
        assert not torch.equal(state[0][0], d0)


def test_style_step_table_row_and_bad_arguments(dev):
    """The table form writes row t_dev[0] (before the increment, clamped to the table) and no other; ``loss_out`` receives the same values;
    bad arguments come back as a status code."""
    from oodgan import ops, _lib
    shape = (3, 1000)
    B = shape[0]
    d0, gr = synth.normal('st.d', shape, 3, 0.1).to(dev), synth.normal('st.g0', shape, 4).to(dev)
    want = (d0.double().cpu() ** 2).mean(dim=1)
    table = torch.full((4, B), -1.0, device=dev)
    first = None
    for row in (2, 9):
        d, t = d0.clone(), _i32(row, dev)
        ops.style_step(d, gr.clone(), torch.zeros_like(d), torch.zeros_like(d), t, 20, style_reg=0.5, table=table)
        assert int(t.item()) == row + 1
        got = table[min(row, 3)]
        assert ((got.double().cpu() - want).abs() / want).max().item() <= 1e-6
        first = got.clone() if first is None else first
        assert torch.equal(got, first)
    assert torch.equal(table[:2], torch.full((2, B), -1.0, device=dev))
    out = torch.full((B,), -1.0, device=dev)
    ops.style_step(d0.clone(), gr.clone(), torch.zeros_like(d0), torch.zeros_like(d0), _i32(5, dev), 20, loss_out=out)
    assert torch.equal(out, first)
    with pytest.raises(ValueError, match='style_step'):
        ops.style_step(d0[0], gr[0], d0[0], d0[0], _i32(0, dev), 20)
    z = torch.zeros_like(d0)
    rl, rates = _grouped_rows(4, shape[1], 11).to(dev), torch.ones(4, device=dev)
    with pytest.raises(ValueError, match='row_lat'):           # rates without the table that says which latent a row reads
        ops.style_step(d0.clone(), gr.clone(), z.clone(), z.clone(), _i32(0, dev), 20, layer_lr=rates)
    with pytest.raises(ValueError, match='layer_lr has 3 entries'):           # fewer rates than the latents the table names
        ops.style_step(d0.clone(), gr.clone(), z.clone(), z.clone(), _i32(0, dev), 20, row_lat=rl, layer_lr=rates[:3].contiguous())
    rc = _lib.lib().oodgan_style_step(ops._p(d0.clone()), ops._p(gr), ops._p(z), ops._p(z), B, shape[1], 0.01, 0.9, 0.999, 1e-8, ops._p(_i32(0, dev)), 20, 0.0,
                                      0.0, 1.0, None, ops._p(rates), 0.0, None, 0, ops._stream())
    assert rc == -1 and b'layer_lr without row_lat' in _lib.lib().oodgan_last_error()
    for kw in (dict(grad_div=0.0), dict(style_reg=-1.0)):
        with pytest.raises(RuntimeError, match='style_step'):
            ops.style_step(d0.clone(), gr.clone(), z.clone(), z.clone(), _i32(0, dev), 20, **kw)


# ------------------------------------------------------------------------------------------------------------- layout
_S64 = {}


def _state64():
    if not _S64:
        _S64['P'] = synth.generator_state(64, seed=5)
    return _S64['P']


def test_layout_is_the_modulation_bias(dev):
    """64², B = 1 (a bias is shared over the batch): for each entry of ``style_layout()``, the forward with an offset only on that slice
    against the forward of a generator whose ``<name>.conv.modulation.bias`` was shifted by the same vector.  The two differ only by where
    fp32 rounds b + delta.  Bar per entry: 4x the image difference of the same two variants in the oracle's fp32 (bias shifted / offset
    added after the affine)."""
    from oodgan.engine import GeneratorEngine
    from oodgan.modules import Generator
    size = 64
    P = _state64()
    lay = Generator(size, 512, 2).style_layout()
    eng = GeneratorEngine({k: v.to(dev) for k, v in P.items()}, size)
    assert eng.style_layout() == lay == SR.layout(P, size) and eng.R == SR.n_rows(P, size)
    w = synth.make_latents(size, 1, seed=14)
    noises = synth.make_noises(size, 1, seed=7)
    wd, nd = w.to(dev), [n.to(dev) for n in noises]
    base = eng.forward(wd, nd)
    assert torch.equal(eng.forward(wd, nd, style_offsets=torch.zeros(1, eng.R, device=dev)), base)
    fails = []
    for name, lat, row, n in lay:
        vec = synth.normal(f'lay.{name}', (n,), 21, 0.2)
        delta = torch.zeros(1, eng.R)
        delta[0, row:row + n] = vec
        got = eng.forward(wd, nd, style_offsets=delta.to(dev))
        Q = dict(P)
        Q[f'{name}.conv.modulation.bias'] = P[f'{name}.conv.modulation.bias'] + vec
        want = GeneratorEngine({k: v.to(dev) for k, v in Q.items()}, size).forward(wd, nd)
        with torch.no_grad():
            a = R.generator_forward(Q, w, noises, size)
            b = SR.forward_offset_after(P, size, w[0], delta[0], noises)
        yard = (a - b).abs().max().item()
        err = (got - want).abs().max().item()
        moved = (got - base).abs().max().item()
        print(f'layout {name} (latent {lat}, rows {row}..{row + n}): |offset - shifted bias| {err:.2e}, oracle fp32 twice {yard:.2e} (bar 4x), the offset moves the image by {moved:.2e}')
        assert moved > 1e-3
        if not err <= 4 * yard:
            fails.append((name, err, yard))
    assert not fails, fails


# ------------------------------------------------------------------------------------------------------------- dL/ds against float64
GRAD_CASES = {
    's64-b1': (64, 1, 1, (1, 2, 4)),
    's64-b3': (64, 3, 1, (1, 2, 4)),
    's256-b2-two-streams': (256, 2, 2, (1, 2, 4)),
    's1024-b1': (1024, 1, 1, (1, 2, 3)),          # the F-form level and the 8-wave routes
}
_GSTATE = {}


def _gstate(size):
    if size not in _GSTATE:
        P = synth.generator_state(size, seed=0)
        _GSTATE.clear()
        _GSTATE[size] = (P, {k: v.double() for k, v in P.items()})
    return _GSTATE[size]


# Points left out of the comparison with the plain float64 oracle, by name, as tests/test_hip_wplus_step_grads.py leaves out its LeakyReLU kinks.
# (case, image, step): 256², image 1, step 1 — seven pre-activations (one each in convs.2, .5, .7, .10, .11, two in convs.9) lie within 3.5e-7 of
# their layer's maximum, below what float32 resolves, and the float64 oracle takes the other LeakyReLU slope there than the kernels' forward:
# dL/ds 2.7e-4 of its maximum against the plain oracle, 1.1e-5 against the same oracle with those seven slopes as the kernels took them
# (measured).  The point stays in the given-slope check below.
KINK_POINTS = {('s256-b2-two-streams', 1, 1)}
# The given-slope check (step 1 of every image): the project's bars for these kernels' gradients (max|dg| / max|g| 1e-4 with three
# matrix instructions per product, 3e-4 with the back-propagated gradient rounded to f16) — the CPU's fp32 is NOT the yardstick there: without the
# slope effect it is at 1e-6, below what 22-bit split-f16 products reach
GIVEN_SLOPE_BAR = {'f16s': 1e-4, 'f16s-g2': 3e-4}
# elements of a forward that may change side: a pre-activation lies within 2^-20 of the layer maximum with probability ~4 * 2^-20 (a density of
# ~0.4 / sigma at zero, a maximum of ~5 sigma), and only those of them whose sign differs are taken; + 8 for the small layers
ADOPTED_MAX = lambda n_elements: 4 * SR.SLOPE_BAND * n_elements + 8


@pytest.mark.parametrize('prec', ['f16s-g2', 'f16s'])
@pytest.mark.parametrize('case', list(GRAD_CASES))
def test_style_gradient_vs_float64(dev, case, prec):
    """dL/ds of every checked step — recovered from Adam's first moment through ``on_step`` (tests/wplus_grads.py) — against the plain float64
    autograd of tests/sspace_ref.py at the same offsets, max-normalised per image.  Yardstick: the same gradient from the oracle run in fp32 on the
    CPU, the largest over the case's images and steps; bar: 4x that yardstick per case (DESIGN.md §5 records the W+ bars at about that ratio to the
    oracle's own fp32).  Asserted at every point but the one ``KINK_POINTS`` names.  No rollback.  Every point's figures are printed.

    At step 1 of every image, where the loop's forward is ``GeneratorEngine.forward`` at (w0, 0) bit for bit, a second check: the float64 reference
    takes the LeakyReLU slope of the pre-activations within 2^-20 of their layer's maximum (16 ulp of float32) from that forward and keeps its own
    everywhere else (``sspace_ref.given_slopes``).  Asserted: no slope OUTSIDE the band differs between the engine and float64; the number taken
    stays within ``ADOPTED_MAX``; dL/ds within ``GIVEN_SLOPE_BAR``.  The fp32 oracle under the same slopes is printed beside it.

    Measured on the MI355X (f16s-g2 / f16s).  Plain oracle, worst kept point against the bar: 64² B=1 4.0e-5 / 4.0e-5 (1.2e-4); 64² B=3 1.7e-4 / 1.7e-4
    (2.7e-4); 256² B=2 on two streams 5.5e-5 / 4.3e-5 (2.1e-4 / 3.8e-4), the named point 2.7e-4 / 2.7e-4; 1024² B=1 1.2e-4 / 1.2e-4 (4.3e-3).  The
    yardstick carries the same slope effect (the oracle's fp32 at 1024²: 4.7e-6 at step 1, 1.1e-3 at step 3), which is why the 1024² bar is wide; the
    given-slope check is the tight one there: step 1, all cases, 9.8e-7 ... 1.4e-5, 1 ... 22 slopes taken, none outside the band."""
    from oodgan.engine import GeneratorEngine, WPlusInverter
    size, B, streams, steps = GRAD_CASES[case]
    N = max(steps)
    P, P64 = _gstate(size)
    target, w0, noises = WG.recipe(size, list(range(B)))
    eng = GeneratorEngine({k: v.to(dev) for k, v in P.items()}, size, precision=prec)
    inv = WPlusInverter(eng, latent_space='s')
    cap = {}

    def on_step(run):
        i = next(n for n, r in enumerate(inv._runs) if r is run)
        cap.setdefault(i, {})[run.t] = (run.w.clone(), run.m.clone())

    inv.on_step = on_step
    delta, losses = inv.invert(target.to(dev), w0.to(dev), [n.to(dev) for n in noises], steps=N, streams=streams)
    torch.cuda.synchronize()
    print(f'[{case} {prec}] stats {inv.last_stats}, plan {inv.last_plan}')
    assert inv.last_stats == {'steps_run': [N] * streams, 'rollbacks': [0] * streams}, inv.last_stats
    assert delta.shape == (B, eng.R) and losses.shape == (N, B)
    cuts = [(i * B) // streams for i in range(streams + 1)]
    lay = SR.layout(P, size)
    styled = [nm for nm, _, _, _ in lay if not nm.startswith('to_rgb')]
    probe = eng.clone_shared()

    def engine_slopes(k):
        """The side of zero every pre-activation of the engine's forward at (w0[k], 0) lies on, per styled conv: the sign of its output."""
        probe.reset_fwd_state()
        probe.forward(w0[k:k + 1].to(dev), [n[k:k + 1].to(dev) for n in noises], save=True, style_offsets=torch.zeros(1, eng.R, device=dev))
        acts = [probe.saved['acts'][nm] for nm in styled]
        out = [((a.to_nchw() if hasattr(a, 'to_nchw') else a) > 0).cpu() for a in acts]
        probe.saved = None
        return out

    points, fails = [], []
    for k in range(B):
        i = next(n for n in range(streams) if cuts[n] <= k < cuts[n + 1])
        j = k - cuts[i]
        nz = [n[k:k + 1] for n in noises]
        for t in steps:
            zero = torch.zeros(eng.R)
            d_prev = zero if t == 1 else cap[i][t - 1][0][j].cpu()
            m_prev = zero if t == 1 else cap[i][t - 1][1][j].cpu()
            g = WG.recover_grad(m_prev, cap[i][t][1][j].cpu(), inv.betas[0])
            l64, _, _, g64 = SR.loss_and_grad(P64, size, w0[k], d_prev, target[k:k + 1], nz)
            _, _, _, g32 = SR.loss_and_grad(P, size, w0[k], d_prev, target[k:k + 1], nz)
            top = g64.abs().max().item()
            dg = (g - g64).abs()
            err, yard = dg.max().item() / top, (g32.double() - g64).abs().max().item() / top
            name = next(nm for nm, _, row, n in lay if row <= int(dg.argmax()) < row + n)
            e_loss = abs(float(losses[t - 1, k]) - l64) / l64
            kept = (case, k, t) not in KINK_POINTS
            print(f'[{case} {prec}] image {k} step {t}: dL/ds rel {err:.2e} (worst in {name}), the oracle in fp32 {yard:.2e}, loss rel {e_loss:.2e}'
                  + ('' if kept else '  [named in KINK_POINTS: not held to the bar]'))
            points.append((k, t, err, yard, kept))
            if not e_loss < 1e-5:
                fails.append(f'image {k} step {t}: loss {e_loss:.2e}')
            if t != 1:
                continue
            slopes = engine_slopes(k)
            with SR.given_slopes(slopes) as gs_:
                _, _, _, g64s = SR.loss_and_grad(P64, size, w0[k], d_prev, target[k:k + 1], nz)
            with SR.given_slopes(slopes):
                _, _, _, g32s = SR.loss_and_grad(P, size, w0[k], d_prev, target[k:k + 1], nz)
            e_s, y_s = (g - g64s).abs().max().item() / top, (g32s.double() - g64s).abs().max().item() / top
            n_el, taken, outside = sum(a.numel() for a in slopes), sum(gs_.adopted), sum(gs_.outside)
            print(f'[{case} {prec}] image {k} step 1, slopes within 2^-20 of the layer maximum as the engine took them: dL/ds rel {e_s:.2e} (bar '
                  f'{GIVEN_SLOPE_BAR[prec]:.0e}), the oracle in fp32 under the same slopes {y_s:.2e}; {taken} of {n_el} slopes taken (at most '
                  f'{ADOPTED_MAX(n_el):.0f}), {outside} differ outside the band')
            if outside != 0:
                fails.append(f'image {k} step 1: {outside} slopes of the engine differ from float64 outside the band')
            if not taken <= ADOPTED_MAX(n_el):
                fails.append(f'image {k} step 1: {taken} slopes taken > {ADOPTED_MAX(n_el):.0f}')
            if not e_s <= GIVEN_SLOPE_BAR[prec]:
                fails.append(f'image {k} step 1: given-slope dL/ds {e_s:.2e} > {GIVEN_SLOPE_BAR[prec]:.0e}')
    bar = 4 * max(y for _, _, _, y, _ in points)
    print(f'[{case} {prec}] yardstick of the case {bar / 4:.2e} -> bar {bar:.2e}; worst kept dL/ds {max(e for _, _, e, _, kept in points if kept):.2e}')
    fails += [f'image {k} step {t}: {e:.2e} > {bar:.2e}' for k, t, e, _, kept in points if kept and not e <= bar]
    assert not fails, f'[{case} {prec}] ' + '; '.join(fails)


# ------------------------------------------------------------------------------------------------------------- the loop
def _golden_inputs(g, dev, size=256, B=2):
    sw, sx, sn, s0 = [int(v) for v in g['seeds']]
    from oodgan.engine import GeneratorEngine
    eng = GeneratorEngine({k: v.to(dev) for k, v in synth.generator_state(size, seed=sw).items()}, size)
    return (eng, synth.make_images(size, B, seed=sx).to(dev), synth.make_latents(size, B, seed=s0, std=0.3).to(dev),
            [n.to(dev) for n in synth.make_noises(size, B, seed=sn)])


def test_loop_256_vs_reference(dev, golden):
    """20 steps at 256² against the reference's autograd + torch.optim.Adam on offsets of its modulation biases.  Loss curve and final loss:
    the 1e-3 bars of the W+ goldens.  Plan replay, Python-driven and ``return_trajectory`` runs agree bit for bit; two streams
    within 0.5 %; the launch count of an 's' step is at most that of the W+ step with the same terms."""
    from oodgan.engine import WPlusInverter
    g = golden('wplus_sspace_256.npz')
    steps = int(g['steps'])
    eng, x, w0, noises = _golden_inputs(g, dev)
    l32, l64 = g['losses_f32'].double(), g['losses_f64'].double()
    e_fix = ((l32 - l64).abs() / l64).max().item()
    inv = WPlusInverter(eng, latent_space='s', use_plan=True)
    d1, l1 = inv.invert(x, w0, noises, steps=steps)
    plan_s = dict(inv.last_plan)
    assert inv.last_stats == {'steps_run': [steps], 'rollbacks': [0]} and plan_s['steps'] == [steps - 3] and plan_s['launches'][0] > 0
    assert inv.last_terms['style'] is None and torch.equal(l1, inv.last_terms['mse'])
    e_curve = ((l1.double().cpu() - l32).abs() / l32).max().item()
    e_final = ((l1[-1].double().cpu() - l32[-1]).abs() / l32[-1]).max().item()
    e_c64 = ((l1.double().cpu() - l64).abs() / l64).max().item()
    print(f'20 steps 256² in S: loss curve rel {e_curve:.2e} vs the reference fp32 loop ({e_c64:.2e} vs its float64 twin), final {e_final:.2e} '
          f'(bars 1e-3); the reference fp32 vs float64: {e_fix:.2e}; loss {l1[0].tolist()} -> {l1[-1].tolist()}; plan {plan_s}')
    d_ref = g[f'delta_step{steps}_f32']
    frac = ((d1.cpu() - d_ref).abs() < 2e-3).float().mean().item()
    print(f'delta after step {steps}: {100 * frac:.3f}% within 2e-3 of the reference fp32 loop (max |delta| {d_ref.abs().max().item():.3e}, '
          f'its float64 twin: {100 * ((g[f"delta_step{steps}_f64"] - d_ref).abs() < 2e-3).float().mean().item():.3f}%)')
    assert e_curve < 1e-3 and e_final < 1e-3
    assert (l1[-1] < l1[0]).all()
    # run kinds
    inv2 = WPlusInverter(eng, latent_space='s', use_plan=False)
    d2, l2 = inv2.invert(x, w0, noises, steps=steps)
    assert inv2.last_plan['steps'] == [0] and torch.equal(d2, d1) and torch.equal(l2, l1)
    d3, l3, traj = inv.invert(x, w0, noises, steps=steps, return_trajectory=True)
    assert torch.equal(d3, d1) and torch.equal(l3, l1) and len(traj) == steps and torch.equal(traj[-1], d1) and traj[0].shape == d1.shape
    e1 = (traj[0].cpu() - g['delta_step1_f32']).abs().max().item()
    print(f'delta after step 1 vs the reference: max diff {e1:.2e} (Adam moves every coordinate by ~lr = 1e-2)')
    d4, l4 = inv.invert(x, w0, noises, steps=steps, streams=2)
    rel = ((l4 - l1).abs() / l1).max().item()
    print(f'two streams vs one: loss rel diff {rel:.2e} (bar 5e-3); plan {inv.last_plan}')
    assert rel <= 5e-3 and inv.last_plan['steps'] == [steps - 3] * 2 and d4.shape == d1.shape
    # the W+ step of the same loss: one launch more (the contraction of dL/ds with the modulation matrices)
    wp = WPlusInverter(eng, use_plan=True)
    wp.invert(x, w0, noises, steps=6)
    print(f"launches per recorded step: 's' {plan_s['launches']}, W+ {wp.last_plan['launches']}")
    assert 0 < plan_s['launches'][0] <= wp.last_plan['launches'][0]
    assert plan_s['launches'][0] == wp.last_plan['launches'][0] - 1


def test_loop_controls(dev):
    """style_reg, layer_lr and the lr ramps in 's' at 64², against the float64 loop of tests/sspace_ref.py: the loss curve within max(1e-3, 3x the
    helper's own fp32-vs-float64 distance) — the bar of the schedule's and the latent controls' loop tests —, the regulariser's table within
    1e-6 absolute, the rows of a frozen latent zero; what the engine refuses."""
    from oodgan.engine import GeneratorEngine, WPlusInverter
    size, B, steps, lam, lr, up, down = 64, 2, 12, 0.5, 0.01, 0.1, 0.3
    P = _state64()
    x, w0, noises = synth.make_images(size, B, seed=9), synth.make_latents(size, B, seed=14), synth.make_noises(size, B, seed=7)
    sched = lambda i: lr * lr_multiplier(i, steps, up, down)
    l64, r64, d64, _ = SR.invert({k: v.double() for k, v in P.items()}, size, w0.double(), x.double(), [n.double() for n in noises], steps, style_reg=lam,
                                 lr_of_step=sched)
    l32, _, _, _ = SR.invert(P, size, w0, x, noises, steps, style_reg=lam, lr_of_step=sched)
    e_self = ((l32 - l64).abs() / l64).max().item()
    eng = GeneratorEngine({k: v.to(dev) for k, v in P.items()}, size)
    xd, wd, nd = x.to(dev), w0.to(dev), [n.to(dev) for n in noises]
    inv = WPlusInverter(eng, lr=lr, latent_space='s', style_reg=lam, lr_rampup=up, lr_rampdown=down)
    d, losses = inv.invert(xd, wd, nd, steps=steps)
    t = inv.last_terms
    e_curve = ((losses.double().cpu() - l64).abs() / l64).max().item()
    e_reg = (t['style'].double().cpu() - r64).abs().max().item()
    print(f"12 steps 64² in S with style_reg {lam} and ramps: loss curve rel {e_curve:.2e} vs the float64 loop (its fp32 twin: {e_self:.2e}); "
          f"|style table - float64| {e_reg:.2e} (max {r64.max().item():.2e}); stats {inv.last_stats}, plan {inv.last_plan}")
    assert e_curve < max(1e-3, 3 * e_self) and e_reg < 1e-6
    assert t['style'].shape == (steps, B) and torch.equal(losses, t['mse'] + lam * t['style']) and (t['style'][0] == 0).all()
    assert inv.last_stats == {'steps_run': [steps], 'rollbacks': [0]} and inv.last_plan['steps'] == [steps - 3]
    # per-layer rates through row_lat: the rows of latents 4.. stay zero, the others move
    L = w0.shape[1]
    inv = WPlusInverter(eng, latent_space='s', layer_lr=[1.0] * 4 + [0.0] * (L - 4))
    d, _ = inv.invert(xd, wd, nd, steps=6)
    rl = eng.row_lat.long()
    assert (d[:, rl >= 4] == 0).all() and (d[:, rl < 4] != 0).any()
    with pytest.raises(ValueError, match='layer_lr'):
        WPlusInverter(eng, latent_space='s', layer_lr=[1.0] * (L + 1)).invert(xd, wd, nd, steps=2)
    with pytest.raises(NotImplementedError, match="latent_space 's'"):
        WPlusInverter(eng, latent_space='s').invert(xd, wd, nd, steps=2, use_graph=True)
    d, l = WPlusInverter(eng, latent_space='s').invert(xd, wd, nd, steps=0)
    assert d.shape == (B, eng.R) and (d == 0).all() and l.shape == (0, B)
    with pytest.raises(ValueError, match='wrt'):
        eng.backward(torch.zeros(B, 3, size, size, device=dev), wrt='w')


def test_backward_to_styles_is_the_latent_gradient_before_its_contraction(dev):
    """``backward(wrt='styles')`` returns gs_all undivided; contracting it with the modulation matrices gives ``backward()``'s dL/dW+ bits."""
    from oodgan import ops
    from oodgan.engine import GeneratorEngine
    size, B = 64, 2
    eng = GeneratorEngine({k: v.to(dev) for k, v in _state64().items()}, size)
    w = synth.make_latents(size, B, seed=14).to(dev)
    nz = [n.to(dev) for n in synth.make_noises(size, B, seed=7)]
    gimg = (synth.normal('ss.gimg', (B, 3, size, size), 8) * 64.0).to(dev)
    eng.forward(w, nz, save=True)
    g_lat = eng.backward(gimg, 64.0)
    eng.forward(w, nz, save=True)
    gs = eng.backward(gimg, 64.0, wrt='styles')
    assert gs.shape == (B, eng.R) and gs is eng.last_gs
    assert torch.equal(ops.style_affine_backward(gs, eng.wcat, eng.lat_start, eng.n_latent, grad_div=64.0), g_lat)


# ------------------------------------------------------------------------------------------------------------- model level
def test_model_invert_in_s_at_64(dev):
    import test_hip_wplus_sched as S
    size, B, steps = 64, 2, 6
    m = S._model_64(dev)
    x = synth.make_images(size, B, seed=44).to(dev)
    kw = dict(enc_lats=synth.make_latents(size, B, seed=42, std=0.3).to(dev), noise=[n.to(dev) for n in synth.make_noises(size, B, seed=45)])
    w0 = m.encode(x, **kw)[0]
    Rn = m.generator.engine().R
    out, lats, losses = m.invert(x, steps=steps, latent_space='s', style_reg=0.1, **kw)
    delta = m.last_style_offsets
    assert torch.equal(lats, w0) and torch.equal(m.last_refined_lats, w0)
    assert delta.shape == (B, Rn) and (delta != 0).any()
    t = m.last_loss_terms
    assert t['style'].shape == (steps, B) and torch.equal(losses, t['mse'] + 0.1 * t['style'])
    again = m(x, lats=lats, style_offsets=delta, **kw)[0]
    assert torch.equal(again, out)
    assert not torch.equal(m(x, lats=lats, **kw)[0], out)
    # the fit: monotone over the first three steps, the last below the first
    l = losses.cpu()
    print(f"model.invert(latent_space='s') at 64²: losses {l[:, 0].tolist()}")
    assert (l[1] < l[0]).all() and (l[2] < l[1]).all() and (l[-1] < l[0]).all()
    # an edit is a StyleSpace direction, added for the final forward only
    e = synth.normal('ss.edit', (Rn,), 46, 0.3).to(dev)
    out_e, lats_e, losses_e = m.invert(x, steps=steps, latent_space='s', style_reg=0.1, edit=e, **kw)
    assert torch.equal(losses_e, losses) and torch.equal(m.last_style_offsets, delta) and torch.equal(lats_e, w0)
    want = m(x, lats=w0, style_offsets=(delta + e).contiguous(), **kw)[0]
    assert torch.equal(out_e, want) and not torch.equal(out_e, out)
    for form in (e[None], e[None].expand(B, -1).contiguous()):
        assert torch.equal(m.invert(x, steps=steps, latent_space='s', style_reg=0.1, edit=form, **kw)[0], out_e)
    L = m.generator.n_latent
    for bad in (torch.zeros(L, 512, device=dev), torch.zeros(B, L, 512, device=dev), e.double(), e.cpu(), e[:-1].contiguous(), 1.0):
        with pytest.raises(ValueError, match='edit'):
            m.invert(x, steps=2, latent_space='s', edit=bad, **kw)
    # the other spaces leave no offsets behind
    m.invert(x, steps=2, **kw)
    assert m.last_style_offsets is None and m.last_loss_terms['style'] is None
    for bad, name in ((dict(latent_space='s', delta_reg=0.5), 'delta_reg'), (dict(latent_space='s', latent_noise=0.05), 'latent_noise'),
                      (dict(latent_space='s', latent_reg=0.5), 'latent_reg'), (dict(style_reg=0.1), 'style_reg'),
                      (dict(latent_space='w', style_reg=0.1), 'style_reg'), (dict(latent_space='s', style_reg=-1.0), 'style_reg')):
        with pytest.raises(ValueError, match=name):
            m.invert(x, steps=2, **bad, **kw)
    with pytest.raises(NotImplementedError):
        m.invert(x, steps=2, latent_space='s', use_graph=True, **kw)


def test_padded_generator_refuses_offsets(dev):
    from oodgan.engine import GeneratorEngine, WPlusInverter
    size, B = 256, 1                 # 256² / 0.1875: 96 ... 48, 24 channels (tests/test_hip_generator.py)
    P = synth.generator_state(size, seed=5, narrow=0.1875)
    eng = GeneratorEngine({k: v.to(dev) for k, v in P.items()}, size, narrow=0.1875)
    assert eng.padded
    w = synth.make_latents(size, B, seed=14).to(dev)
    nz = [n.to(dev) for n in synth.make_noises(size, B, seed=7)]
    with pytest.raises(NotImplementedError, match='zero-padded'):
        eng.forward(w, nz, style_offsets=torch.zeros(B, eng.R, device=dev))
    with pytest.raises(NotImplementedError, match='zero-padded'):
        WPlusInverter(eng, latent_space='s').invert(synth.make_images(size, B, seed=9).to(dev), w, nz, steps=2)
    with pytest.raises(NotImplementedError, match='zero-padded'):
        eng.style_layout()


def test_model_in_s_at_256_with_modulation(dev):
    """With the modulation blocks: the SAMM hooks keep reading w0, and the output is the model's own forward at (w0, delta), masks and blend
    included, bit for bit."""
    import test_hip_wplus_masked as M
    size, B, steps = 256, 2, 3
    m = M._ood_model(dev)
    x, kw = M._ood_inputs(dev, size, B)
    w0 = m.encode(x, **kw)[0]
    out, lats, losses = m.invert(x, steps=steps, latent_space='s', **kw)
    delta = m.last_style_offsets
    assert torch.equal(lats, w0) and (delta != 0).any() and torch.isfinite(out).all() and torch.isfinite(losses).all()
    assert torch.equal(m(x, lats=lats, style_offsets=delta, **kw)[0], out)
    assert not torch.equal(m(x, lats=lats, **kw)[0], out)
    e = synth.normal('ss.edit256', (delta.shape[1],), 47, 0.3).to(dev)
    out_e, _, l_e = m.invert(x, steps=steps, latent_space='s', edit=e, **kw)
    assert torch.equal(l_e, losses) and torch.equal(m.last_style_offsets, delta)
    assert torch.equal(out_e, m(x, lats=w0, style_offsets=(delta + e).contiguous(), **kw)[0])
