"""The feature offset of the W+ loop: ``invert(feature_layer=l)`` fits, beside the latents, an offset on the input of the styled
up-conv that reads latent l.

The two kernels against float64 and bit for bit against what they extend (oodgan_feature_add: one fp32 addition; oodgan_feature_step:
oodgan_adam_step_dev_sched with every option off); the engine's forward against the float64 helper (tests/fspace_ref.py); dL/ddelta and
dL/dW+ of the running loop — read back from Adam's first moments as tests/wplus_grads.py does — against float64 autograd through the oracle;
the loop against the reference's own autograd + Adam with a forward pre-hook on the up-conv (tests/golden/wplus_fspace.npz); the range
guard's rollback; the controls and refusals; the model-level arguments."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import ref_cpu as R  # noqa: E402,F401
from oodgan import synth  # noqa: E402
from oodgan.ops import lr_multiplier  # noqa: E402
import fspace_ref as FR  # noqa: E402
import wplus_grads as WG  # noqa: E402

SUB = (slice(None), slice(None, None, 16), slice(None, None, 2), slice(None, None, 2))


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


def _i32(v, dev):
    return torch.tensor([v], dtype=torch.int32, device=dev)


# ------------------------------------------------------------------------------------------------------------- y = x + delta
@pytest.mark.parametrize('shape', [(3, 512, 16, 16), (2, 512, 32, 32), (1, 512, 8, 8), (105,)], ids=['16', '32', '8', 'n105'])
def test_feature_add_is_one_fp32_addition(dev, shape):
    """Bit-equal to torch's x + d.  n = 105 takes the 16-byte lanes with a scalar tail of one element; the same 105 elements as a view that starts
    4 bytes into its buffer take the element-by-element kernel."""
    from oodgan import ops, _lib
    x, d = synth.normal('fa.x', shape, 1).to(dev), synth.normal('fa.d', shape, 2, 0.3).to(dev)
    want = x + d
    assert torch.equal(ops.feature_add(x, d), want)
    out = torch.full_like(x, -7.0)
    assert ops.feature_add(x, d, out=out) is out and torch.equal(out, want)
    if len(shape) == 1:
        n = shape[0]
        bx, bd, by = (torch.full((n + 5,), -7.0, device=dev) for _ in range(3))
        bx[1:n + 1], bd[1:n + 1] = x, d
        rc = _lib.lib().oodgan_feature_add(ops._p(bx[1:]), ops._p(bd[1:]), ops._p(by[1:]), n, ops._stream())
        assert rc == 0 and torch.equal(by[1:n + 1], want) and (by[0] == -7.0) and (by[n + 1:] == -7.0).all()     # nothing written outside
    with pytest.raises(ValueError, match='feature_add'):
        ops.feature_add(x, d.flatten()[:-1].contiguous())
    rc = _lib.lib().oodgan_feature_add(ops._p(x), None, ops._p(out), x.numel(), ops._stream())
    assert rc == -1 and b'feature_add' in _lib.lib().oodgan_last_error()


# ------------------------------------------------------------------------------------------------------------- the feature step
_STEP = dict(total=8, up=0.05, down=0.25, lr=0.01)


@pytest.mark.parametrize('B', [1, 3])
@pytest.mark.parametrize('n', [105, 512 * 8 * 8, 512 * 32 * 32])
def test_feature_step_vs_float64(dev, n, B):
    """Three consecutive steps from counter value 2 (ramps 0.05 / 0.25 of 8: on the ramp, then full) with lambda = 0.5 and grad_div = 64 against
    torch.optim.Adam in float64 with lambda * mean delta^2 in the loss.  Bars, those of oodgan_style_step for the same quantities
    (tests/test_hip_sspace.py — the same arithmetic): delta 1e-6 max(1, max|delta|), R 1e-6 relative, the g written back 1e-6 of its maximum.
    The call leaves the counter alone (the latent-side call of a step increments it: here the test does).  n = 105: one partial block, the
    element-by-element kernel; 512*8*8: 8 blocks per image; 512*32*32: 128."""
    from oodgan import ops
    total, up, down, lr = _STEP['total'], _STEP['up'], _STEP['down'], _STEP['lr']
    lam, grad_div, t0 = 0.5, 64.0, 2
    shape = (B, n)
    d0 = synth.normal('fs.d', shape, 3, 0.1)
    leaf = d0.double().clone().requires_grad_(True)
    opt = torch.optim.Adam([leaf], lr=lr, betas=(0.9, 0.999), eps=1e-8)
    # the reference's Adam counts its own steps from 1: bring its bias corrections to t0 by t0 steps of zero gradient (moments stay zero)
    for _ in range(t0):
        leaf.grad = torch.zeros_like(leaf)
        opt.param_groups[0]['lr'] = 0.0
        opt.step()
    dd = d0.clone().to(dev)
    m, v, t = torch.zeros_like(dd), torch.zeros_like(dd), _i32(t0, dev)
    table = torch.full((total, B), -1.0, device=dev)
    part = ops.feature_step_parts(B, n, dev)
    for i in range(t0, t0 + 3):
        gr = synth.normal(f'fs.g{i}', shape, 4) * (10.0 ** (-(i % 3) - 1))
        opt.param_groups[0]['lr'] = lr * lr_multiplier(i, total, up, down)
        opt.zero_grad(set_to_none=True)
        R_ref = (leaf ** 2).mean(dim=1)
        ((gr.double() * leaf).sum() + lam * R_ref.sum()).backward()
        g_ref = leaf.grad.clone()
        opt.step()
        gs = (gr * grad_div).to(dev)                     # a power of two: the division gives gr back exactly
        ops.feature_step(dd, gs, m, v, t, total, up, down, lr, grad_div=grad_div, feature_reg=lam, table=table, part=part)
        assert int(t.item()) == i                        # read, not incremented
        t += 1
        d_ref = leaf.detach()
        e_d = (dd.double().cpu() - d_ref).abs().max().item() / max(1.0, d_ref.abs().max().item())
        e_g = (gs.double().cpu() - g_ref).abs().max().item() / g_ref.abs().max().item()
        e_R = ((table[i].double().cpu() - R_ref.detach()).abs() / R_ref.detach()).max().item()
        print(f'feature step n {n} B {B} step {i + 1}: delta err {e_d:.2e}, R rel err {e_R:.2e}, g err {e_g:.2e} of max (bars 1e-6)')
        assert e_d <= 1e-6 and e_R <= 1e-6 and e_g <= 1e-6
    assert (table[t0:t0 + 3] >= 0).all() and (table[:t0] == -1).all() and (table[t0 + 3:] == -1).all()
    assert not torch.equal(dd.cpu(), d0)


@pytest.mark.parametrize('shape', [(1, 105), (3, 512 * 8 * 8), (2, 512 * 32 * 32)])
def test_feature_step_off_is_the_scheduled_adam(dev, shape):
    """The anchor: grad_div = 1, lambda = 0, no table -> delta, m, v bit for bit those of oodgan_adam_step_dev_sched run on the same buffers from the
    same counter value, ramps on or off; g comes back unchanged.  Two calls on equal inputs give equal bits, with the table as well."""
    from oodgan import ops
    total, up, down, lr = _STEP['total'], _STEP['up'], _STEP['down'], _STEP['lr']
    d0 = synth.normal('fs.d', shape, 3, 0.1).to(dev)
    for ramps in ((up, down), (0.0, 0.0)):
        a = [d0.clone(), torch.zeros_like(d0), torch.zeros_like(d0), _i32(0, dev)]
        b = [d0.clone(), torch.zeros_like(d0), torch.zeros_like(d0), _i32(0, dev)]
        for i in range(4):
            gr = (synth.normal(f'fs.g{i}', shape, 4) * (10.0 ** (-(i % 3) - 1))).to(dev)
            gb = gr.clone()
            ops.feature_step(b[0], gb, b[1], b[2], b[3], total, ramps[0], ramps[1], lr)         # counter i -> uses t = i + 1
            ops.adam_step_dev_sched(a[0].view(-1), gr.view(-1), a[1].view(-1), a[2].view(-1), a[3], total, ramps[0], ramps[1], lr)      # i -> i + 1
            assert int(b[3].item()) == i
            b[3] += 1
            assert all(torch.equal(p, q) for p, q in zip(a, b)), (shape, ramps, i)
            assert torch.equal(gb, gr)
        assert not torch.equal(a[0], d0)
    B = shape[0]
    outs = []
    for _ in range(2):
        d, g = d0.clone(), (synth.normal('fs.g0', shape, 4) * 64.0).to(dev)
        m, v, table = torch.zeros_like(d), torch.zeros_like(d), torch.zeros(3, B, device=dev)
        ops.feature_step(d, g, m, v, _i32(1, dev), total, up, down, lr, grad_div=64.0, feature_reg=0.5, table=table)
        outs.append((d, g, m, v, table))
    assert all(torch.equal(p, q) for p, q in zip(*outs))


def test_feature_step_table_row_and_bad_arguments(dev):
    """The table form writes row t_dev[0] = t - 1, clamped to the table, and no other; ``loss_out`` receives the same values; bad arguments come
    back as a status code with the entry's name."""
    from oodgan import ops, _lib
    shape = (3, 4096 + 105)
    B = shape[0]
    d0, gr = synth.normal('fs.d', shape, 3, 0.1).to(dev), synth.normal('fs.g0', shape, 4).to(dev)
    want = (d0.double().cpu() ** 2).mean(dim=1)
    table = torch.full((4, B), -1.0, device=dev)
    first = None
    for row in (2, 9):
        d, t = d0.clone(), _i32(row, dev)
        ops.feature_step(d, gr.clone(), torch.zeros_like(d), torch.zeros_like(d), t, 20, feature_reg=0.5, table=table)
        assert int(t.item()) == row
        got = table[min(row, 3)]
        assert ((got.double().cpu() - want).abs() / want).max().item() <= 1e-6
        first = got.clone() if first is None else first
        assert torch.equal(got, first)
    assert torch.equal(table[:2], torch.full((2, B), -1.0, device=dev))
    out = torch.full((B,), -1.0, device=dev)
    ops.feature_step(d0.clone(), gr.clone(), torch.zeros_like(d0), torch.zeros_like(d0), _i32(5, dev), 20, loss_out=out)
    assert torch.equal(out, first)
    z = torch.zeros_like(d0)
    L = _lib.lib()
    args = lambda delta, tab, part: (delta, ops._p(gr), ops._p(z), ops._p(z), B, shape[1], 0.01, 0.9, 0.999, 1e-8, ops._p(_i32(0, dev)), 20, 0.0, 0.0, 1.0,
                                     0.0, tab, 4 if tab is not None else 0, part, ops._stream())
    assert L.oodgan_feature_step(*args(None, None, None)) == -1 and b'feature_step' in L.oodgan_last_error()
    assert L.oodgan_feature_step(*args(ops._p(d0.clone()), ops._p(table), None)) == -1 and b'reg_table without part' in L.oodgan_last_error()
    assert L.oodgan_feature_step_nparts(0) == 0 and L.oodgan_feature_step_nparts(105) == 1 and L.oodgan_feature_step_nparts(512 * 32 * 32) == 128
    for kw in (dict(grad_div=0.0), dict(feature_reg=-1.0)):
        with pytest.raises(RuntimeError, match='feature_step'):
            ops.feature_step(d0.clone(), gr.clone(), z.clone(), z.clone(), _i32(0, dev), 20, **kw)


# ------------------------------------------------------------------------------------------------------------- forward
_STATE = {}


def _state(size, seed=0):
    if (size, seed) not in _STATE:
        P = synth.generator_state(size, seed=seed)
        _STATE.clear()
        _STATE[(size, seed)] = (P, {k: v.double() for k, v in P.items()})
    return _STATE[(size, seed)]


@pytest.mark.parametrize('l', [3, 5, 7])
def test_forward_with_offset_at_64(dev, l):
    """64², B = 2, a random offset of std 0.3: a zero offset is the plain forward bit for bit; the engine against the float64 helper within the
    project's forward bar (1e-3 absolute); the offset moves the image by more than that; ``forward(save=True)`` keeps both the
    offset input and the un-offset activation; a wrong shape or layer raises ValueError."""
    from oodgan.engine import GeneratorEngine
    size, B = 64, 2
    P, P64 = _state(size, 5)
    eng = GeneratorEngine({k: v.to(dev) for k, v in P.items()}, size)
    w, noises = synth.make_latents(size, B, seed=14), synth.make_noises(size, B, seed=7)
    wd, nd = w.to(dev), [n.to(dev) for n in noises]
    shape = (B,) + FR.feature_shape(P, l)
    assert eng.feature_shape(l) == shape[1:] == (512, 4 << ((l - 1) // 2), 4 << ((l - 1) // 2))
    delta = synth.normal(f'ff.d{l}', shape, 21, 0.3)
    base = eng.forward(wd, nd)
    assert torch.equal(eng.forward(wd, nd, feature_offset=(l, torch.zeros(shape, device=dev))), base)
    got = eng.forward(wd, nd, feature_offset=(l, delta.to(dev)))
    with torch.no_grad():
        want = FR.forward(P64, size, w.double(), l, delta.double(), [n.double() for n in noises])
    err, moved = (got.double().cpu() - want).abs().max().item(), (got - base).abs().max().item()
    print(f'forward 64² with an offset on latent {l} {shape}: |engine - float64| {err:.2e} (bar 1e-3), the offset moves the image by {moved:.2e}')
    assert err < 1e-3 and moved > 1e-3
    saved = eng.forward(wd, nd, save=True, feature_offset=(l, delta.to(dev)))
    sv = eng.saved
    assert torch.equal(saved, got) and sv['f_lat'] == l
    assert torch.equal(sv['f_in'], sv['acts'][f'convs.{l - 2}'] + delta.to(dev))        # x' beside the un-offset x under its own name
    eng.saved = None
    for bad in ((l, delta[:, :-1].contiguous().to(dev)), (l + 1, delta.to(dev)), (9, delta.to(dev))):
        with pytest.raises(ValueError, match='feature'):
            eng.forward(wd, nd, feature_offset=bad)


# ------------------------------------------------------------------------------------------------------------- gradients in the running loop
GRAD_CASES = {
    's64-b1-l3': (64, 1, 1, 3, 'f16s'), 's64-b1-l5': (64, 1, 1, 5, 'f16s'), 's64-b1-l7': (64, 1, 1, 7, 'f16s'),
    's64-b3-l3': (64, 3, 1, 3, 'f16s'), 's64-b3-l5': (64, 3, 1, 5, 'f16s'), 's64-b3-l7': (64, 3, 1, 7, 'f16s'),
    's64-b1-l5-g2': (64, 1, 1, 5, 'f16s-g2'),
    's256-b2-two-streams-l5': (256, 2, 2, 5, 'f16s'),
}
GRAD_STEPS, GRAD_RUN = (1, 2, 4), 5        # the exact step, the carried Python step, a replayed step (step 3 of 5 is the recorded one)
# Points left out of the comparison with the plain float64 oracle, by name, as tests/test_hip_sspace.py leaves out its LeakyReLU kinks: (case,
# image, step) -> the measured reason.  At most one per case, never step 1's given-slope check.
KINK_POINTS = {
    # a few pre-activations (three at 64²) of image 1's first forward lie within 2^-20 of their layer's maximum and the kernels' float32 puts them on the other side
    # of zero than float64: the offset's gradient is a map, not a contraction over one, and one slope moves a 3x3 patch of it in every channel
    ('s64-b3-l3', 1, 1): 'dL/ddelta 1.1e-3 against the plain oracle, 9.3e-7 with those three slopes as the kernels took them',
    ('s64-b3-l5', 1, 1): 'dL/ddelta 6.1e-3 against the plain oracle, 1.9e-6 with those three slopes as the kernels took them',
    ('s256-b2-two-streams-l5', 1, 1): 'dL/ddelta 6.2e-3 against the plain oracle, 1.9e-6 with the eight slopes of its band as the kernels took them',
}
GIVEN_SLOPE_BAR = {'f16s': 1e-4, 'f16s-g2': 3e-4}          # DESIGN.md §5, as tests/test_hip_sspace.py
ADOPTED_MAX = lambda n_elements: 4 * FR.SLOPE_BAND * n_elements + 8


@pytest.mark.parametrize('case', list(GRAD_CASES))
def test_gradients_vs_float64(dev, case):
    """dL/ddelta and dL/dW+ of steps 1, 2 and 4 — recovered from Adam's first moments of the offset and of the latents through ``on_step`` —
    against the plain float64 autograd of tests/fspace_ref.py at the same (w, delta), max-normalised per image.  Yardstick: the same gradients
    from the helper run in fp32 on the CPU; bar: 4x the case's largest yardstick over its points and quantities (the ratio of the existing
    gradient tests; each quantity's own largest yardstick is printed beside it).  Row l of dL/dW+ — the style-gradient dot of the offset layer,
    which must read x' and not x: from step 2 on, with delta ~ lr, reading x puts ~1e-2 into it — is held to the bar on its own, normalised by
    its own maximum.  No rollback.  Every point's figures are printed.

    At step 1, where the loop's forward is ``GeneratorEngine.forward`` at (w0, 0) bit for bit, the given-slope check of tests/test_hip_sspace.py:
    float64 takes the LeakyReLU side of the pre-activations within 2^-20 of their layer's maximum from that forward; no slope outside the band
    may differ, the number taken stays within ``ADOPTED_MAX``, both gradients within ``GIVEN_SLOPE_BAR``."""
    from oodgan.engine import GeneratorEngine, WPlusInverter
    size, B, streams, l, prec = GRAD_CASES[case]
    N = GRAD_RUN
    P, P64 = _state(size, 0)
    target, w0, noises = WG.recipe(size, list(range(B)))
    eng = GeneratorEngine({k: v.to(dev) for k, v in P.items()}, size, precision=prec)
    inv = WPlusInverter(eng, feature_layer=l)
    cap, slopes_of = {}, {}
    styled = ['conv1'] + [f'convs.{j}' for j in range(2 * (eng.log_size - 2))]

    def on_step(run):
        i = next(n for n, r in enumerate(inv._runs) if r is run)
        cap.setdefault(i, {})[run.t] = (run.w.clone(), run.m.clone(), run.f.clone(), run.fm.clone())
        if run.t == 1:
            # the side of zero every pre-activation of the loop's own first forward lies on, per styled conv: the sign of its saved output.  Taken
            # from the run itself — a second forward of the same inputs need not choose the same kernels (the loop on two streams lowers the
            # 8-wave kernel's threshold, engine.MULTI_STREAM_S1_BIG_MIN_ITEMS) and a sum that float32 cannot tell from 0 may then take the other sign
            acts = [run.eng.saved['acts'][nm] for nm in styled]
            slopes_of[i] = [((a.to_nchw() if hasattr(a, 'to_nchw') else a) > 0).cpu() for a in acts]

    inv.on_step = on_step
    w, losses = inv.invert(target.to(dev), w0.to(dev), [n.to(dev) for n in noises], steps=N, streams=streams)
    torch.cuda.synchronize()
    print(f'[{case}] stats {inv.last_stats}, plan {inv.last_plan}')
    assert inv.last_stats == {'steps_run': [N] * streams, 'rollbacks': [0] * streams}, inv.last_stats
    assert inv.last_plan['steps'] == [N - 3] * streams
    fshape = FR.feature_shape(P, l)
    assert inv.last_feature_offset.shape == (B,) + fshape and losses.shape == (N, B)
    cuts = [(i * B) // streams for i in range(streams + 1)]
    points, fails = [], []
    for k in range(B):
        i = next(n for n in range(streams) if cuts[n] <= k < cuts[n + 1])
        j = k - cuts[i]
        nz = [n[k:k + 1] for n in noises]
        for t in GRAD_STEPS:
            if t == 1:
                w_prev, m_prev, d_prev, fm_prev = w0[k], torch.zeros_like(w0[k]), torch.zeros(fshape), torch.zeros(fshape)
            else:
                w_prev, m_prev, d_prev, fm_prev = (c[j].cpu() for c in cap[i][t - 1])
            gw = WG.recover_grad(m_prev, cap[i][t][1][j].cpu(), inv.betas[0])
            gd = WG.recover_grad(fm_prev, cap[i][t][3][j].cpu(), inv.betas[0])
            l64, _, _, gw64, gd64 = FR.loss_and_grad(P64, size, w_prev, l, d_prev, target[k:k + 1], nz)
            _, _, _, gw32, gd32 = FR.loss_and_grad(P, size, w_prev, l, d_prev, target[k:k + 1], nz)
            tw, td, tl = gw64.abs().max().item(), gd64.abs().max().item(), gw64[l].abs().max().item()
            e_w, y_w = (gw - gw64).abs().max().item() / tw, (gw32.double() - gw64).abs().max().item() / tw
            e_d, y_d = (gd - gd64).abs().max().item() / td, (gd32.double() - gd64).abs().max().item() / td
            e_l, y_l = (gw[l] - gw64[l]).abs().max().item() / tl, (gw32[l].double() - gw64[l]).abs().max().item() / tl
            e_loss = abs(float(losses[t - 1, k]) - l64) / l64
            kept = (case, k, t) not in KINK_POINTS
            print(f'[{case}] image {k} step {t}: dL/ddelta rel {e_d:.2e} (fp32 oracle {y_d:.2e}), dL/dW+ rel {e_w:.2e} ({y_w:.2e}), its row {l} {e_l:.2e} '
                  f'({y_l:.2e}), loss rel {e_loss:.2e}' + ('' if kept else '  [named in KINK_POINTS: not held to the bar]'))
            points.append((k, t, (e_d, e_w, e_l), (y_d, y_w, y_l), kept))
            if not e_loss < 1e-5:
                fails.append(f'image {k} step {t}: loss {e_loss:.2e}')
            if t != 1:
                continue
            slopes = [s[j:j + 1] for s in slopes_of[i]]
            with FR.given_slopes(slopes) as gs_:
                _, _, _, gw64s, gd64s = FR.loss_and_grad(P64, size, w_prev, l, d_prev, target[k:k + 1], nz)
            es_w, es_d = (gw - gw64s).abs().max().item() / tw, (gd - gd64s).abs().max().item() / td
            es_l = (gw[l] - gw64s[l]).abs().max().item() / tl
            n_el, taken, outside = sum(a.numel() for a in slopes), sum(gs_.adopted), sum(gs_.outside)
            print(f'[{case}] image {k} step 1, slopes within 2^-20 of the layer maximum as the engine took them: dL/ddelta rel {es_d:.2e}, dL/dW+ rel '
                  f'{es_w:.2e}, its row {l} {es_l:.2e} (bar {GIVEN_SLOPE_BAR[prec]:.0e}); {taken} of {n_el} slopes taken (at most {ADOPTED_MAX(n_el):.0f}), '
                  f'{outside} differ outside the band')
            if outside != 0:
                fails.append(f'image {k} step 1: {outside} slopes of the engine differ from float64 outside the band')
            if not taken <= ADOPTED_MAX(n_el):
                fails.append(f'image {k} step 1: {taken} slopes taken > {ADOPTED_MAX(n_el):.0f}')
            for nm, e in (('dL/ddelta', es_d), ('dL/dW+', es_w), (f'row {l} of dL/dW+', es_l)):
                if not e <= GIVEN_SLOPE_BAR[prec]:
                    fails.append(f'image {k} step 1: given-slope {nm} {e:.2e} > {GIVEN_SLOPE_BAR[prec]:.0e}')
    bar = 4 * max(max(y) for _, _, _, y, _ in points)
    for idx, nm in enumerate(('dL/ddelta', 'dL/dW+', f'row {l} of dL/dW+')):
        print(f'[{case}] {nm}: its own largest yardstick {max(y[idx] for _, _, _, y, _ in points):.2e}; worst kept {max(e[idx] for _, _, e, _, kept in points if kept):.2e} '
              f'(bar of the case {bar:.2e})')
        fails += [f'image {k} step {t}: {nm} {e[idx]:.2e} > {bar:.2e}' for k, t, e, _, kept in points if kept and not e[idx] <= bar]
    assert not fails, f'[{case}] ' + '; '.join(fails)


# ------------------------------------------------------------------------------------------------------------- the loop
def _golden_inputs(g, name, dev):
    size, l, steps = [int(v) for v in g[f'{name}_meta']]
    sw, sx, sn, s0 = [int(v) for v in g['seeds']]
    from oodgan.engine import GeneratorEngine
    eng = GeneratorEngine({k: v.to(dev) for k, v in synth.generator_state(size, seed=sw).items()}, size)
    return (eng, l, steps, synth.make_images(size, 2, seed=sx).to(dev), synth.make_latents(size, 2, seed=s0, std=0.3).to(dev),
            [n.to(dev) for n in synth.make_noises(size, 2, seed=sn)])


# launches a recorded step gains with the offset on: the addition, the feature step's kernel, and what the offset layer's
# stride-2 input-gradient conv no longer does in its epilogue — stated per case there
LAUNCH_DELTA = {'s256_l5': 2, 's64_l3': 2, 's64_l7': 2}


@pytest.mark.parametrize('name', ['s256_l5', 's64_l3', 's64_l7'])
def test_loop_vs_reference(dev, golden, name):
    """The loop against the reference's autograd + torch.optim.Adam on (w, delta).  Loss curve and final loss within 1e-3 relative of the
    reference's fp32 loop, the bar of the W+ goldens.  w and the offset's subsample: printed beside the golden's own fp32 / float64
    distance, asserted only as >= 99 % of the elements within 2 * lr * steps / 10 (the reference's two precisions meet that:
    tests/test_fspace_cpu.py).  Plan replay, Python-driven and ``return_trajectory`` runs agree bit for bit; two streams within 5e-3 on the
    loss; no rollback; the launch count of a recorded step is the W+ step's plus the constant of DESIGN.md §21."""
    from oodgan.engine import WPlusInverter
    g = golden('wplus_fspace.npz')
    eng, l, steps, x, w0, noises = _golden_inputs(g, name, dev)
    l32, l64 = g[f'{name}_losses_f32'].double(), g[f'{name}_losses_f64'].double()
    e_fix = ((l32 - l64).abs() / l64).max().item()
    inv = WPlusInverter(eng, feature_layer=l, use_plan=True)
    w1, l1 = inv.invert(x, w0, noises, steps=steps)
    d1, plan_f = inv.last_feature_offset, dict(inv.last_plan)
    assert inv.last_stats == {'steps_run': [steps], 'rollbacks': [0]} and plan_f['steps'] == [steps - 3] and plan_f['launches'][0] > 0
    assert inv.last_terms['feature'] is None and torch.equal(l1, inv.last_terms['mse'])
    e_curve = ((l1.double().cpu() - l32).abs() / l32).max().item()
    e_final = ((l1[-1].double().cpu() - l32[-1]).abs() / l32[-1]).max().item()
    e_c64 = ((l1.double().cpu() - l64).abs() / l64).max().item()
    print(f'{name}: {steps} steps: loss curve rel {e_curve:.2e} vs the reference fp32 loop ({e_c64:.2e} vs its float64 twin), final {e_final:.2e} (bars '
          f'1e-3); the reference fp32 vs float64: {e_fix:.2e}; loss {l1[0].tolist()} -> {l1[-1].tolist()}; plan {plan_f}')
    tol = 2 * 0.01 * steps / 10
    w_ref, w_r64 = g[f'{name}_w_step{steps}_f32'], g[f'{name}_w_step{steps}_f64']
    s_ref, s_r64 = g[f'{name}_delta_sub_f32'], g[f'{name}_delta_sub_f64']
    fw, fd = ((w1.cpu() - w_ref).abs() < tol).float().mean().item(), ((d1.cpu()[SUB] - s_ref).abs() < tol).float().mean().item()
    nrm = d1.double().flatten(1).norm(dim=1).cpu()
    print(f'{name}: w within {tol:.3f} of the reference fp32 loop: {100 * fw:.3f} % (max diff {(w1.cpu() - w_ref).abs().max().item():.2e}; its float64 '
          f'twin {(w_r64 - w_ref).abs().max().item():.2e}); offset subsample {100 * fd:.3f} % (max diff {(d1.cpu()[SUB] - s_ref).abs().max().item():.2e}; '
          f'twin {(s_r64 - s_ref).abs().max().item():.2e}); ||delta|| {nrm.tolist()} vs {g[f"{name}_delta_norm_f32"][-1].tolist()}')
    assert e_curve < 1e-3 and e_final < 1e-3
    assert fw >= 0.99 and fd >= 0.99
    assert (l1[-1] < l1[0]).all()
    # run kinds
    inv2 = WPlusInverter(eng, feature_layer=l, use_plan=False)
    w2, l2 = inv2.invert(x, w0, noises, steps=steps)
    assert inv2.last_plan['steps'] == [0] and torch.equal(w2, w1) and torch.equal(l2, l1) and torch.equal(inv2.last_feature_offset, d1)
    w3, l3, traj = inv.invert(x, w0, noises, steps=steps, return_trajectory=True)
    assert torch.equal(w3, w1) and torch.equal(l3, l1) and torch.equal(inv.last_feature_offset, d1)
    assert len(traj) == steps and torch.equal(traj[-1], w1) and traj[0].shape == w1.shape           # the trajectory stays the latents'
    w4, l4 = inv.invert(x, w0, noises, steps=steps, streams=2)
    rel = ((l4 - l1).abs() / l1).max().item()
    print(f'{name}: two streams vs one: loss rel diff {rel:.2e} (bar 5e-3); plan {inv.last_plan}')
    assert rel <= 5e-3 and inv.last_plan['steps'] == [steps - 3] * 2 and inv.last_feature_offset.shape == d1.shape
    assert inv.last_stats['rollbacks'] == [0, 0]
    # against the W+ step of the same loss
    wp = WPlusInverter(eng, use_plan=True)
    wp.invert(x, w0, noises, steps=6)
    assert wp.last_feature_offset is None and wp.last_terms['feature'] is None
    print(f"{name}: launches per recorded step: with the offset {plan_f['launches']}, W+ {wp.last_plan['launches']}")
    assert plan_f['launches'][0] == wp.last_plan['launches'][0] + LAUNCH_DELTA[name]


@pytest.mark.parametrize('use_plan', [True, False])
def test_rollback_restores_the_offset_and_its_moments(dev, use_plan):
    """A forward scale sabotaged after step 15 of 40 (as tests/test_hip_ssim.py, tests/test_hip_wplus_long.py) with feature_layer = 5 at 32²: one
    window is repeated with exact scales from the last clean snapshot — (f, fm, fv) restored with (w, m, v) — and the run ends where the
    undisturbed run ends: losses within 1e-3 relative, the bar of that test.  Moments left at their sabotaged-window values would not."""
    from oodgan.engine import GeneratorEngine, WPlusInverter
    size, B, steps = 32, 2, 40
    eng = GeneratorEngine({k: v.to(dev) for k, v in synth.generator_state(size, seed=5).items()}, size)
    target = synth.make_images(size, B, seed=9).to(dev)
    noises = [n.to(dev) for n in synth.make_noises(size, B, seed=7)]
    w0 = synth.make_latents(size, B, seed=14).to(dev)
    inv = WPlusInverter(eng, use_plan=use_plan, feature_layer=5)
    w_ref, l_ref = inv.invert(target, w0, noises, steps=steps)
    d_ref = inv.last_feature_offset.clone()
    assert inv.last_stats == {'steps_run': [steps], 'rollbacks': [0]}
    done = {'n': 0}

    def sabotage(run):
        if run.steps_run == 15 and not done['n']:
            done['n'] = 1
            eng.fwd_range.q[3].mul_(2.0 ** 12)
    inv.on_step = sabotage
    w, l = inv.invert(target, w0, noises, steps=steps)
    inv.on_step = None
    d = inv.last_feature_offset
    rel = ((l - l_ref).abs() / l_ref).max().item()
    print(f'forward scale sabotaged after step 15 of {steps} with feature_layer 5 (plans {use_plan}): {inv.last_stats}; loss rel diff {rel:.2e} (bar 1e-3), '
          f'|delta - undisturbed| {(d - d_ref).abs().max().item():.2e}, |w - undisturbed| {(w - w_ref).abs().max().item():.2e}')
    assert inv.last_stats['rollbacks'] == [1] and inv.last_stats['steps_run'][0] == steps + inv.check_every + inv.check_lag
    assert torch.isfinite(l).all() and torch.isfinite(d).all()
    assert torch.equal(l[:inv.check_every], l_ref[:inv.check_every])        # the rows before the clean snapshot were never rewritten
    assert rel < 1e-3


def test_loop_controls(dev):
    """64², l = 5: ``feature_reg`` against the float64 loop of tests/fspace_ref.py (table within 1e-6 absolute, the total includes the term);
    ``layer_lr`` all zero leaves w bit-unchanged while the offset moves; ``feature_lr`` = 0 leaves the offset at zero while w moves; the SSIM
    term and a robust pixel term run with plan bits equal to Python-driven bits; latent_space 'w' runs; every refusal names its option."""
    from oodgan.engine import GeneratorEngine, WPlusInverter
    size, B, steps, lam, l = 64, 2, 8, 0.5, 5
    P, P64 = _state(size, 5)
    x, w0, noises = synth.make_images(size, B, seed=9), synth.make_latents(size, B, seed=14), synth.make_noises(size, B, seed=7)
    flr = 0.005     # not the latents' rate, and not above it: the absolute bar on the table belongs to offsets of size ~ lr * steps, as in tests/test_hip_sspace.py
    l64, r64, _, d64, _ = FR.invert(P64, size, w0.double(), l, x.double(), [n.double() for n in noises], steps, feature_lr=flr, feature_reg=lam)
    l32, r32 = FR.invert(P, size, w0, l, x, noises, steps, feature_lr=flr, feature_reg=lam)[:2]
    e_self, r_self = ((l32 - l64).abs() / l64).max().item(), (r32 - r64).abs().max().item()
    eng = GeneratorEngine({k: v.to(dev) for k, v in P.items()}, size)
    xd, wd, nd = x.to(dev), w0.to(dev), [n.to(dev) for n in noises]
    inv = WPlusInverter(eng, feature_layer=l, feature_lr=flr, feature_reg=lam)
    w, losses = inv.invert(xd, wd, nd, steps=steps)
    t = inv.last_terms
    e_curve = ((losses.double().cpu() - l64).abs() / l64).max().item()
    e_reg = (t['feature'].double().cpu() - r64).abs().max().item()
    print(f"{steps} steps 64² with feature_reg {lam}, feature_lr {flr}: loss curve rel {e_curve:.2e} vs the float64 loop (its fp32 twin: {e_self:.2e}); |feature table - float64| "
          f"{e_reg:.2e} (bar 1e-6; the helper's fp32 twin {r_self:.2e}; max {r64.max().item():.2e}); stats {inv.last_stats}, plan {inv.last_plan}")
    assert e_reg < 1e-6 and e_curve < max(1e-3, 3 * e_self)
    assert t['feature'].shape == (steps, B) and torch.equal(losses, t['mse'] + lam * t['feature']) and (t['feature'][0] == 0).all()
    assert (t['feature'][1:] > 0).all()
    assert inv.last_stats == {'steps_run': [steps], 'rollbacks': [0]} and inv.last_plan['steps'] == [steps - 3]
    # the offset alone
    inv = WPlusInverter(eng, feature_layer=l, layer_lr=[0.0] * w0.shape[1])
    w, lo = inv.invert(xd, wd, nd, steps=6)
    assert torch.equal(w, wd) and (inv.last_feature_offset != 0).any() and (lo[-1] < lo[0]).all()
    # the latents alone: a rate of 0 leaves the offset at zero
    inv = WPlusInverter(eng, feature_layer=l, feature_lr=0.0)
    w, lo = inv.invert(xd, wd, nd, steps=6)
    assert (inv.last_feature_offset == 0).all() and not torch.equal(w, wd) and (lo[-1] < lo[0]).all()
    # loss-side options and W: plan bits = Python-driven bits
    for kw in (dict(ssim_weight=0.5), dict(pixel_loss='huber', pixel_scale=0.1), dict(latent_space='w')):
        runs = []
        for use_plan in (True, False):
            inv = WPlusInverter(eng, feature_layer=l, use_plan=use_plan, **kw)
            w, lo = inv.invert(xd, wd, nd, steps=6)
            runs.append((w, lo, inv.last_feature_offset))
            assert inv.last_plan['steps'] == [3 if use_plan else 0] and inv.last_stats['rollbacks'] == [0]
        assert all(torch.equal(a, b) for a, b in zip(*runs)) and torch.isfinite(runs[0][1]).all() and (runs[0][2] != 0).any(), kw
    # refusals, each naming its option
    with pytest.raises(NotImplementedError, match='feature_layer'):
        WPlusInverter(eng, feature_layer=l).invert(xd, wd, nd, steps=2, use_graph=True)
    with pytest.raises(ValueError, match='feature_layer'):
        WPlusInverter(eng, feature_layer=l, latent_space='s')
    with pytest.raises(ValueError, match='feature_layer'):
        WPlusInverter(eng, feature_layer=9)
    w, lo = WPlusInverter(eng, feature_layer=l).invert(xd, wd, nd, steps=0)
    assert lo.shape == (0, B) and torch.equal(w, wd)
    e16 = GeneratorEngine({k: v.to(dev) for k, v in synth.generator_state(16, seed=5).items()}, 16)
    with pytest.raises(ValueError, match='feature_layer'):      # 16² has no up-conv that reads latent 5
        WPlusInverter(e16, feature_layer=5).invert(synth.make_images(16, 1, seed=9).to(dev), synth.make_latents(16, 1, seed=14).to(dev),
                                                   [n.to(dev) for n in synth.make_noises(16, 1, seed=7)], steps=2)
    with pytest.raises(RuntimeError, match='feature_grad'):
        eng.forward(wd, nd, save=True)
        eng.backward(torch.zeros(B, 3, size, size, device=dev), feature_grad=torch.zeros((B,) + eng.feature_shape(l), device=dev))
    eng.saved = None


def test_padded_generator_refuses_the_offset(dev):
    from oodgan.engine import GeneratorEngine, WPlusInverter
    size, B = 256, 1                 # 256² / 0.1875: 96 ... 48, 24 channels (tests/test_hip_generator.py)
    P = synth.generator_state(size, seed=5, narrow=0.1875)
    eng = GeneratorEngine({k: v.to(dev) for k, v in P.items()}, size, narrow=0.1875)
    assert eng.padded
    w = synth.make_latents(size, B, seed=14).to(dev)
    nz = [n.to(dev) for n in synth.make_noises(size, B, seed=7)]
    with pytest.raises(NotImplementedError, match='feature_layer'):
        eng.forward(w, nz, feature_offset=(5, torch.zeros(B, 96, 16, 16, device=dev)))
    with pytest.raises(NotImplementedError, match='feature_layer'):
        WPlusInverter(eng, feature_layer=5).invert(synth.make_images(size, B, seed=9).to(dev), w, nz, steps=2)


def test_loop_1024(dev):
    """1024², B = 1, l = 5, 6 steps — the F-form top level and the 8-wave routes above the offset layer; no oracle: finite, no rollback, the offset
    moves, plan bits = Python-driven bits."""
    from oodgan.engine import GeneratorEngine, WPlusInverter
    size, steps = 1024, 6
    P, _ = _state(size, 0)
    eng = GeneratorEngine({k: v.to(dev) for k, v in P.items()}, size)
    target, w0, noises = WG.recipe(size, [0])
    xd, wd, nd = target.to(dev), w0.to(dev), [n.to(dev) for n in noises]
    runs = []
    for use_plan in (True, False):
        inv = WPlusInverter(eng, feature_layer=5, use_plan=use_plan)
        w, lo = inv.invert(xd, wd, nd, steps=steps)
        assert inv.last_stats == {'steps_run': [steps], 'rollbacks': [0]} and inv.last_plan['steps'] == [steps - 3 if use_plan else 0]
        runs.append((w, lo, inv.last_feature_offset))
    w, lo, d = runs[0]
    print(f'1024² B=1 feature_layer 5, {steps} steps: loss {lo[:, 0].tolist()}, max |delta| {d.abs().max().item():.3e}')
    assert all(torch.equal(a, b) for a, b in zip(*runs))
    assert torch.isfinite(lo).all() and torch.isfinite(w).all() and torch.isfinite(d).all() and (d != 0).any() and (lo[-1] < lo[0]).all()


# ------------------------------------------------------------------------------------------------------------- model level
def test_model_invert_with_offset_at_64(dev):
    import test_hip_wplus_sched as S
    size, B, steps = 64, 2, 6
    m = S._model_64(dev)
    x = synth.make_images(size, B, seed=44).to(dev)
    kw = dict(enc_lats=synth.make_latents(size, B, seed=42, std=0.3).to(dev), noise=[n.to(dev) for n in synth.make_noises(size, B, seed=45)])
    out, lats, losses = m.invert(x, steps=steps, feature_layer=5, feature_reg=0.1, **kw)
    delta = m.last_feature_offset
    assert m.last_feature_layer == 5 and delta.shape == (B, 512, 16, 16) and (delta != 0).any() and torch.equal(lats, m.last_refined_lats)
    t = m.last_loss_terms
    assert t['feature'].shape == (steps, B) and torch.equal(losses, t['mse'] + 0.1 * t['feature'])
    again = m(x, lats=lats, feature_offset=delta, feature_layer=5, **kw)[0]
    assert torch.equal(again, out)
    plain = m(x, lats=lats, **kw)[0]
    moved = (plain - out).abs().max().item()
    print(f'model.invert(feature_layer=5) at 64²: losses {losses[:, 0].tolist()}; the offset moves the output by {moved:.2e}')
    assert moved > 1e-3 and (losses[-1] < losses[0]).all()
    # the generators take the same two keywords
    img, _ = m.generator(lats, input_is_tensor=True, input_is_latent=True, noise=kw['noise'], feature_offset=delta, feature_layer=5)
    assert torch.equal(img, out)
    with pytest.raises(ValueError, match='feature_layer'):
        m.generator(lats, input_is_tensor=True, input_is_latent=True, noise=kw['noise'], feature_offset=delta)
    # an edit keeps its meaning: added to the refined latents for the final forward, the offset as fitted
    e = synth.normal('fs.edit', tuple(lats.shape[1:]), 46, 0.1).to(dev)
    out_e, lats_e, losses_e = m.invert(x, steps=steps, feature_layer=5, feature_reg=0.1, edit=e, **kw)
    assert torch.equal(losses_e, losses) and torch.equal(m.last_feature_offset, delta) and torch.equal(lats_e, (lats + e).contiguous())
    assert torch.equal(out_e, m(x, lats=lats_e, feature_offset=delta, feature_layer=5, **kw)[0])
    # without the option nothing is left behind
    m.invert(x, steps=2, **kw)
    assert m.last_feature_offset is None and m.last_feature_layer is None and m.last_loss_terms['feature'] is None
    for bad, name in ((dict(feature_layer=4), 'feature_layer'), (dict(feature_layer=9), 'feature_layer'), (dict(feature_reg=0.1), 'feature_reg'),
                      (dict(feature_layer=5, latent_space='s'), 'feature_layer'), (dict(feature_layer=5, feature_lr=-1.0), 'feature_lr')):
        with pytest.raises(ValueError, match=name):
            m.invert(x, steps=2, **bad, **kw)
    with pytest.raises(NotImplementedError, match='feature_layer'):
        m.invert(x, steps=2, feature_layer=5, use_graph=True, **kw)


def test_model_with_modulation_at_256(dev):
    """With the modulation blocks (SAMM hooks on latents 5 and 7): the hook on the offset layer receives the raw up-conv output, which includes
    the offset's effect, and the output is the model's own forward at (w, delta), masks and blend included, bit for bit."""
    import test_hip_wplus_masked as M
    size, B, steps = 256, 2, 3
    m = M._ood_model(dev)
    x, kw = M._ood_inputs(dev, size, B)
    out, lats, losses = m.invert(x, steps=steps, feature_layer=5, **kw)
    delta = m.last_feature_offset
    assert (delta != 0).any() and torch.isfinite(out).all() and torch.isfinite(losses).all()
    assert torch.equal(m(x, lats=lats, feature_offset=delta, feature_layer=5, **kw)[0], out)
    assert not torch.equal(m(x, lats=lats, **kw)[0], out)
