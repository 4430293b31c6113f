"""Latent controls and edits of the W+ loop (csrc/wplus_sched.hip): the W tie, per-layer learning rates, the spread term, and
an editing direction applied after the fit.

The latent-step kernel against torch.optim.Adam in float64 and, with everything off, bit for bit against the scheduled Adam; the tied latent
noise against tests/latent_noise_ref.py; short runs against the oracle's autograd loop (inputs of tests/test_hip_wplus_sched.py); the
untouched default path, launch plans, streams, a rollback; the model-level arguments at 64², 256² (modulation blocks) and one step at 1024²."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import ref_cpu as R  # noqa: E402
from oodgan import synth  # noqa: E402
from oodgan.ops import lr_multiplier  # noqa: E402
import latent_noise_ref as N  # noqa: E402
import test_hip_wplus_masked as M  # noqa: E402   (_ood_model, _ood_inputs)
import test_hip_wplus_sched as S  # noqa: E402    (_inputs, _hip_inputs, _engine, _model_64, _RUN, _OPT)


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


def _i32(v, dev):
    return torch.tensor([v], dtype=torch.int32, device=dev)


def _spread(w):
    """R_b = mean_le (w_le - mean_l w_le)^2 for w (B, L, D)."""
    return ((w - w.mean(dim=1, keepdim=True)) ** 2).mean(dim=(1, 2))


def _rows_identical(t):
    return bool(torch.equal(t, t[:, :1].expand_as(t)))


# ------------------------------------------------------------------------------------------------------------- the kernel
_SHAPES = [(2, 18, 512), (3, 10, 512), (1, 4, 37), (2, 3, 600), (2, 1, 512)]
_ADAM = dict(total=6, up=0.34, down=0.5, lr=0.01)


def _rates(L):
    return [((l + 1) % 4) * 0.5 for l in range(L)]     # 0.5, 1, 1.5, 0 (frozen), ...


@pytest.mark.parametrize('controls', ['tie', 'layer_lr', 'delta', 'layer_lr+delta'])
@pytest.mark.parametrize('shape', _SHAPES)
def test_latent_step_vs_float64(dev, shape, controls):
    """Six steps with the gradients of test_scheduled_adam_vs_float64 against torch.optim.Adam in float64: on a (B,D) leaf expanded to the L
    layers (tie), on one leaf per layer with lr * layer_lr[l], with lambda * R added to the loss (its gradient by autograd).  Bars (double
    sums rounded once, as the prior's and the scheduled Adam's): w 1e-6 max(1, max|w|), R 1e-6 relative, the g written back 1e-6 of its maximum."""
    from oodgan import ops
    B, L, D = shape
    total, up, down, lr = _ADAM['total'], _ADAM['up'], _ADAM['down'], _ADAM['lr']
    tied = controls == 'tie'
    rates = _rates(L) if 'layer_lr' in controls else None
    lam = 0.5 if 'delta' in controls else 0.0
    w0 = synth.normal('ad.w', shape, 3)
    if tied:
        w0 = w0[:, :1].expand(shape).contiguous()
        leaves = [w0[:, 0].double().clone().requires_grad_(True)]
        opt = torch.optim.Adam(leaves, lr=lr, betas=(0.9, 0.999), eps=1e-8)
    else:
        leaves = [w0[:, l].double().clone().requires_grad_(True) for l in range(L)]
        opt = torch.optim.Adam([dict(params=[p]) for p in leaves], lr=lr, betas=(0.9, 0.999), eps=1e-8)
    wd = w0.clone().to(dev)
    m, v, t = torch.zeros_like(wd), torch.zeros_like(wd), _i32(0, dev)
    rd = None if rates is None else torch.tensor(rates, dtype=torch.float32, device=dev)
    table = torch.full((total, B), -1.0, device=dev)
    worst = dict(w=0.0, R=0.0, g=0.0)
    for i in range(total):
        gr = synth.normal(f'ad.g{i}', shape, 4) * (10.0 ** (-(i % 3) - 1))
        for k, grp in enumerate(opt.param_groups):
            grp['lr'] = lr * lr_multiplier(i, total, up, down) * (1.0 if rates is None else rates[k])
        opt.zero_grad(set_to_none=True)
        w = leaves[0][:, None, :].expand(shape) if tied else torch.stack(leaves, 1)
        w.retain_grad()
        R_ref = _spread(w)
        # d(sum_b (gr . w + lam R_b))/d leaf: the step's gradient gr and the spread term's, through the expansion / the stack
        ((gr.double() * w).sum() + lam * R_ref.sum()).backward()
        g_ref = w.grad.sum(dim=1, keepdim=True).expand(shape) if tied else w.grad
        opt.step()
        g = gr.to(dev)
        ops.latent_step(wd, g, m, v, t, total, up, down, lr, layer_lr=rd, delta_reg=lam, tied=tied, table=table)
        w_ref = (leaves[0][:, None, :].expand(shape) if tied else torch.stack(leaves, 1)).detach()
        e_w = (wd.double().cpu() - w_ref).abs().max().item() / max(1.0, w_ref.abs().max().item())
        e_g = (g.double().cpu() - g_ref).abs().max().item() / g_ref.abs().max().item()
        got_R, R_ref = table[i].double().cpu(), R_ref.detach()
        e_R = 0.0 if (L == 1 or tied) else ((got_R - R_ref).abs() / R_ref).max().item()
        print(f'latent step {shape} {controls} step {i}: w err {e_w:.2e}, R rel err {e_R:.2e}, g err {e_g:.2e} of max (bars 1e-6)')
        assert e_w <= 1e-6 and e_R <= 1e-6 and e_g <= 1e-6
        assert int(t.item()) == i + 1
        if L == 1 or tied:                  # one layer, or identical layers: no spread
            assert (got_R == 0).all() and R_ref.max().item() <= 1e-25
        if tied:
            assert _rows_identical(wd) and _rows_identical(m) and _rows_identical(v) and _rows_identical(g)
        if lam == 0.0 and not tied:
            assert torch.equal(g.cpu(), gr)                 # nothing to add: g is not touched
        for l in [l for l, r in enumerate(rates or []) if r == 0.0]:        # rate 0: the row never moves, its moments do
            assert torch.equal(wd[:, l].cpu(), w0[:, l]) and (m[:, l] != 0).any() and (v[:, l] != 0).any()
        worst = {k: max(worst[k], e) for k, e in (('w', e_w), ('R', e_R), ('g', e_g))}
    assert (table >= 0).all()               # every row written, each by its own step
    assert not torch.equal(wd.cpu(), w0)


@pytest.mark.parametrize('shape', [(2, 18, 512), (1, 4, 37), (2, 3, 600)])
def test_latent_step_off_is_the_scheduled_adam(dev, shape):
    """No tie, lambda = 0, layer_lr absent or all 1.0: w, m, v, t bit for bit those of adam_step_dev_sched — with both ramps off therefore
    those of adam_step_dev (tests/test_hip_wplus_sched.py) — and g is not written."""
    from oodgan import ops
    total, up, down, lr = _ADAM['total'], _ADAM['up'], _ADAM['down'], _ADAM['lr']
    w0 = synth.normal('ad.w', shape, 3).to(dev)
    ones = torch.ones(shape[1], device=dev)
    for ramps in ((up, down), (0.0, 0.0)):
        state = [[w0.clone(), torch.zeros_like(w0), torch.zeros_like(w0), _i32(0, dev)] for _ in range(3)]
        for i in range(total):
            gr = (synth.normal(f'ad.g{i}', shape, 4) * (10.0 ** (-(i % 3) - 1))).to(dev)
            (wa, ma, va, ta), (wb, mb, vb, tb), (wc, mc, vc, tc) = state
            ops.adam_step_dev_sched(wa, gr, ma, va, ta, total, ramps[0], ramps[1], lr)
            gb, gc = gr.clone(), gr.clone()
            ops.latent_step(wb, gb, mb, vb, tb, total, ramps[0], ramps[1], lr)
            ops.latent_step(wc, gc, mc, vc, tc, total, ramps[0], ramps[1], lr, layer_lr=ones)
            for got in (state[1], state[2]):
                assert all(torch.equal(a, b) for a, b in zip(state[0], got)), (shape, ramps, i)
            assert torch.equal(gb, gr) and torch.equal(gc, gr)
        assert not torch.equal(state[0][0], w0)


def test_latent_step_table_row_and_single_value_form(dev):
    """The table form writes row t_dev[0] (before the increment, clamped to the table) and no other; ``loss_out`` receives the same values."""
    from oodgan import ops
    shape = (3, 10, 512)
    B = shape[0]
    w0 = synth.normal('ad.w', shape, 3).to(dev)
    gr = synth.normal('ad.g0', shape, 4).to(dev)
    want = _spread(w0.double().cpu())
    table = torch.full((4, B), -1.0, device=dev)
    first = None
    for row in (2, 9):
        w, t = w0.clone(), _i32(row, dev)
        ops.latent_step(w, gr.clone(), torch.zeros_like(w), torch.zeros_like(w), t, 20, delta_reg=0.5, table=table)
        assert int(t.item()) == row + 1
        got = table[min(row, 3)]
        assert ((got.double().cpu() - want).abs() / want).max().item() <= 1e-6
        first = got.clone() if first is None else first
        assert torch.equal(got, first)
    assert torch.equal(table[:2], torch.full((2, B), -1.0, device=dev))
    out = torch.full((B,), -1.0, device=dev)
    ops.latent_step(w0.clone(), gr.clone(), torch.zeros_like(w0), torch.zeros_like(w0), _i32(5, dev), 20, delta_reg=0.5, loss_out=out)
    assert torch.equal(out, first)
    with pytest.raises(ValueError, match='latent_step'):
        ops.latent_step(w0[0], gr[0], w0[0], w0[0], _i32(0, dev), 20)


def test_tied_noise(dev):
    """period = 512 on a (B, 18*512) latent with identical rows: the draws of latent_noise_ref for n = 512, tiled over the layers, within the
    noise kernel's bar (1e-5 sigma_0), and the rows of w_in bit-identical; period = n: the bits of ops.latent_noise; a bad period raises."""
    from oodgan import ops
    ids, L, D, total, sigma0, ramp, seed, step = [0, 2 ** 33 + 1, 7], 18, 512, 20, 0.5, 0.75, 3, 7
    B, n = len(ids), L * D
    row = synth.normal('tied.w', (B, 1, D), 21)
    w = row.expand(B, L, D).contiguous().to(dev)
    t_dev, idt = _i32(step, dev), torch.tensor(ids, dtype=torch.int64, device=dev)
    w_in = ops.latent_noise(w, t_dev, idt, total, sigma0, ramp, seed, period=D)
    ref = np.tile(N.latent_noise(seed, ids, step, D, total, sigma0, ramp), (1, L))
    err = np.abs(w_in.double().cpu().numpy().reshape(B, n) - w.double().cpu().numpy().reshape(B, n) - ref).max()
    print(f'tied latent noise B={B}, period {D} of {n}: max |w_in - w - sigma n_ref| = {err:.2e} (bar {1e-5 * sigma0:.1e})')
    assert err <= 1e-5 * sigma0 and _rows_identical(w_in) and not torch.equal(w_in, w)
    # the first period is what the untied entry draws there; period = n is the untied entry
    plain = ops.latent_noise(w, t_dev, idt, total, sigma0, ramp, seed)
    assert torch.equal(plain[:, 0], w_in[:, 0]) and not torch.equal(plain[:, 1], w_in[:, 1])
    assert torch.equal(ops.latent_noise(w, t_dev, idt, total, sigma0, ramp, seed, period=n), plain)
    flat = w.reshape(B, n)
    assert torch.equal(ops.latent_noise(flat, t_dev, idt, total, sigma0, ramp, seed, period=D).reshape(B, L, D), w_in)
    for bad in (0, -512, 6, 510, 1024 * 5, 2 * n, 512.0, True):
        with pytest.raises(ValueError, match='period'):
            ops.latent_noise(w, t_dev, idt, total, sigma0, ramp, seed, period=bad)
    from oodgan import _lib
    rc = _lib.lib().oodgan_latent_noise_tied(ops._p(w), ops._p(w_in), ops._p(idt), ops._p(t_dev), B, n, 6, seed, total, sigma0, ramp, ops._stream())
    assert rc == -1 and b'latent_noise_tied' in _lib.lib().oodgan_last_error()


# ------------------------------------------------------------------------------------------------------- the loop
_RUN, _OPT = S._RUN, S._OPT
_FROZEN_FROM = 4
_ORACLE = {}


def _oracle_run(kind, dt):
    """The oracle's autograd + torch.optim.Adam loop of tests/test_hip_wplus_sched.py (ramps, noise, prior towards the start latents) in
    dtype ``dt`` with kind 'w': a (B,512) leaf, the layer mean of the start latents, expanded to the L layers, one 512-vector of noise
    repeated; 'delta': 0.5 * R added to the loss and the layers from _FROZEN_FROM on at learning rate 0.  -> (total losses, R tables)."""
    if (kind, dt) not in _ORACLE:
        size, B, steps, lr = _RUN['size'], _RUN['B'], _RUN['steps'], _RUN['lr']
        P, x, noises, w0 = S._inputs(size, B)
        P, x, noises, w0 = {k: v.to(dt) for k, v in P.items()}, x.to(dt), [n.to(dt) for n in noises], w0.to(dt)
        L, D = w0.shape[1:]
        if kind == 'w':
            leaves = [w0.mean(dim=1).clone().requires_grad_(True)]
            groups = [dict(params=leaves)]
        else:
            leaves = [w0[:, :_FROZEN_FROM].clone().requires_grad_(True), w0[:, _FROZEN_FROM:].clone().requires_grad_(True)]
            groups = [dict(params=[leaves[0]]), dict(params=[leaves[1]])]
        opt = torch.optim.Adam(groups, lr=lr, betas=(0.9, 0.999), eps=1e-8)
        tot, spread = [], []
        for i in range(steps):
            lr_i = lr * lr_multiplier(i, steps, _OPT['lr_rampup'], _OPT['lr_rampdown'])
            opt.param_groups[0]['lr'] = lr_i
            if kind != 'w':
                opt.param_groups[1]['lr'] = 0.0
            opt.zero_grad(set_to_none=True)
            if kind == 'w':
                w = leaves[0][:, None, :].expand(B, L, D)
                nz = np.tile(N.latent_noise(0, range(B), i, D, steps, _OPT['latent_noise'], _OPT['noise_ramp']), (1, L))
            else:
                w = torch.cat(leaves, 1)
                nz = N.latent_noise(0, range(B), i, L * D, steps, _OPT['latent_noise'], _OPT['noise_ramp'])
            img = R.generator_forward(P, w + torch.from_numpy(nz).to(dt).reshape(B, L, D), noises, size)
            p, r = ((w - w0) ** 2).mean(dim=(1, 2)), _spread(w)
            t = ((img - x) ** 2).mean(dim=(1, 2, 3)) + _OPT['latent_reg'] * p + (0.5 * r if kind != 'w' else 0.0)
            t.sum().backward()
            tot.append(t.detach().clone())
            spread.append(r.detach().clone())
            opt.step()
        _ORACLE[(kind, dt)] = (torch.stack(tot).double(), torch.stack(spread).double())
    return _ORACLE[(kind, dt)]


def test_w_space_run_vs_the_oracle_loop(dev):
    """20 steps at 64², B=3 in W with ramps, noise and prior on: the total-loss curve within max(1e-3, 3x the oracle's own fp32-vs-float64
    distance) of the oracle's loop on a (B,512) leaf; the rows of the final w bit-identical."""
    from oodgan.engine import WPlusInverter
    size, B, steps = _RUN['size'], _RUN['B'], _RUN['steps']
    l64, _ = _oracle_run('w', torch.float64)
    l32, _ = _oracle_run('w', torch.float32)
    e_self = ((l32 - l64).abs() / l64).max().item()
    x, w0, noises = S._hip_inputs(dev, size, B)
    inv = WPlusInverter(S._engine(dev, size), lr=_RUN['lr'], latent_space='w', **_OPT)
    w, losses = inv.invert(x, w0, noises, steps=steps, latent_anchor=w0)
    e_curve = ((losses.double().cpu() - l64).abs() / l64).max().item()
    print(f"20 steps 64² in W with the schedule: loss curve rel {e_curve:.2e} vs the float64 oracle loop (its own fp32 loop: {e_self:.2e}); "
          f'stats {inv.last_stats}, plan {inv.last_plan}')
    assert e_curve < max(1e-3, 3 * e_self)
    assert _rows_identical(w) and not torch.equal(w, w0.mean(dim=1, keepdim=True).expand_as(w0))
    t = inv.last_terms
    assert t['delta'] is None and torch.equal(losses, t['mse'] + _OPT['latent_reg'] * t['latent'])
    assert inv.last_stats == {'steps_run': [steps], 'rollbacks': [0]}


def test_spread_and_frozen_layers_run_vs_the_oracle_loop(dev):
    """The same comparison with delta_reg = 0.5 and layer_lr 1 on the first four layers, 0 on the rest: the curve as above, the spread's table
    within 1e-5 absolute, the frozen rows those of w0."""
    from oodgan.engine import WPlusInverter
    size, B, steps = _RUN['size'], _RUN['B'], _RUN['steps']
    l64, r64 = _oracle_run('delta', torch.float64)
    l32, _ = _oracle_run('delta', torch.float32)
    e_self = ((l32 - l64).abs() / l64).max().item()
    x, w0, noises = S._hip_inputs(dev, size, B)
    L = w0.shape[1]
    rates = [1.0] * _FROZEN_FROM + [0.0] * (L - _FROZEN_FROM)
    inv = WPlusInverter(S._engine(dev, size), lr=_RUN['lr'], delta_reg=0.5, layer_lr=rates, **_OPT)
    w, losses = inv.invert(x, w0, noises, steps=steps, latent_anchor=w0)
    t = inv.last_terms
    e_curve = ((losses.double().cpu() - l64).abs() / l64).max().item()
    e_dl = (t['delta'].double().cpu() - r64).abs().max().item()
    print(f'20 steps 64² with delta_reg 0.5, layers {_FROZEN_FROM}.. frozen: loss curve rel {e_curve:.2e} vs the float64 oracle loop (its own fp32 '
          f'loop: {e_self:.2e}); |spread table - oracle| {e_dl:.2e} (max {r64.max().item():.2e}); stats {inv.last_stats}')
    assert e_curve < max(1e-3, 3 * e_self)
    assert e_dl < 1e-5
    assert torch.equal(w[:, _FROZEN_FROM:], w0[:, _FROZEN_FROM:]) and not torch.equal(w[:, :_FROZEN_FROM], w0[:, :_FROZEN_FROM])
    assert t['delta'].shape == (steps, B) and torch.equal(losses, t['mse'] + _OPT['latent_reg'] * t['latent'] + 0.5 * t['delta'])
    assert inv.last_stats == {'steps_run': [steps], 'rollbacks': [0]}


def _controls(L):
    return (dict(latent_space='w'), dict(layer_lr=[1.0] * 4 + [0.5] * (L - 4)), dict(delta_reg=0.5))


def test_defaults_are_the_parent_path_and_each_control_moves_the_run(dev):
    from oodgan.engine import WPlusInverter
    size, B, steps = 64, 2, 8
    eng = S._engine(dev, size)
    x, w0, noises = S._hip_inputs(dev, size, B)
    L = w0.shape[1]
    base = WPlusInverter(eng)
    w_b, l_b = base.invert(x, w0, noises, steps=steps)
    n_b = base.last_plan['launches']
    assert base.last_terms['delta'] is None and n_b[0] > 0
    off = WPlusInverter(eng, latent_space='w+', layer_lr=None, delta_reg=0.0)
    w, l = off.invert(x, w0, noises, steps=steps)
    assert torch.equal(w, w_b) and torch.equal(l, l_b) and off.last_plan['launches'] == n_b and off.last_terms['delta'] is None
    # the latent step replaces the Adam call: the counter increment plus one kernel either way
    for opt in _controls(L):
        inv = WPlusInverter(eng, **opt)
        w, l = inv.invert(x, w0, noises, steps=steps)
        assert torch.isfinite(w).all() and torch.isfinite(l).all() and not torch.equal(w, w_b), opt
        assert inv.last_plan['launches'] == n_b, (opt, inv.last_plan, n_b)
        assert (inv.last_terms['delta'] is not None) == ('delta_reg' in opt)
        assert _rows_identical(w) == ('latent_space' in opt)
        with pytest.raises(NotImplementedError):
            WPlusInverter(eng, **opt).invert(x, w0, noises, steps=2, use_graph=True)
    # rates of 1.0 are the default run
    w, l = WPlusInverter(eng, layer_lr=[1.0] * L).invert(x, w0, noises, steps=steps)
    assert torch.equal(w, w_b) and torch.equal(l, l_b)
    with pytest.raises(ValueError, match='layer_lr'):
        WPlusInverter(eng, layer_lr=[1.0] * (L + 1)).invert(x, w0, noises, steps=2)
    # no steps: W still returns its start, the layer mean on every layer
    w, l = WPlusInverter(eng, latent_space='w').invert(x, w0, noises, steps=0)
    assert _rows_identical(w) and l.shape == (0, B)


def test_plans_and_streams(dev):
    """Plan on and off are bit-equal; two streams within the bars of tests/test_hip_wplus_sched.py::test_plans_streams_and_trajectory."""
    from oodgan.engine import WPlusInverter
    size, B, steps = 64, 3, 12
    eng = S._engine(dev, size)
    x, w0, noises = S._hip_inputs(dev, size, B)
    L = w0.shape[1]
    anchor = (w0 + 0.1).contiguous()
    for opt in (dict(latent_space='w'), dict(layer_lr=[1.0] * 4 + [0.0] * (L - 4), delta_reg=0.5)):
        inv = WPlusInverter(eng, use_plan=True, **opt, **_OPT)
        w1, l1 = inv.invert(x, w0, noises, steps=steps, latent_anchor=anchor)
        d1 = None if inv.last_terms['delta'] is None else inv.last_terms['delta'].clone()
        assert inv.last_plan['steps'] == [steps - 3] and inv.last_stats['rollbacks'] == [0]
        inv2 = WPlusInverter(eng, use_plan=False, **opt, **_OPT)
        w2, l2 = inv2.invert(x, w0, noises, steps=steps, latent_anchor=anchor)
        assert inv2.last_plan['steps'] == [0]
        assert torch.equal(w1, w2) and torch.equal(l1, l2) and (d1 is None or torch.equal(d1, inv2.last_terms['delta']))
        w3, l3 = inv.invert(x, w0, noises, steps=steps, streams=2, latent_anchor=anchor)
        rel0 = (l3[0] - l1[0]).abs().max().item() / l1[0].abs().max().item()
        rel = (l3 - l1).abs().max().item() / l1.abs().max().item()
        frac = ((w3 - w1).abs() < 5e-4).float().mean().item()
        print(f'{opt}: 2 streams vs 1 at 64², B={B}: loss rel diff step 1 {rel0:.2e}, all steps {rel:.2e}, {100 * frac:.3f}% of w within 5e-4; '
              f'plan {inv.last_plan}')
        assert rel0 <= 1e-5 and rel <= 1e-3 and frac > 0.999
        assert inv.last_plan['steps'] == [steps - 3] * 2
        if 'latent_space' in opt:
            assert _rows_identical(w1) and _rows_identical(w3)
        else:
            assert torch.equal(w3[:, 4:], w0[:, 4:]) and inv.last_terms['delta'].shape == (steps, B)


def test_rollback_keeps_the_tie(dev):
    """A forward scale sabotaged after step 15 of 40 (the pattern of tests/test_hip_wplus_sched.py::test_rollback_repeats_the_same_draws), in W
    with noise, plans on: exactly one rollback, finite results, rows still bit-identical, the loss within 1e-3 relative of the undisturbed run."""
    from oodgan.engine import WPlusInverter
    size, B, steps = 32, 2, 40
    eng = S._engine(dev, size)
    x, w0, noises = S._hip_inputs(dev, size, B)
    inv = WPlusInverter(eng, use_plan=True, latent_space='w', lr_rampup=0.05, lr_rampdown=0.25, latent_noise=0.05, noise_ramp=0.0, noise_seed=2,
                        latent_reg=0.5)
    w_ref, l_ref = inv.invert(x, w0, noises, steps=steps, latent_anchor=w0)
    assert inv.last_stats == {'steps_run': [steps], 'rollbacks': [0]}
    done = {'n': 0}

    def fault(run):
        if run.steps_run == 15 and not done['n']:
            done['n'] = 1
            eng.fwd_range.q[3].mul_(2.0 ** 12)

    inv.on_step = fault
    w, l = inv.invert(x, w0, noises, steps=steps, latent_anchor=w0)
    inv.on_step = None
    rel = ((l - l_ref).abs() / l_ref).max().item()
    print(f'rollback in W: {inv.last_stats}, plan {inv.last_plan}; |loss - undisturbed| rel {rel:.2e}')
    assert inv.last_stats['rollbacks'] == [1] and inv.last_stats['steps_run'][0] == steps + inv.check_every + inv.check_lag
    assert torch.isfinite(w).all() and torch.isfinite(l).all()
    assert _rows_identical(w) and _rows_identical(w_ref)
    assert rel < 1e-3


# ------------------------------------------------------------------------------------------------------- model level
def test_model_edit_at_64(dev):
    size, B, steps = 64, 2, 6
    m = S._model_64(dev)
    x = synth.make_images(size, B, seed=44).to(dev)
    kw = dict(enc_lats=synth.make_latents(size, B, seed=42, std=0.3).to(dev), noise=[n.to(dev) for n in synth.make_noises(size, B, seed=45)])
    L = m.generator.n_latent
    d = synth.normal('edit.d', (L, 512), 46, 0.2).to(dev)
    out0, lats0, l0 = m.invert(x, steps=steps, **kw)
    ref0 = m.last_refined_lats.clone()
    assert torch.equal(ref0, lats0)                                      # set without an edit as well
    out, lats, l = m.invert(x, steps=steps, edit=d, **kw)
    assert torch.equal(l, l0) and torch.equal(m.last_refined_lats, ref0)
    assert torch.equal(lats, ref0 + d)
    want, _ = m.generator(ref0 + d, input_is_tensor=True, input_is_latent=True, noise=kw['noise'])
    assert torch.equal(out, want) and not torch.equal(out, out0)
    for form in (d[None], d[None].expand(B, -1, -1).contiguous()):
        o2, la2, l2 = m.invert(x, steps=steps, edit=form, **kw)
        assert torch.equal(o2, out) and torch.equal(la2, lats) and torch.equal(l2, l0)
    for bad in (d[:, :100].contiguous(), d[None].expand(B + 1, -1, -1).contiguous(), d.double(), d.cpu(), d.reshape(-1), 1.0):
        with pytest.raises(ValueError, match='edit'):
            m.invert(x, steps=2, edit=bad, **kw)
    # the controls through the model: checked there, passed on, their table in last_loss_terms
    o, la, lo = m.invert(x, steps=steps, latent_space='w', **kw)
    assert _rows_identical(m.last_refined_lats) and torch.equal(la, m.last_refined_lats) and m.last_loss_terms['delta'] is None
    o, la, lo = m.invert(x, steps=steps, delta_reg=0.5, layer_lr=[1.0] * 4 + [0.0] * (L - 4), **kw)
    w0 = m.encode(x, **kw)[0]
    t = m.last_loss_terms
    assert torch.equal(la[:, 4:], w0[:, 4:]) and torch.equal(lo, t['mse'] + 0.5 * t['delta'])
    for bad, name in ((dict(latent_space='z'), 'latent_space'), (dict(layer_lr=[1.0] * (L - 1)), 'layer_lr'), (dict(layer_lr=[-1.0] * L), 'layer_lr'),
                      (dict(delta_reg=float('nan')), 'delta_reg'), (dict(latent_space='w', delta_reg=1.0), 'delta_reg'),
                      (dict(latent_space='w', layer_lr=[1.0] * L), 'layer_lr')):
        with pytest.raises(ValueError, match=name):
            m.invert(x, steps=2, **bad, **kw)
    for opt in (dict(latent_space='w'), dict(layer_lr=[1.0] * L), dict(delta_reg=0.5)):
        with pytest.raises(NotImplementedError):
            m.invert(x, steps=2, use_graph=True, **opt, **kw)


def test_model_edit_at_256_with_modulation(dev):
    """With the modulation blocks: the output is the model's own forward at refined + d (masks and blend included), bit for bit."""
    size, B, steps = 256, 2, 3
    m = M._ood_model(dev)
    x, kw = M._ood_inputs(dev, size, B)
    d = synth.normal('edit.d', (m.generator.n_latent, 512), 47, 0.2).to(dev)
    out0, lats0, l0 = m.invert(x, steps=steps, **kw)
    out, lats, l = m.invert(x, steps=steps, edit=d, **kw)
    refined = m.last_refined_lats
    assert torch.equal(l, l0) and torch.equal(refined, lats0) and torch.equal(lats, refined + d)
    want = m(x, lats=(refined + d).contiguous(), **kw)[0]
    assert torch.equal(out, want) and not torch.equal(out, out0)
    o2, la2, _ = m.invert(x, steps=steps, edit=d[None].expand(B, -1, -1).contiguous(), **kw)
    assert torch.equal(o2, out) and torch.equal(la2, lats)


def test_one_w_step_at_1024(dev):
    """One 1024² step at B=1 in W with noise and the prior (the pattern of tests/test_hip_wplus_sched.py::test_one_step_at_1024): finite, the rows
    identical, the loss row the sum of its terms."""
    from oodgan.engine import GeneratorEngine, WPlusInverter
    size, B, reg = 1024, 1, 0.5
    eng = GeneratorEngine({k: v.to(dev) for k, v in synth.generator_state(size, seed=0).items()}, size)
    target = synth.make_images(size, B, seed=81).to(dev)
    noises = [n.to(dev) for n in synth.make_noises(size, B, seed=82)]
    w0 = synth.make_latents(size, B, seed=83, std=0.3).to(dev)
    anchor = synth.make_latents(size, 1, seed=84, std=0.3)[0].to(dev)
    inv = WPlusInverter(eng, latent_space='w', latent_noise=0.05, noise_ramp=0.75, noise_seed=7, latent_reg=reg)
    w, losses = inv.invert(target, w0, noises, steps=1, latent_anchor=anchor)
    torch.cuda.synchronize()
    t = inv.last_terms
    assert inv.last_stats == {'steps_run': [1], 'rollbacks': [0]} and torch.isfinite(w).all() and torch.isfinite(losses).all()
    assert losses.shape == (1, B) and torch.equal(losses, t['mse'] + reg * t['latent'])
    start = w0.mean(dim=1, keepdim=True).expand_as(w0)
    assert _rows_identical(w) and not torch.equal(w, start)
    want = ((start.double() - anchor.double()) ** 2).mean(dim=(1, 2)).cpu()
    assert ((t['latent'][0].double().cpu() - want).abs() / want).max().item() <= 1e-6
