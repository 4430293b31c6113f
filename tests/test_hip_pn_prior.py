"""The P_N+ prior of the W+ loop (csrc/latent_pn.hip): pn_reg * mean_{l,d} q^T M q per image, q = l5(w) - mu.

The kernel against float64 autograd (tests/pn_ref.py) on synthetic statistics with the spread of a real mapping network;
``Generator.pn_stats`` against the yardstick's statistics; the latent side of a step against torch.optim.Adam in float64; the loop at 64²
(plans, streams, the untouched default path, the refusals); a 20-step run against the reference's autograd loop (tests/golden/wplus_pn.npz);
the model-level arguments.

Measured on an MI355X (this file's own prints):
  kernel against float64, the 5e7-conditioned spectrum — loss rel err / gradient err of its maximum (the fp32 restatement's own errors):
    (1,18,512) 3.1e-8 / 1.5e-7 (9.3e-8 / 6.0e-7)    (3,10,512) 2.4e-8 / 1.3e-7 (1.1e-7 / 4.8e-7)    (2,1,512) 3.6e-8 / 1.2e-7 (2.7e-7 / 5.0e-7)
    (2,3,37) 2.2e-8 / 9.7e-8 (2.0e-7 / 1.6e-7)      (1,4,600) 2.7e-8 / 1.2e-7 (2.7e-8 / 3.2e-7)      (2,3,512), matrix 4 bytes off: 6.0e-8 / 1.4e-7 (1.5e-7 / 9.1e-7)
  Generator.pn_stats(4096, 3, floor 1e-4): mean equal to the yardstick's; pn of 8 probes 5.0e-8 from the float64 statistics (restatement 7.5e-8)
  latent side, six Adam steps: w within 1.5e-7 max(1, max|w|) of float64 in every mode and shape (bar 1e-6)
  loop at 64², B = 3: two streams 0 (step 1) / 5.7e-8 (all steps) of one, 100 % of w within 5e-4; pn 4.8e5 -> 9.1e4 in 12 steps at lambda 1e-3
  20 steps at 64² against the reference loop: loss curve 9.3e-6 of float64 (the reference's own fp32 loop: 8.9e-6), pn table 3.6e-6,
  max |w - reference fp32| 3.5e-6 / 1.7e-4 / 7.0e-4 after steps 1 / 10 / 20"""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import ref_cpu as R  # noqa: E402
from oodgan import synth  # noqa: E402
from oodgan.ops import lr_multiplier  # noqa: E402
import pn_ref  # noqa: E402
import test_hip_wplus_sched as S  # noqa: E402    (_engine, _hip_inputs, _model_64, _OPT)
import wplus_one_run_cases as C  # noqa: E402     (COUNTERS)

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'wplus_pn.npz')


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


def _i32(v, dev):
    return torch.tensor([v], dtype=torch.int32, device=dev)


_SYN = {}


def _synthetic(dim, dev):
    """(yardstick statistics, PNStats on the device) for the synthetic spectrum, once per width."""
    from oodgan.pn import PNStats
    if dim not in _SYN:
        ref = pn_ref.synthetic_stats(dim, seed=dim)
        _SYN[dim] = (ref, PNStats(ref['mean'], ref['components'], ref['variance'], n=0, seed=dim, floor=0.0, device=dev))
    return _SYN[dim]


def _float64(w, ref, weight):
    """(pn_b, weight * d sum_b pn_b / dw) by float64 autograd through the whitened coordinates."""
    x = w.double().clone().requires_grad_(True)
    pn = pn_ref.term(x, ref)
    (weight * pn.sum()).backward()
    return pn.detach(), x.grad


def _restatement_errors(w, ref, weight, pn64, g64):
    """The errors of the fp32 plain-torch restatement of the kernel's formula (float32 mean and matrix, the quadratic form, autograd) on the
    same inputs, against float64: (loss rel err, gradient err relative to max|grad|).  They set the kernel's bars."""
    x = w.clone().requires_grad_(True)
    pn = pn_ref.term_matrix(x, ref['mean'].float(), ref['matrix'].float())
    (weight * pn.sum()).backward()
    return (((pn.detach().double() - pn64).abs() / pn64).max().item(), (x.grad.double() - g64).abs().max().item() / g64.abs().max().item())


# ------------------------------------------------------------------------------------------------------------- the kernel
_SHAPES = [(1, 18, 512), (3, 10, 512), (2, 1, 512), (2, 3, 37), (1, 4, 600)]


@pytest.mark.parametrize('shape', _SHAPES)
def test_kernel_vs_float64(dev, shape):
    """Bars: loss rel err <= max(1e-6, 4 x the fp32 restatement's own error against float64), gradient err <= the same rule relative to
    max|grad|; the factor 4 covers another summation order.  The call accumulates into a non-zero g; the loss-only call, the table form and
    a second call give the same bits."""
    from oodgan import _lib, ops
    B, L, D = shape
    weight = 0.7
    ref, st = _synthetic(D, dev)
    w = pn_ref.sample(ref, shape, seed=17)
    w[:, 0, 0], w[:, 0, 1], w[-1, -1, -1] = 0.0, -0.0, 0.0
    assert (w < 0).float().mean().item() > 0.2 and (w[:, 0, :2] == 0).all()
    pn64, g64 = _float64(w, ref, weight)
    e_loss_r, e_grad_r = _restatement_errors(w, ref, weight, pn64, g64)
    bar_loss, bar_grad = max(1e-6, 4 * e_loss_r), max(1e-6, 4 * e_grad_r)
    wd = w.to(dev)
    g0 = (0.5 * g64.abs().max().item() * synth.normal('pn.g0', shape, 3)).to(dev)
    g = g0.clone()
    n0 = _lib.dispatch_count('pn')
    loss = ops.pn_prior_loss_grad(wd, st.mean, st.matrix, g, weight)
    assert _lib.dispatch_count('pn') == n0 + 1
    e_loss = ((loss.double().cpu() - pn64).abs() / pn64).max().item()
    e_grad = (g.double().cpu() - (g0.double().cpu() + g64)).abs().max().item() / g64.abs().max().item()
    print(f'pn prior {shape}: loss rel err {e_loss:.2e} (restatement {e_loss_r:.2e}, bar {bar_loss:.1e}); gradient err {e_grad:.2e} of max '
          f'(restatement {e_grad_r:.2e}, bar {bar_grad:.1e}); pn {pn64.tolist()}')
    assert e_loss <= bar_loss and e_grad <= bar_grad
    assert not torch.equal(g, g0) and torch.isfinite(g).all()
    # forward only: the same loss bits, nothing else needed
    assert torch.equal(ops.pn_prior_loss_grad(wd, st.mean, st.matrix), loss)
    # twice: the same bits, with a caller's partial-sum buffer as well
    g2, part = g0.clone(), ops.pn_prior_parts(B, L, dev)
    assert part.shape == (B, L) and part.dtype == torch.float64
    assert torch.equal(ops.pn_prior_loss_grad(wd, st.mean, st.matrix, g2, weight, part=part), loss) and torch.equal(g2, g)
    # the table form writes row dev_t (clamped to the table) and no other
    table = torch.full((4, B), -1.0, device=dev)
    for row in (2, 9):
        g3 = g0.clone()
        assert ops.pn_prior_loss_grad(wd, st.mean, st.matrix, g3, weight, table=table, row_dev=_i32(row, dev), part=part) is None
        assert torch.equal(table[min(row, 3)], loss) and torch.equal(g3, g)
    assert torch.equal(table[:2], torch.full((2, B), -1.0, device=dev))
    out = torch.full((B,), -1.0, device=dev)
    assert ops.pn_prior_loss_grad(wd, st.mean, st.matrix, loss_out=out) is out and torch.equal(out, loss)
    # a (B, D) latent is one row per image
    if L == 1:
        assert torch.equal(ops.pn_prior_loss_grad(wd[:, 0].contiguous(), st.mean, st.matrix), loss)


def test_kernel_general_path_and_refusals(dev):
    """D % 4 == 0 with a matrix 4 bytes off a 16-byte boundary takes the element-by-element path: within the same bars of float64 (another
    summation order, not the same bits required).  Wrong shapes raise ValueError; a weight < 0 and D > 4096 are refused by the library."""
    from oodgan import _lib, ops
    shape, weight = (2, 3, 512), 1.0
    B, L, D = shape
    ref, st = _synthetic(D, dev)
    w = pn_ref.sample(ref, shape, seed=23)
    pn64, g64 = _float64(w, ref, weight)
    e_loss_r, e_grad_r = _restatement_errors(w, ref, weight, pn64, g64)
    buf = torch.zeros(D * D + 1, device=dev)
    buf[1:].copy_(st.matrix.reshape(-1))
    M1 = buf[1:].view(D, D)
    assert M1.data_ptr() % 16 == 4 and M1.is_contiguous()
    wd, g = w.to(dev), torch.zeros(shape, device=dev)
    loss = ops.pn_prior_loss_grad(wd, st.mean, M1, g, weight)
    e_loss = ((loss.double().cpu() - pn64).abs() / pn64).max().item()
    e_grad = (g.double().cpu() - g64).abs().max().item() / g64.abs().max().item()
    print(f'pn prior {shape}, unaligned matrix: loss rel err {e_loss:.2e} (restatement {e_loss_r:.2e}); gradient err {e_grad:.2e} (restatement {e_grad_r:.2e})')
    assert e_loss <= max(1e-6, 4 * e_loss_r) and e_grad <= max(1e-6, 4 * e_grad_r)
    for bad_mu, bad_M in ((st.mean[:-1].contiguous(), st.matrix), (st.mean, st.matrix[:, :-1].contiguous()), (st.mean, st.matrix[:-1].contiguous())):
        with pytest.raises(ValueError, match='pn_prior_loss_grad'):
            ops.pn_prior_loss_grad(wd, bad_mu, bad_M)
    with pytest.raises(ValueError, match='pn_prior_loss_grad'):
        ops.pn_prior_loss_grad(wd[0, 0].contiguous(), st.mean, st.matrix)
    lib, n0 = _lib.lib(), _lib.dispatch_count('pn')
    out, part = torch.full((B,), -1.0, device=dev), ops.pn_prior_parts(B, L, dev)
    p = ops._p
    assert lib.oodgan_pn_prior_fwd_bwd(p(wd), p(st.mean), p(st.matrix), None, p(out), B, L, D, -1.0, p(part), ops._stream()) == -1
    assert b'pn_prior' in lib.oodgan_last_error()
    assert lib.oodgan_pn_prior_fwd_bwd(p(wd), p(st.mean), p(st.matrix), None, p(out), B, L, 4100, 1.0, p(part), ops._stream()) == -1
    assert lib.oodgan_pn_prior_fwd_bwd(p(wd), p(st.mean), p(st.matrix), None, p(out), B, L, D, 1.0, None, ops._stream()) == -1
    torch.cuda.synchronize()
    assert (out == -1.0).all() and _lib.dispatch_count('pn') == n0           # refused before anything is launched or counted


# ------------------------------------------------------------------------------------------------------------- the statistics
def test_generator_pn_stats(dev):
    """``Generator.pn_stats(n=4096, seed=3, floor=1e-4)`` on a seeded generator: the mean against the yardstick's (float64 sums of the same
    HIP mapping outputs in another order: 1e-10 absolute covers 4096 values of |x| < 100 at 2^-53 each many times over); pn_b of 8 probe latents
    through ``stats.matrix`` on the kernel against the yardstick's float64 statistics, bar as in test_kernel_vs_float64 — the quadratic form,
    never the eigenvectors.  The floor keeps the comparison off eigenvalues at the fp32 mapping's noise level.  Cached per mapping weights."""
    from oodgan import ops
    from oodgan.modules import Generator
    from oodgan.pn import PNStats
    size = 64
    G = Generator(size, 512, 8)
    G.load_state_dict(synth.generator_state(size, seed=5), strict=True)
    G = G.to(dev).eval()
    st = G.pn_stats(n=4096, seed=3, floor=1e-4)
    assert isinstance(st, PNStats) and (st.n, st.seed, st.floor) == (4096, 3, 1e-4)
    assert st.mean.device.type == 'cuda' and st.matrix.shape == (512, 512) and st.matrix.dtype == torch.float32
    assert G.pn_stats(n=4096, seed=3, floor=1e-4) is st                                  # cached
    with torch.no_grad():
        ref = pn_ref.stats(G.style, 512, 4096, seed=3, floor=1e-4, device=dev)
    e_mean = (st.mean64 - ref['mean']).abs().max().item()
    assert e_mean <= 1e-10
    ratio = (ref['variance'].max() / ref['variance'].min()).item()
    assert abs(ratio - 1e4) <= 1e-6 * 1e4                                               # the floor is active
    w = pn_ref.sample(ref, (8, 10, 512), seed=29)
    pn64, g64 = _float64(w, ref, 1.0)
    e_loss_r, _ = _restatement_errors(w, ref, 1.0, pn64, g64)
    got = ops.pn_prior_loss_grad(w.to(dev), st.mean, st.matrix)
    e = ((got.double().cpu() - pn64).abs() / pn64).max().item()
    e_host = ((st.distance(w) - pn64).abs() / pn64).max().item()
    print(f'Generator.pn_stats(4096, 3, 1e-4): |mean - yardstick| {e_mean:.2e}; pn of 8 probes rel err {e:.2e} (restatement {e_loss_r:.2e}, '
          f'bar {max(1e-6, 4 * e_loss_r):.1e}); PNStats.distance rel err {e_host:.2e}; variance max/min {ratio:.3e}')
    # the host form on the module's own float64 statistics: the two float64 sums differ in order, n * 2^-53 of the largest variance, 1e-4 of
    # which is the smallest kept one — 5e-9 of that; 1e-7 covers it
    assert e <= max(1e-6, 4 * e_loss_r) and e_host <= 1e-7
    # other mapping weights miss the cache
    with torch.no_grad():
        G.style[1].bias.add_(0.25)
    st2 = G.pn_stats(n=4096, seed=3, floor=1e-4)
    assert st2 is not st and not torch.equal(st2.mean64, st.mean64) and G.pn_stats(n=4096, seed=3, floor=1e-4) is st2
    # n <= D without a floor: refused, naming both options
    with pytest.raises(ValueError, match=r'pn_samples.*pn_floor'):
        G.pn_stats(n=256, seed=0)


# ------------------------------------------------------------------------------------------------------------- the latent side
_ADAM = dict(total=6, up=0.34, down=0.5, lr=0.01)


@pytest.mark.parametrize('mode', ['plain', 'w', 'layer_lr', 'latent_reg'])
@pytest.mark.parametrize('shape', [(2, 18, 512), (1, 4, 37)])
def test_latent_side_vs_float64_adam(dev, shape, mode):
    """Six steps of the latent side alone, the calls in the loop's order — [latent prior,] P_N+ prior, then the latent step or the scheduled
    Adam — on the synthetic gradients of tests/test_hip_latent_controls.py, against torch.optim.Adam in float64 with lambda * pn_b (and the
    prior) in the loss.  lambda is set from the yardstick so that the term's largest gradient entry at the start is 1e-2: a tenth of the
    first synthetic gradient's scale, ten times the smallest's.  Bar: w within 1e-6 max(1, max|w|), as for the other latent-side kernels."""
    from oodgan import ops
    B, L, D = shape
    total, up, down, lr = _ADAM['total'], _ADAM['up'], _ADAM['down'], _ADAM['lr']
    ref, st = _synthetic(D, dev)
    tied, reg = mode == 'w', 0.5 if mode == 'latent_reg' else 0.0
    rates = [((l + 1) % 4) * 0.5 for l in range(L)] if mode == 'layer_lr' else None     # 0.5, 1, 1.5, 0 (frozen), ...
    w0 = pn_ref.sample(ref, shape, seed=31)
    if tied:
        w0 = w0[:, :1].expand(shape).contiguous()
    _, g_start = _float64(w0, ref, 1.0)
    lam = 1e-2 / g_start.abs().max().item()
    anchor = (w0 + 0.1 * synth.normal('pn.anchor', shape, 5)).contiguous()
    if tied:
        leaves = [w0[:, 0].double().clone().requires_grad_(True)]
        opt = torch.optim.Adam(leaves, lr=lr, betas=(0.9, 0.999), eps=1e-8)
    else:
        leaves = [w0[:, l].double().clone().requires_grad_(True) for l in range(L)]
        opt = torch.optim.Adam([dict(params=[p]) for p in leaves], lr=lr, betas=(0.9, 0.999), eps=1e-8)
    wd = w0.clone().to(dev)
    m, v, t = torch.zeros_like(wd), torch.zeros_like(wd), _i32(0, dev)
    rd = None if rates is None else torch.tensor(rates, dtype=torch.float32, device=dev)
    table, part = torch.full((total, B), -1.0, device=dev), ops.pn_prior_parts(B, L, dev)
    worst_w = worst_pn = 0.0
    for i in range(total):
        gr = synth.normal(f'ad.g{i}', shape, 4) * (10.0 ** (-(i % 3) - 1))
        for k, grp in enumerate(opt.param_groups):
            grp['lr'] = lr * lr_multiplier(i, total, up, down) * (1.0 if rates is None else rates[k])
        opt.zero_grad(set_to_none=True)
        w = leaves[0][:, None, :].expand(shape) if tied else torch.stack(leaves, 1)
        pn = pn_ref.term(w, ref)
        loss = (gr.double() * w).sum() + lam * pn.sum()
        if reg:
            loss = loss + reg * ((w - anchor.double()) ** 2).mean(dim=(1, 2)).sum()
        loss.backward()
        opt.step()
        g = gr.to(dev)
        if reg:
            ops.latent_prior_loss_grad(wd, anchor.to(dev), g, reg)
        ops.pn_prior_loss_grad(wd, st.mean, st.matrix, g, lam, table=table, row_dev=t, part=part)
        if tied or rd is not None:
            ops.latent_step(wd, g, m, v, t, total, up, down, lr, layer_lr=rd, tied=tied)
        else:
            ops.adam_step_dev_sched(wd, g, m, v, t, total, up, down, lr)
        w_ref = (leaves[0][:, None, :].expand(shape) if tied else torch.stack(leaves, 1)).detach()
        e_w = (wd.double().cpu() - w_ref).abs().max().item() / max(1.0, w_ref.abs().max().item())
        e_pn = ((table[i].double().cpu() - pn.detach()).abs() / pn.detach()).max().item()
        print(f'latent side {shape} {mode} step {i}: w err {e_w:.2e} (bar 1e-6), pn rel err {e_pn:.2e}, lambda {lam:.2e}')
        worst_w, worst_pn = max(worst_w, e_w), max(worst_pn, e_pn)
        assert int(t.item()) == i + 1
    assert worst_w <= 1e-6
    assert worst_pn <= 1e-4                     # each step's row, from that step's fp32 w against the float64 leaf's: a check of the row, not the kernel's bar
    assert (table >= 0).all() and not torch.equal(wd.cpu(), w0)
    if tied:
        assert torch.equal(wd, wd[:, :1].expand_as(wd))
    for l in [l for l, r in enumerate(rates or []) if r == 0.0]:
        assert torch.equal(wd[:, l].cpu(), w0[:, l])


# ------------------------------------------------------------------------------------------------------------- the loop
def _counters():
    from oodgan import _lib
    return {c: _lib.dispatch_count(c) for c in C.COUNTERS + ('pooled_pixel', 'pn')}


def test_loop_plans_streams_and_the_default_path(dev):
    from oodgan import _lib
    from oodgan.engine import WPlusInverter
    size, B, steps, lam = 64, 3, 12, 1e-3
    eng = S._engine(dev, size)
    x, w0, noises = S._hip_inputs(dev, size, B)
    _, st = _synthetic(512, dev)
    w0 = pn_ref.sample(_synthetic(512, dev)[0], tuple(w0.shape), seed=37).to(dev)
    # off: the bits, the launch count and the dispatch counters of a run without the option
    _lib.dispatch_reset()
    base = WPlusInverter(eng)
    w_b, l_b = base.invert(x, w0, noises, steps=steps)
    torch.cuda.synchronize()
    c_b = _counters()
    assert base.last_terms['pn'] is None and c_b['pn'] == 0
    _lib.dispatch_reset()
    off = WPlusInverter(eng, pn_reg=0.0)
    w, l = off.invert(x, w0, noises, steps=steps, pn_stats=st)
    torch.cuda.synchronize()
    assert torch.equal(w, w_b) and torch.equal(l, l_b) and off.last_plan == base.last_plan and off.last_stats == base.last_stats
    assert _counters() == c_b and off.last_terms['pn'] is None
    # on: plan and no plan bit for bit, two launches more per recorded step, the loss row the sum of its terms
    inv = WPlusInverter(eng, use_plan=True, pn_reg=lam)
    w1, l1 = inv.invert(x, w0, noises, steps=steps, pn_stats=st)
    t1 = inv.last_terms
    assert inv.last_plan['steps'] == [steps - 3] and inv.last_stats['rollbacks'] == [0]
    assert inv.last_plan['launches'] == [base.last_plan['launches'][0] + 2]
    assert t1['pn'].shape == (steps, B) and (t1['pn'] > 0).all() and torch.equal(l1, t1['mse'] + lam * t1['pn'])
    assert not torch.equal(w1, w_b) and torch.isfinite(w1).all()
    want = _synthetic(512, dev)[1].distance(w0)
    assert ((t1['pn'][0].double().cpu() - want).abs() / want).max().item() <= 1e-5         # the first row is pn of the start latents
    assert (t1['pn'][-1] < t1['pn'][0]).all()                                              # and the term pulls
    pn1 = t1['pn'].clone()
    inv2 = WPlusInverter(eng, use_plan=False, pn_reg=lam)
    w2, l2 = inv2.invert(x, w0, noises, steps=steps, pn_stats=st)
    assert inv2.last_plan['steps'] == [0]
    assert torch.equal(w1, w2) and torch.equal(l1, l2) and torch.equal(pn1, inv2.last_terms['pn'])
    # two streams: the bars of tests/test_hip_wplus_sched.py::test_plans_streams_and_trajectory; the statistics are shared
    w3, l3 = inv.invert(x, w0, noises, steps=steps, streams=2, pn_stats=st)
    rel0 = (l3[0] - l1[0]).abs().max().item() / l1[0].abs().max().item()
    rel = (l3 - l1).abs().max().item() / l1.abs().max().item()
    frac = ((w3 - w1).abs() < 5e-4).float().mean().item()
    print(f'pn_reg {lam}: 2 streams vs 1 at 64², B={B}: loss rel diff step 1 {rel0:.2e}, all steps {rel:.2e}, {100 * frac:.3f}% of w within 5e-4; '
          f'plan {inv.last_plan}; pn {pn1[0].tolist()} -> {pn1[-1].tolist()}')
    assert rel0 <= 1e-5 and rel <= 1e-3 and frac > 0.999
    assert inv.last_plan['steps'] == [steps - 3] * 2 and inv.last_terms['pn'].shape == (steps, B)
    assert torch.equal(l3, inv.last_terms['mse'] + lam * inv.last_terms['pn'])
    # with the W tie, the schedule and the prior: composes, rows identical
    inv4 = WPlusInverter(eng, pn_reg=lam, latent_space='w', **S._OPT)
    w4, l4 = inv4.invert(x, w0, noises, steps=steps, pn_stats=st, latent_anchor=w0)
    t4 = inv4.last_terms
    assert torch.equal(w4, w4[:, :1].expand_as(w4)) and torch.equal(l4, t4['mse'] + S._OPT['latent_reg'] * t4['latent'] + lam * t4['pn'])
    # a trajectory run takes the term too
    w5, l5, traj = WPlusInverter(eng, pn_reg=lam).invert(x, w0, noises, steps=4, return_trajectory=True, pn_stats=st)
    assert len(traj) == 4 and torch.equal(traj[-1], w5) and torch.equal(l5, l1[:4])


def test_loop_refusals(dev):
    from oodgan.engine import WPlusInverter
    from oodgan.pn import PNStats
    size, B = 64, 2
    eng = S._engine(dev, size)
    x, w0, noises = S._hip_inputs(dev, size, B)
    ref, st = _synthetic(512, dev)
    with pytest.raises(NotImplementedError, match='pn_reg'):
        WPlusInverter(eng, pn_reg=1e-3).invert(x, w0, noises, steps=2, use_graph=True, pn_stats=st)
    with pytest.raises(ValueError, match=r"pn_reg.*latent_space 's'"):
        WPlusInverter(eng, pn_reg=1e-3, latent_space='s')
    with pytest.raises(ValueError, match='pn_reg > 0 needs pn_stats'):
        WPlusInverter(eng, pn_reg=1e-3).invert(x, w0, noises, steps=2)
    cpu = PNStats(ref['mean'], ref['components'], ref['variance'], 0, 0, 0.0)
    with pytest.raises(ValueError, match='pn_stats must be on'):
        WPlusInverter(eng, pn_reg=1e-3).invert(x, w0, noises, steps=2, pn_stats=cpu)
    assert cpu.to(dev).mean.device == w0.device and cpu.to(dev).mean64 is cpu.mean64
    narrow = _synthetic(37, dev)[1]
    with pytest.raises(ValueError, match='pn_stats must hold'):
        WPlusInverter(eng, pn_reg=1e-3).invert(x, w0, noises, steps=2, pn_stats=narrow)
    # a graph run without the option is untouched by it
    w, l = WPlusInverter(eng, pn_reg=0.0).invert(x, w0, noises, steps=3, use_graph=True, pn_stats=st)
    assert torch.isfinite(l).all()


# ------------------------------------------------------------------------------------------------------------- against the reference
def test_20_steps_vs_the_reference_loop(dev):
    """tests/golden/wplus_pn.npz (make_wplus_pn.py): the reference ``Generator``'s autograd + torch.optim.Adam, 20 steps at 64², B = 2,
    lambda = 1e-3, statistics from tests/pn_ref.py on the reference's own mapping network (n = 4096, seed 3, floor 1e-4), in fp32 and
    float64.  Here the statistics are rebuilt with pn_ref from the same seeded weights on the oracle's mapping network and passed as
    ``pn_stats``.  The loss curve stays within the project's 1e-3 bar of the float64 curve."""
    from oodgan.engine import GeneratorEngine, WPlusInverter
    from oodgan.pn import PNStats
    gold = np.load(GOLD)
    size, B, steps, lam = 64, 2, int(gold['steps']), float(gold['pn_reg'])
    seeds = dict(zip(('weights', 'x', 'noise', 'w0'), gold['seeds'].tolist()))
    P = synth.generator_state(size, seed=seeds['weights'])
    with torch.no_grad():
        ref = pn_ref.stats(lambda z: R.mapping_network(P, z), 512, int(gold['stats_n']), seed=int(gold['stats_seed']), floor=float(gold['stats_floor']))
    assert np.abs(ref['mean'][:8].numpy() - gold['stats_mean_head']).max() <= 1e-6          # the fixture's statistics, rebuilt
    assert np.abs(np.array([ref['variance'].min().item(), ref['variance'].max().item()]) / gold['stats_var_minmax'] - 1).max() <= 1e-5
    st = PNStats(ref['mean'], ref['components'], ref['variance'], int(gold['stats_n']), int(gold['stats_seed']), float(gold['stats_floor']), dev)
    eng = GeneratorEngine({k: v.to(dev) for k, v in P.items()}, size)
    x = synth.make_images(size, B, seed=seeds['x']).to(dev)
    noises = [n.to(dev) for n in synth.make_noises(size, B, seed=seeds['noise'])]
    w0 = synth.make_latents(size, B, seed=seeds['w0']).to(dev)
    inv = WPlusInverter(eng, lr=0.01, pn_reg=lam)
    w, losses, traj = inv.invert(x, w0, noises, steps=steps, return_trajectory=True, pn_stats=st)
    l64, p64 = torch.from_numpy(gold['losses_f64']), torch.from_numpy(gold['pn_f64'])
    e_curve = ((losses.double().cpu() - l64).abs() / l64).max().item()
    e_pn = ((inv.last_terms['pn'].double().cpu() - p64).abs() / p64).max().item()
    e_w = {t: (traj[t - 1].cpu() - torch.from_numpy(gold[f'w_step{t}'])).abs().max().item() for t in (1, 10, 20)}
    print(f"20 steps 64² with pn_reg {lam}: loss curve rel {e_curve:.2e} vs the reference's float64 loop (its own fp32 loop: {float(gold['ref_f32_vs_f64']):.2e}); "
          f'pn table rel {e_pn:.2e}; max |w - reference fp32| after steps 1, 10, 20: {e_w}; stats {inv.last_stats}')
    assert e_curve <= 1e-3 and e_pn <= 1e-3
    # Adam's first steps move every coordinate by ~lr * sign(g): a coordinate whose gradient is ~0 may take the other sign (smoke()'s rule)
    for t in (1, 10, 20):
        assert ((traj[t - 1].cpu() - torch.from_numpy(gold[f'w_step{t}'])).abs() < 2e-3).float().mean().item() > 0.999
    assert inv.last_stats == {'steps_run': [steps], 'rollbacks': [0]}
    # the plan run of the same call: its losses, bit for bit
    w_p, l_p = inv.invert(x, w0, noises, steps=steps, pn_stats=st)
    assert torch.equal(l_p, losses) and torch.equal(w_p, w)


# ------------------------------------------------------------------------------------------------------------- model level
def test_model_invert_with_pn_reg(dev):
    size, B, steps = 64, 2, 4
    m = S._model_64(dev)
    x = synth.make_images(size, B, seed=44).to(dev)
    kw = dict(enc_lats=synth.make_latents(size, B, seed=42, std=0.3).to(dev), noise=[n.to(dev) for n in synth.make_noises(size, B, seed=45)])
    out0, lats0, l0 = m.invert(x, steps=steps, **kw)
    assert m.last_loss_terms['pn'] is None and m.last_pn_stats is None
    out, lats, l = m.invert(x, steps=steps, pn_reg=1e-3, pn_samples=4096, **kw)
    t = m.last_loss_terms
    st = m.generator.pn_stats(4096, 0, 0.0)
    assert m.last_pn_stats is st and (st.n, st.seed, st.floor) == (4096, 0, 0.0)
    assert t['pn'].shape == (steps, B) and torch.isfinite(l).all() and torch.isfinite(out).all() and torch.equal(l, t['mse'] + 1e-3 * t['pn'])
    assert not torch.equal(lats, lats0)
    w_start = m.encode(x, **kw)[0]
    want = st.distance(w_start)
    assert ((t['pn'][0].double().cpu() - want).abs() / want).max().item() <= 1e-5
    # the explicit statistics win over the three parameters, and give the same run
    out2, lats2, l2 = m.invert(x, steps=steps, pn_reg=1e-3, pn_samples=7, pn_seed=9, pn_floor=0.5, pn_stats=st, **kw)
    assert torch.equal(out2, out) and torch.equal(lats2, lats) and torch.equal(l2, l) and m.last_pn_stats is st
    # other parameters: other statistics, another run
    out3, lats3, l3 = m.invert(x, steps=steps, pn_reg=1e-3, pn_samples=4096, pn_floor=1e-2, **kw)
    assert m.last_pn_stats.floor == 1e-2 and not torch.equal(l3, l)
    for bad, name in ((dict(pn_reg=-1.0), 'pn_reg'), (dict(pn_reg=float('nan')), 'pn_reg'), (dict(pn_reg=0.1, pn_samples=1), 'pn_samples'),
                      (dict(pn_reg=0.1, pn_seed=-1), 'pn_seed'), (dict(pn_reg=0.1, pn_floor=-1.0), 'pn_floor'),
                      (dict(pn_reg=0.1, latent_space='s'), 'latent_space'), (dict(pn_reg=0.1, pn_stats='x'), 'pn_stats'),
                      (dict(pn_reg=0.1, pn_samples=256), 'pn_floor')):
        with pytest.raises(ValueError, match=name):
            m.invert(x, steps=2, **bad, **kw)
    with pytest.raises(NotImplementedError, match='pn_reg'):
        m.invert(x, steps=2, use_graph=True, pn_reg=0.1, pn_samples=4096, **kw)
