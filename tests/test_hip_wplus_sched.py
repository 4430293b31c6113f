"""The projector schedule of the W+ loop (csrc/wplus_sched.hip): learning-rate ramps, latent noise, latent prior.

The three kernels against float64 (the noise against tests/latent_noise_ref.py, which tests/test_wplus_sched_cpu.py pins to Philox's known
answers); a short run against the oracle's float64 Adam loop with the same schedule; the untouched default path; launch plans, streams, the
range guard's rollback; the model-level arguments; one step at 1024²."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import ref_cpu as R  # noqa: E402
from oodgan import synth  # noqa: E402
from oodgan.ops import lr_multiplier  # noqa: E402
import latent_noise_ref as N  # noqa: E402


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


def _i32(v, dev):
    return torch.tensor([v], dtype=torch.int32, device=dev)


def _i64(v, dev):
    return torch.tensor(list(v), dtype=torch.int64, device=dev)


# ------------------------------------------------------------------------------------------------------------- kernels
@pytest.mark.parametrize('step', [0, 7])
@pytest.mark.parametrize('n', [5120, 9216, 37])
@pytest.mark.parametrize('ids', [[5], [0, 2 ** 33 + 1, 7]])
def test_noise_kernel_vs_float64(dev, ids, n, step):
    """|w_in - w - sigma_i n_ref| <= 1e-5 sigma_0.  |n| <= 5.9 by construction; the kernel takes the logarithm and the sine / cosine in double
    and rounds n once (4e-7 at most); what remains is the fp32 rounding of the sum w + sigma n, half an ulp of |w_in| < 8: 4.8e-7 — here
    sigma_0 = 0.5 against latents of unit scale, so the bar (5e-6) is ten times that."""
    from oodgan import ops
    B, total, sigma0, ramp, seed = len(ids), 20, 0.5, 0.75, 3
    w = synth.normal('sched.w', (B, n), 21).to(dev)
    t_dev, idt = _i32(step, dev), _i64(ids, dev)
    w_in = ops.latent_noise(w, t_dev, idt, total, sigma0, ramp, seed)
    assert int(t_dev.item()) == step                    # read, not incremented
    ref = N.latent_noise(seed, ids, step, n, total, sigma0, ramp)
    assert N.sigma(step, total, sigma0, ramp) > 0
    err = np.abs(w_in.double().cpu().numpy() - w.double().cpu().numpy() - ref).max()
    print(f'latent noise B={B} n={n} step {step}: sigma_i {N.sigma(step, total, sigma0, ramp):.4f}, max |w_in - w - sigma n_ref| = {err:.2e} '
          f'(bar {1e-5 * sigma0:.1e})')
    assert err <= 1e-5 * sigma0
    # two identical calls are bit-equal; a caller's buffer receives the same bits
    out = torch.full_like(w, float('nan'))
    assert ops.latent_noise(w, t_dev, idt, total, sigma0, ramp, seed, out=out) is out and torch.equal(out, w_in)
    # an image's draws depend on its id, not on its place in the batch or on the batch
    if B == 3:
        one = ops.latent_noise(w[2:3].contiguous(), t_dev, _i64([7], dev), total, sigma0, ramp, seed)
        assert torch.equal(one, w_in[2:3])
    # sigma_i == 0 (tau >= noise_ramp): w_in = w bit for bit
    assert N.sigma(15, total, sigma0, ramp) == 0.0
    assert torch.equal(ops.latent_noise(w, _i32(15, dev), idt, total, sigma0, ramp, seed), w)
    # noise_ramp <= 0: constant strength
    c = ops.latent_noise(w, _i32(15, dev), idt, total, sigma0, 0.0, seed)
    assert np.abs(c.double().cpu().numpy() - w.double().cpu().numpy() - N.latent_noise(seed, ids, 15, n, total, sigma0, 0.0)).max() <= 1e-5 * sigma0
    # another seed, another step: other draws
    assert not torch.equal(ops.latent_noise(w, t_dev, idt, total, sigma0, ramp, seed + 1), w_in)
    assert not torch.equal(ops.latent_noise(w, _i32(step + 1, dev), idt, total, sigma0, 0.0, seed), ops.latent_noise(w, t_dev, idt, total, sigma0, 0.0, seed))


def test_noise_kernel_unaligned_pointers_take_the_scalar_path(dev):
    """n a multiple of 4 but the tensors 4 bytes off a 16-byte boundary: the same bits as the vector path."""
    from oodgan import ops
    B, n = 2, 512
    w = synth.normal('sched.w', (B, n), 22).to(dev)
    t_dev, ids = _i32(2, dev), _i64([4, 9], dev)
    want = ops.latent_noise(w, t_dev, ids, 10, 0.5, 0.75, 1)
    buf, obuf = torch.zeros(B * n + 1, device=dev), torch.zeros(B * n + 1, device=dev)
    buf[1:].copy_(w.reshape(-1))
    src, dst = buf[1:].view(B, n), obuf[1:].view(B, n)
    assert src.data_ptr() % 16 == 4 and src.is_contiguous()
    ops.latent_noise(src, t_dev, ids, 10, 0.5, 0.75, 1, out=dst)
    assert torch.equal(dst, want) and obuf[0].item() == 0.0


def test_scheduled_adam_vs_float64(dev):
    from oodgan import ops
    shape, total, up, down, lr = (2, 18, 512), 6, 0.34, 0.5, 0.01
    w0 = synth.normal('ad.w', shape, 3)
    w = w0.double().clone().requires_grad_(True)
    opt = torch.optim.Adam([w], lr=lr, betas=(0.9, 0.999), eps=1e-8)
    wd = w0.clone().to(dev)
    m, v, t = torch.zeros_like(wd), torch.zeros_like(wd), _i32(0, dev)
    # both ramps off: the same bits as adam_step_dev
    wp, wq = w0.clone().to(dev), w0.clone().to(dev)
    mp, vp, tp, mq, vq, tq = torch.zeros_like(wd), torch.zeros_like(wd), _i32(0, dev), torch.zeros_like(wd), torch.zeros_like(wd), _i32(0, dev)
    for i in range(total):
        gr = synth.normal(f'ad.g{i}', shape, 4) * (10.0 ** (-(i % 3) - 1))
        opt.param_groups[0]['lr'] = lr * lr_multiplier(i, total, up, down)
        w.grad = gr.double().clone()
        opt.step()
        ops.adam_step_dev_sched(wd, gr.to(dev), m, v, t, total, up, down, lr)
        err = (wd.double().cpu() - w.detach()).abs().max().item()
        print(f'scheduled Adam step {i}: lr factor {lr_multiplier(i, total, up, down):.4f}, max |w - float64| = {err:.2e}')
        assert err <= 1e-6 * max(1.0, w.detach().abs().max().item())
        assert int(t.item()) == i + 1
        if i == 0:          # lr_0 = 0: the first step only fills the moments
            assert lr_multiplier(0, total, up, down) == 0.0 and torch.equal(wd.cpu(), w0) and (m != 0).any() and (v != 0).any()
        ops.adam_step_dev_sched(wp, gr.to(dev), mp, vp, tp, total, 0.0, 0.0, lr)
        ops.adam_step_dev(wq, gr.to(dev), mq, vq, tq, lr)
        assert torch.equal(wp, wq) and torch.equal(mp, mq) and torch.equal(vp, vq) and torch.equal(tp, tq)
    assert not torch.equal(wd, wq)
    # the moments do not know about the schedule
    assert torch.equal(m, mq) and torch.equal(v, vq)


@pytest.mark.parametrize('shape,batched', [((3, 10, 512), False), ((3, 10, 512), True), ((2, 37), False), ((1, 18, 512), True)])
def test_prior_kernel_vs_float64(dev, shape, batched):
    """Bars: loss 1e-6 relative (the kernel sums in double and rounds once), gradient 1e-6 of its maximum (two fp32 roundings)."""
    from oodgan import ops
    B, weight = shape[0], 0.7
    w = synth.normal('prior.w', shape, 31)
    a = synth.normal('prior.a', shape if batched else shape[1:], 32, 0.5)
    d = w.double() - a.double()
    dims = tuple(range(1, len(shape)))
    loss_ref = (d ** 2).mean(dim=dims)
    g_ref = weight * 2.0 * d / (d.numel() // B)
    wd, ad = w.to(dev), a.to(dev)
    z = torch.zeros_like(wd)
    loss = ops.latent_prior_loss_grad(wd, ad, z, weight)
    e_loss = ((loss.double().cpu() - loss_ref).abs() / loss_ref).max().item()
    e_g = (z.double().cpu() - g_ref).abs().max().item() / g_ref.abs().max().item()
    print(f'latent prior {shape} anchor per image {batched}: loss rel err {e_loss:.2e}, gradient err {e_g:.2e} of max (bars 1e-6)')
    assert e_loss <= 1e-6 and e_g <= 1e-6
    # accumulated into a non-zero g, not written over it: g = g0 + z up to one rounding of the sum
    g0 = synth.normal('prior.g0', shape, 33).to(dev) * z.abs().max()
    g = g0.clone()
    assert torch.equal(ops.latent_prior_loss_grad(wd, ad, g, weight), loss)
    assert (g - (g0 + z)).abs().max().item() <= 1e-6 * (g0.abs().max().item() + z.abs().max().item())
    assert not torch.equal(g, z)
    # forward only: the same value; the table form writes row row_dev[0] (clamped to the table) and nothing else
    assert torch.equal(ops.latent_prior_loss_grad(wd, ad), loss)
    table = torch.full((4, B), -1.0, device=dev)
    for row in (2, 9):
        z3 = torch.zeros_like(z)
        assert ops.latent_prior_loss_grad(wd, ad, z3, weight, table=table, row_dev=_i32(row, dev)) is None
        assert torch.equal(table[min(row, 3)], loss) and torch.equal(z3, z)
    assert torch.equal(table[:2], torch.full((2, B), -1.0, device=dev))
    with pytest.raises(ValueError, match='anchor'):
        ops.latent_prior_loss_grad(wd, ad.reshape(-1)[:5].contiguous())


# ------------------------------------------------------------------------------------------------------- the loop
_RUN = dict(size=64, B=3, steps=20, lr=0.01)
_OPT = dict(lr_rampup=0.1, lr_rampdown=0.3, latent_noise=0.05, noise_ramp=0.5, latent_reg=0.5)
_ORACLE = {}


def _inputs(size, B):
    return (synth.generator_state(size, seed=5), synth.make_images(size, B, seed=9), synth.make_noises(size, B, seed=7),
            synth.make_latents(size, B, seed=14))


def _oracle_run(dt):
    """The oracle's autograd + torch.optim.Adam loop with the schedule of ``_OPT`` in dtype ``dt`` (the lr set per step, the latent noise of
    tests/latent_noise_ref.py, the prior towards the start latents added to the loss): (total losses[steps,B], prior tables)."""
    if dt not in _ORACLE:
        size, B, steps, lr = _RUN['size'], _RUN['B'], _RUN['steps'], _RUN['lr']
        P, x, noises, w0 = _inputs(size, B)
        P, x, noises, w0 = {k: v.to(dt) for k, v in P.items()}, x.to(dt), [n.to(dt) for n in noises], w0.to(dt)
        w = w0.clone().requires_grad_(True)
        opt = torch.optim.Adam([w], lr=lr, betas=(0.9, 0.999), eps=1e-8)
        tot, pri = [], []
        for i in range(steps):
            opt.param_groups[0]['lr'] = lr * lr_multiplier(i, steps, _OPT['lr_rampup'], _OPT['lr_rampdown'])
            opt.zero_grad(set_to_none=True)
            nz = N.latent_noise(0, range(B), i, w0[0].numel(), steps, _OPT['latent_noise'], _OPT['noise_ramp'])
            img = R.generator_forward(P, w + torch.from_numpy(nz).to(dt).reshape(w.shape), noises, size)
            p = ((w - w0) ** 2).mean(dim=(1, 2))
            t = ((img - x) ** 2).mean(dim=(1, 2, 3)) + _OPT['latent_reg'] * p
            t.sum().backward()
            tot.append(t.detach().clone())
            pri.append(p.detach().clone())
            opt.step()
        _ORACLE[dt] = (torch.stack(tot).double(), torch.stack(pri).double())
    return _ORACLE[dt]


def _engine(dev, size):
    from oodgan.engine import GeneratorEngine
    return GeneratorEngine({k: v.to(dev) for k, v in synth.generator_state(size, seed=5).items()}, size)


def _hip_inputs(dev, size, B):
    _, x, noises, w0 = _inputs(size, B)
    return x.to(dev), w0.to(dev), [n.to(dev) for n in noises]


def test_short_run_vs_the_oracle_loop(dev):
    """20 steps at 64², B=3, ramps + noise + prior towards the start latents: the total-loss curve within max(1e-3, 3x the oracle's own
    fp32-vs-float64 distance); the prior's table within 1e-5 absolute."""
    from oodgan.engine import WPlusInverter
    size, B, steps = _RUN['size'], _RUN['B'], _RUN['steps']
    l64, p64 = _oracle_run(torch.float64)
    l32, _ = _oracle_run(torch.float32)
    e_self = ((l32 - l64).abs() / l64).max().item()
    x, w0, noises = _hip_inputs(dev, size, B)
    inv = WPlusInverter(_engine(dev, size), lr=_RUN['lr'], **_OPT)
    w, losses = inv.invert(x, w0, noises, steps=steps, latent_anchor=w0)
    t = inv.last_terms
    e_curve = ((losses.double().cpu() - l64).abs() / l64).max().item()
    e_lat = (t['latent'].double().cpu() - p64).abs().max().item()
    print(f'20 steps 64² with the schedule: loss curve rel {e_curve:.2e} vs the float64 oracle loop (its own fp32 loop: {e_self:.2e}); '
          f'|prior table - oracle| {e_lat:.2e} (max prior {p64.max().item():.2e}); stats {inv.last_stats}, plan {inv.last_plan}')
    assert e_curve < max(1e-3, 3 * e_self)
    assert e_lat < 1e-5
    assert t['latent'].shape == (steps, B) and torch.equal(losses, t['mse'] + _OPT['latent_reg'] * t['latent'])
    assert not inv.engine.bwd_scale_violated() and not inv.engine.fwd_range_violated()
    assert inv.last_stats == {'steps_run': [steps], 'rollbacks': [0]}
    assert (t['latent'][0] == 0).all() and (t['latent'][-1] > 0).all()         # evaluated at w: zero at the start latents


def test_defaults_are_the_parent_path_and_each_option_moves_the_run(dev):
    from oodgan.engine import WPlusInverter
    size, B, steps = 64, 2, 8
    eng = _engine(dev, size)
    x, w0, noises = _hip_inputs(dev, size, B)
    base = WPlusInverter(eng)
    w_b, l_b = base.invert(x, w0, noises, steps=steps)
    n_b = base.last_plan['launches']
    assert base.last_terms['latent'] is None and n_b[0] > 0
    off = WPlusInverter(eng, lr_rampup=0.0, lr_rampdown=0.0, latent_noise=0.0, noise_ramp=0.75, noise_seed=0, latent_reg=0.0)
    w, l = off.invert(x, w0, noises, steps=steps, noise_ids=None, latent_anchor=None)
    assert torch.equal(w, w_b) and torch.equal(l, l_b) and off.last_plan['launches'] == n_b and off.last_terms['latent'] is None
    # the scheduled Adam replaces the plain one (two launches either way); the noise and the prior are one launch each
    for opt, extra in ((dict(lr_rampup=0.2), 0), (dict(lr_rampdown=0.3), 0), (dict(latent_noise=0.05), 1), (dict(latent_reg=0.5), 1)):
        inv = WPlusInverter(eng, **opt)
        w, l = inv.invert(x, w0, noises, steps=steps, latent_anchor=w0)
        assert torch.isfinite(w).all() and not torch.equal(w, w_b), opt
        assert inv.last_plan['launches'] == [n_b[0] + extra], (opt, inv.last_plan, n_b)
    # the seed and the ids select the draws; the default ids are arange(B)
    runs = {}
    for key, kw, ids in (('a', {}, None), ('b', {}, _i64([0, 1], dev)), ('c', {}, _i64([0, 5], dev)), ('d', dict(noise_seed=1), None)):
        runs[key] = WPlusInverter(eng, latent_noise=0.05, **kw).invert(x, w0, noises, steps=steps, noise_ids=ids)[0]
    assert torch.equal(runs['a'], runs['b']) and not torch.equal(runs['a'], runs['d']) and not torch.equal(runs['a'][1], runs['c'][1])
    # the refusals
    with pytest.raises(ValueError, match='latent_anchor'):
        WPlusInverter(eng, latent_reg=0.5).invert(x, w0, noises, steps=2)
    with pytest.raises(ValueError, match='latent_anchor'):
        WPlusInverter(eng, latent_reg=0.5).invert(x, w0, noises, steps=2, latent_anchor=w0[:, 0].contiguous())
    with pytest.raises(ValueError, match='noise_ids'):
        WPlusInverter(eng, latent_noise=0.05).invert(x, w0, noises, steps=2, noise_ids=torch.arange(B, device=dev, dtype=torch.int32))
    for opt in (dict(lr_rampup=0.2), dict(lr_rampdown=0.3), dict(latent_noise=0.05), dict(latent_reg=0.5)):
        with pytest.raises(NotImplementedError):
            WPlusInverter(eng, **opt).invert(x, w0, noises, steps=2, use_graph=True, latent_anchor=w0)


def test_plans_streams_and_trajectory(dev):
    from oodgan.engine import WPlusInverter
    size, B, steps = 64, 3, 12
    eng = _engine(dev, size)
    x, w0, noises = _hip_inputs(dev, size, B)
    anchor = (w0 + 0.1).contiguous()
    inv = WPlusInverter(eng, use_plan=True, **_OPT)
    w1, l1 = inv.invert(x, w0, noises, steps=steps, latent_anchor=anchor)
    p1 = inv.last_terms['latent'].clone()
    assert inv.last_plan['steps'] == [steps - 3] and inv.last_stats['rollbacks'] == [0]
    inv2 = WPlusInverter(eng, use_plan=False, **_OPT)
    w2, l2 = inv2.invert(x, w0, noises, steps=steps, latent_anchor=anchor)
    assert inv2.last_plan['steps'] == [0]
    assert torch.equal(w1, w2) and torch.equal(l1, l2) and torch.equal(p1, inv2.last_terms['latent']) and torch.equal(inv.last_terms['mse'], inv2.last_terms['mse'])
    # driven from Python with the trajectory kept: the same run
    w4, l4, traj = inv.invert(x, w0, noises, steps=steps, latent_anchor=anchor, return_trajectory=True)
    assert torch.equal(w4, w1) and torch.equal(l4, l1) and len(traj) == steps and torch.equal(traj[-1], w1)
    assert torch.equal(traj[0], w0)                                                # lr_0 = 0
    # two streams (sub-batches of 1 and 2 images, the anchor per image): the ids travel with the images; the bars of
    # tests/test_hip_generator.py::test_streams_vs_one_at_full_size
    seen = []
    inv.on_step = lambda run: seen.append(run.ids.clone()) if run.t == 1 else None
    w3, l3 = inv.invert(x, w0, noises, steps=steps, streams=2, latent_anchor=anchor.expand(B, -1, -1).contiguous())
    inv.on_step = None
    assert torch.equal(torch.cat(seen), torch.arange(B, device=dev)) and len(seen) == 2
    rel0 = (l3[0] - l1[0]).abs().max().item() / l1[0].abs().max().item()
    rel = (l3 - l1).abs().max().item() / l1.abs().max().item()
    frac = ((w3 - w1).abs() < 5e-4).float().mean().item()
    print(f'schedule on, 2 streams vs 1 at 64², B={B}: loss rel diff step 1 {rel0:.2e}, all steps {rel:.2e}, {100 * frac:.3f}% of w within 5e-4; '
          f'plan {inv.last_plan}')
    assert rel0 <= 1e-5 and rel <= 1e-3 and frac > 0.999
    assert inv.last_terms['latent'].shape == (steps, B) and inv.last_plan['steps'] == [steps - 3] * 2


@pytest.mark.parametrize('use_plan', [True, False])
def test_rollback_repeats_the_same_draws(dev, use_plan):
    """A forward scale sabotaged after step 15 of 40 (as tests/test_hip_ssim.py): one window is repeated with exact scales.  The noise of
    every step — w_in of the step minus w before it — is the reference's for (seed, id, step) in the first pass, in the repeated window and
    after it."""
    from oodgan.engine import WPlusInverter
    size, B, steps, sigma0, ramp, seed = 32, 2, 40, 0.05, 0.0, 2
    eng = _engine(dev, size)
    x, w0, noises = _hip_inputs(dev, size, B)
    inv = WPlusInverter(eng, use_plan=use_plan, lr_rampup=0.05, lr_rampdown=0.25, latent_noise=sigma0, noise_ramp=ramp, noise_seed=seed, latent_reg=0.5)
    ids = _i64([3, 2 ** 33 + 1], dev)
    rec, done = [], {'n': 0}

    def watch(run, fault):
        rec.append((run.t, run.w_in.clone(), run.w.clone()))
        if fault and run.steps_run == 15 and not done['n']:
            done['n'] = 1
            eng.fwd_range.q[3].mul_(2.0 ** 12)

    inv.on_step = lambda run: watch(run, False)
    w_ref, l_ref = inv.invert(x, w0, noises, steps=steps, noise_ids=ids, latent_anchor=w0)
    assert inv.last_stats == {'steps_run': [steps], 'rollbacks': [0]}
    clean, rec = rec, []
    inv.on_step = lambda run: watch(run, True)
    w, l = inv.invert(x, w0, noises, steps=steps, noise_ids=ids, latent_anchor=w0)
    inv.on_step = None
    assert inv.last_stats['rollbacks'] == [1] and inv.last_stats['steps_run'][0] == steps + inv.check_every + inv.check_lag
    assert torch.isfinite(w).all() and torch.isfinite(l).all() and torch.isfinite(inv.last_terms['latent']).all()
    n = w0[0].numel()
    want = {}

    def noise_err(records):
        worst, seen, top = 0.0, [], 0.0
        for (t0, _, w_before), (t1, w_in, _) in zip(records[:-1], records[1:]):
            if t1 != t0 + 1:
                continue            # the step after the rollback: w was restored in between
            i = t1 - 1              # the zero-based step: dev_t while it ran
            if i not in want:
                want[i] = N.latent_noise(seed, [3, 2 ** 33 + 1], i, n, steps, sigma0, ramp)
            got = (w_in.double() - w_before.double()).cpu().numpy().reshape(B, n)
            worst = max(worst, np.abs(got - want[i]).max())
            seen.append(i)
            top = max(top, w_in.abs().max().item())
        assert top < 8.0            # half an ulp of w_in is then <= 2.4e-7
        return worst, seen

    e_clean, s_clean = noise_err(clean)
    e_fault, s_fault = noise_err(rec)
    print(f'rollback with the schedule (plans {use_plan}): {inv.last_stats}; max |w_in - w - sigma n_ref| {e_clean:.2e} undisturbed, {e_fault:.2e} '
          f'with the repeated window (bar {1e-5 * sigma0 + 2.4e-7:.1e}); |loss - undisturbed| rel {((l - l_ref).abs() / l_ref).max().item():.2e}')
    assert s_clean == list(range(1, steps))
    # steps 11..21 ran twice (the window 10..20 and the two steps of the check's lag), and steps after the window are there
    assert sorted(set(s_fault)) == list(range(1, steps)) and all(s_fault.count(i) == 2 for i in range(11, 22)) and 24 in s_fault
    # the kernel's bar plus the fp32 rounding of w + sigma n at |w_in| < 8 (2.4e-7), which the difference w_in - w carries
    assert e_clean <= 1e-5 * sigma0 + 2.4e-7 and e_fault <= 1e-5 * sigma0 + 2.4e-7
    # rows before the clean snapshot were never rewritten; afterwards the runs differ by the rounding of exact against carried scales
    ce = inv.check_every
    assert torch.equal(l[:ce], l_ref[:ce])
    assert ((l - l_ref).abs() / l_ref).max().item() < 1e-3


# ------------------------------------------------------------------------------------------------------- model level
def _model_64(dev):
    """ood_faceGAN_e4e at 64² without the modulation blocks (they start at 256²): encoder latents in, generator, W+ loop."""
    from oodgan.arch import ood_faceGAN_e4e
    size = 64
    m = ood_faceGAN_e4e(out_size=size, style_dim=512, encoder='E4E', enable_modulation=False, build_encoder=False)
    sd = dict(synth.generator_state(size, seed=5, prefix='generator.'))
    sd['avg_latent'] = synth.normal('avg_latent', (1, 512), 41, 0.5)
    sd['delta_latent'] = synth.normal('delta_latent', (1, 10, 512), 41, 0.05)
    res = m.load_state_dict(sd, strict=False)
    assert not res.missing_keys and not res.unexpected_keys, res
    return m.to(dev).eval()


def test_model_invert_and_latent_std(dev):
    size, B, steps = 64, 2, 6
    m = _model_64(dev)
    x = synth.make_images(size, B, seed=44).to(dev)
    kw = dict(enc_lats=synth.make_latents(size, B, seed=42, std=0.3).to(dev), noise=[n.to(dev) for n in synth.make_noises(size, B, seed=45)])
    # the projector's scalar against the oracle's mapping network in float64 on the same z
    z = torch.randn(256, 512, generator=torch.Generator().manual_seed(0))
    P = {k: v.double() for k, v in synth.generator_state(size, seed=5).items()}
    wz = R.mapping_network(P, z.double())
    std_ref = ((wz - wz.mean(0, keepdim=True)) ** 2).sum().div(256).sqrt().item()
    std = m.generator.latent_std(n=256, seed=0)
    print(f'latent_std(n=256, seed=0) = {std:.6f}, float64 oracle {std_ref:.6f}')
    assert abs(std - std_ref) <= 1e-4 * std_ref and m.generator.latent_std(n=256, seed=0) == std
    assert m.generator.latent_std(n=256, seed=1) != std
    out0, lats0, l0 = m.invert(x, steps=steps, **kw)
    assert m.last_loss_terms['latent'] is None
    out, lats, losses = m.invert(x, steps=steps, latent_noise=0.05, lr_rampup=0.05, lr_rampdown=0.25, latent_reg=0.1, latent_anchor='mean', **kw)
    t = m.last_loss_terms
    assert torch.isfinite(out).all() and torch.isfinite(lats).all() and torch.isfinite(losses).all()
    assert t['latent'].shape == (steps, B) and torch.equal(losses, t['mse'] + 0.1 * t['latent']) and not torch.equal(lats, lats0)
    # 'mean': the prior of the first step is mean (w0 - (avg + delta))^2 = mean enc_lats^2
    want = (kw['enc_lats'].double() ** 2).mean(dim=(1, 2)).cpu()
    assert ((t['latent'][0].double().cpu() - want).abs() / want).max().item() < 1e-5
    # 'start' and a tensor holding the start latents are the same run
    w0 = m.encode(x, **kw)[0]
    a = m.invert(x, steps=steps, latent_reg=0.1, **kw)
    b = m.invert(x, steps=steps, latent_reg=0.1, latent_anchor=w0.clone(), **kw)
    assert torch.equal(a[1], b[1]) and torch.equal(a[2], b[2]) and (m.last_loss_terms['latent'][0] == 0).all()
    for name in ('lr_rampup', 'lr_rampdown', 'latent_noise', 'noise_ramp', 'latent_reg', 'noise_seed'):
        for bad in (-1, float('nan')):
            with pytest.raises(ValueError, match=name):
                m.invert(x, steps=2, **{name: bad}, **kw)
    with pytest.raises(ValueError, match='latent_anchor'):
        m.invert(x, steps=2, latent_reg=0.1, latent_anchor='median', **kw)
    for opt in (dict(latent_noise=0.05), dict(lr_rampup=0.05), dict(lr_rampdown=0.25), dict(latent_reg=0.1)):
        with pytest.raises(NotImplementedError):
            m.invert(x, steps=2, use_graph=True, **opt, **kw)


def test_one_step_at_1024(dev):
    """One 1024² step at B=1 with every option on: the loss row is MSE + latent_reg * prior, the prior is the float64 value, and with a
    ramp-up the first step leaves w where it was."""
    from oodgan.engine import GeneratorEngine, WPlusInverter
    size, B, reg = 1024, 1, 0.5
    eng = GeneratorEngine({k: v.to(dev) for k, v in synth.generator_state(size, seed=0).items()}, size)
    target = synth.make_images(size, B, seed=81).to(dev)
    noises = [n.to(dev) for n in synth.make_noises(size, B, seed=82)]
    w0 = synth.make_latents(size, B, seed=83, std=0.3).to(dev)
    anchor = synth.make_latents(size, 1, seed=84, std=0.3)[0].to(dev)
    inv = WPlusInverter(eng, lr_rampup=0.05, lr_rampdown=0.25, latent_noise=0.05, noise_ramp=0.75, noise_seed=7, latent_reg=reg)
    w, losses = inv.invert(target, w0, noises, steps=1, latent_anchor=anchor)
    torch.cuda.synchronize()
    t = inv.last_terms
    assert inv.last_stats == {'steps_run': [1], 'rollbacks': [0]} and torch.isfinite(w).all() and torch.isfinite(losses).all()
    assert losses.shape == (1, B) and torch.equal(losses, t['mse'] + reg * t['latent'])
    want = ((w0.double() - anchor.double()) ** 2).mean(dim=(1, 2)).cpu()
    assert ((t['latent'][0].double().cpu() - want).abs() / want).max().item() <= 1e-6
    assert torch.equal(w, w0)
    # the noise reached the generator: another seed, another MSE
    inv2 = WPlusInverter(eng, lr_rampup=0.05, lr_rampdown=0.25, latent_noise=0.05, noise_ramp=0.75, noise_seed=8, latent_reg=reg)
    inv2.invert(target, w0, noises, steps=1, latent_anchor=anchor)
    assert not torch.equal(inv2.last_terms['mse'], t['mse']) and torch.equal(inv2.last_terms['latent'], t['latent'])
