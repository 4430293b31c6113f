"""The feature offset of the W+ loop without a GPU: the float64 helper of the GPU tests (tests/fspace_ref.py) against the
reference's own autograd + torch.optim.Adam with a forward pre-hook on the up-conv (tests/golden/wplus_fspace.npz), the golden's own
float32 / float64 distance — the yardstick of the GPU tests —, the helper's Adam on two leaves against torch.optim.Adam, and the option
checks."""
import pytest
import torch

from oodgan import synth
import fspace_ref as FR

CASES = {'s64_l3': 12, 's64_l7': 12, 's256_l5': 5}        # steps compared: all twelve at 64², the first five (w after 1 and 5) at 256²
SUB = (slice(None), slice(None, None, 16), slice(None, None, 2), slice(None, None, 2))


def _inputs(g, name):
    size, l, steps = [int(v) for v in g[f'{name}_meta']]
    sw, sx, sn, s0 = [int(v) for v in g['seeds']]
    return (size, l, steps, synth.generator_state(size, seed=sw), synth.make_images(size, 2, seed=sx), synth.make_latents(size, 2, seed=s0, std=0.3),
            synth.make_noises(size, 2, seed=sn))


@pytest.mark.parametrize('name', list(CASES))
def test_helper_float64_loop_is_the_reference_loop(golden, name):
    """Both are float64 autograd of the same graph and the same Adam: losses within 1e-9 relative; w (stored as float32) within 1e-6; at the
    cases run to their end the offset's subsample within 1e-6 and its norm within 1e-9 relative."""
    g = golden('wplus_fspace.npz')
    size, l, steps, P, x, w0, noises = _inputs(g, name)
    n = CASES[name]
    keep = [int(t) for t in g[f'{name}_keep'] if int(t) <= n]
    P64 = {k: v.double() for k, v in P.items()}
    losses, _, w, d, kept = FR.invert(P64, size, w0.double(), l, x.double(), [z.double() for z in noises], n, keep=keep)
    ref = g[f'{name}_losses_f64'][:n]
    e_l = ((losses - ref).abs() / ref).max().item()
    e_w = max((kept[t][0].float() - g[f'{name}_w_step{t}_f64']).abs().max().item() for t in keep)
    print(f'{name}: {n} steps, float64 helper vs the reference float64 loop: loss rel {e_l:.2e} (bar 1e-9), w after steps {keep} {e_w:.2e} (bar 1e-6)')
    assert e_l <= 1e-9 and e_w <= 1e-6
    assert tuple(d.shape[1:]) == FR.feature_shape(P, l)
    if n == steps:
        e_d = (d.float()[SUB] - g[f'{name}_delta_sub_f64']).abs().max().item()
        e_n = ((d.flatten(1).norm(dim=1) - g[f'{name}_delta_norm_f64'][-1]).abs() / g[f'{name}_delta_norm_f64'][-1]).max().item()
        print(f'{name}: offset subsample {e_d:.2e} (bar 1e-6), ||delta|| rel {e_n:.2e} (bar 1e-9)')
        assert e_d <= 1e-6 and e_n <= 1e-9


@pytest.mark.parametrize('name', list(CASES))
def test_golden_float32_float64_distance(golden, name):
    """How far the reference's own two precisions drift apart: the yardstick the GPU loop test prints beside its figures.  Pinned: the loss curve
    an order of magnitude inside the 1e-3 bar of the loop tests, and >= 99 % of w and of the offset's subsample within 2 * lr * steps / 10 — the
    form the GPU test asserts, which the reference alone must meet."""
    g = golden('wplus_fspace.npz')
    steps = int(g[f'{name}_meta'][2])
    l32, l64 = g[f'{name}_losses_f32'], g[f'{name}_losses_f64']
    e = ((l32 - l64).abs() / l64).max().item()
    tol = 2 * 0.01 * steps / 10
    fw = ((g[f'{name}_w_step{steps}_f32'] - g[f'{name}_w_step{steps}_f64']).abs() < tol).float().mean().item()
    fd = ((g[f'{name}_delta_sub_f32'] - g[f'{name}_delta_sub_f64']).abs() < tol).float().mean().item()
    print(f'{name}: reference fp32 vs float64: loss curve rel {e:.2e}; w within {tol:.3f}: {100 * fw:.3f} %, offset subsample: {100 * fd:.3f} %; '
          f'loss {l64[0].tolist()} -> {l64[-1].tolist()}')
    assert e < 1e-4 and fw >= 0.99 and fd >= 0.99
    assert (l64[-1] < l64[0]).all()


def test_helper_adam_on_two_leaves_is_torch_adam():
    """16², l = 3, float64, 4 steps with feature_reg and two learning rates: the helper's written-out loop against torch.optim.Adam with two
    parameter groups on autograd through the same wrapped oracle."""
    from oracle import ref_cpu as R
    size, l, steps, lam, lr, flr = 16, 3, 4, 0.5, 0.01, 0.03
    P = {k: v.double() for k, v in synth.generator_state(size, seed=5).items()}
    x, w0 = synth.make_images(size, 1, seed=9).double(), synth.make_latents(size, 1, seed=14).double()
    noises = [z.double() for z in synth.make_noises(size, 1, seed=7)]
    losses, regs, w, d, _ = FR.invert(P, size, w0, l, x, noises, steps, lr=lr, feature_lr=flr, feature_reg=lam)
    wt = w0.clone().requires_grad_(True)
    dt = torch.zeros((1,) + FR.feature_shape(P, l), dtype=torch.float64, requires_grad=True)
    opt = torch.optim.Adam([dict(params=[wt], lr=lr), dict(params=[dt], lr=flr)], betas=(0.9, 0.999), eps=1e-8)
    for i in range(steps):
        opt.zero_grad()
        tot = R.wplus_loss(FR.forward(P, size, wt, l, dt, noises), x) + lam * (dt ** 2).mean()
        tot.backward()
        assert abs(float(tot.detach()) - float(losses[i, 0])) <= 1e-12 * abs(float(tot.detach()))
        opt.step()
    assert (wt.detach() - w).abs().max().item() <= 1e-12 and (dt.detach() - d).abs().max().item() <= 1e-12
    assert regs[0, 0] == 0 and regs[-1, 0] > 0 and d.abs().max() > 0


def test_offset_reaches_only_its_layer():
    """The wrapped oracle adds the offset to ONE call: a zero offset is the plain forward bit for bit, a non-zero one moves the picture, and the
    wrapper is gone afterwards."""
    from oracle import ref_cpu as R
    size = 16
    P = synth.generator_state(size, seed=5)
    w, noises = synth.make_latents(size, 2, seed=14), synth.make_noises(size, 2, seed=7)
    plain = R.styled_conv
    base = R.generator_forward(P, w, noises, size)
    shape = (2,) + FR.feature_shape(P, 3)
    assert shape == (2, 512, 8, 8)
    assert torch.equal(FR.forward(P, size, w, 3, torch.zeros(shape), noises), base)
    assert (FR.forward(P, size, w, 3, synth.normal('fs.d', shape, 3, 0.3), noises) - base).abs().max() > 1e-3
    assert R.styled_conv is plain


def test_option_checks():
    from oodgan.engine import FEATURE_LAYERS, WPlusInverter, check_feature_layer, check_feature_offset
    from oodgan import cli
    assert FEATURE_LAYERS == FR.FEATURE_LAYERS == (3, 5, 7)
    assert check_feature_layer(None) is None and [check_feature_layer(l, 18) for l in (3, 5, 7)] == [3, 5, 7]
    for bad in (0, 1, 2, 4, 6, 9, 11, -3, 5.0, '5', True, [5]):
        with pytest.raises(ValueError, match='feature_layer'):
            check_feature_layer(bad)
    assert check_feature_layer(5, 8) == 5 and check_feature_layer(7, 10) == 7       # 32²: up-convs read latents 1, 3, 5; 64²: 1 ... 7
    for l, n in ((5, 6), (7, 8), (7, 6), (3, 4)):           # latent n - 1 feeds only the last ToRGB: 16² has no up-conv on latent 5, 32² none on 7
        with pytest.raises(ValueError, match='feature_layer'):
            check_feature_layer(l, n)
    assert check_feature_offset(None, None, 0.0, 0.01) == (None, None, 0.0)
    assert check_feature_offset(5, None, 0.0, 0.02) == (5, 0.02, 0.0)         # the default rate is the latents'
    assert check_feature_offset(5, 0.0, 0.25, 0.02, 'w') == (5, 0.0, 0.25)    # a rate of 0 is allowed: the offset stays at zero
    for kw, name in ((dict(feature_layer=None, feature_lr=0.01), 'feature_lr'), (dict(feature_layer=None, feature_reg=0.5), 'feature_reg'),
                     (dict(feature_layer=5, feature_lr=-1.0), 'feature_lr'), (dict(feature_layer=5, feature_reg=float('nan')), 'feature_reg'),
                     (dict(feature_layer=5, feature_reg='x'), 'feature_reg'), (dict(feature_layer=4), 'feature_layer'),
                     (dict(feature_layer=5, latent_space='s'), 'feature_layer')):
        args = dict(feature_layer=None, feature_lr=None, feature_reg=0.0, latent_space='w+')
        args.update(kw)
        with pytest.raises(ValueError, match=name):
            check_feature_offset(args['feature_layer'], args['feature_lr'], args['feature_reg'], 0.01, args['latent_space'])
        with pytest.raises(ValueError, match=name):
            WPlusInverter(None, **kw)
    inv = WPlusInverter(None, lr=0.02, feature_layer=7, feature_reg=0.5)
    assert (inv.feature_layer, inv.feature_lr, inv.feature_reg, inv.last_feature_offset) == (7, 0.02, 0.5, None)
    inv = WPlusInverter(None)
    assert (inv.feature_layer, inv.feature_lr, inv.feature_reg) == (None, None, 0.0)
    with pytest.raises(NotImplementedError, match='feature_layer'):
        WPlusInverter(None, feature_layer=5)._refuse_graph(None)
    # the command-line keys
    assert cli.feature_options({}) == dict(feature_layer=None, feature_lr=None, feature_reg=0.0)
    assert cli.feature_options(dict(feature_layer=5, feature_lr=0.05, feature_reg=0.1), 18) == dict(feature_layer=5, feature_lr=0.05, feature_reg=0.1)
    assert cli.feature_options(dict(feature_layer=3))['feature_lr'] is None      # left to invert(): its ``lr``
    for bad, name in ((dict(feature_layer=9), 'inversion.feature_layer'), (dict(feature_reg=0.1), 'inversion.feature_reg'),
                      (dict(feature_layer=5, feature_lr=-1), 'inversion.feature_lr'), (dict(feature_layer=5, latent_space='s'), 'inversion.feature_layer')):
        with pytest.raises(ValueError, match=name):
            cli.feature_options(bad)
    with pytest.raises(ValueError, match='inversion.feature_layer'):
        cli.feature_options(dict(feature_layer=7), 6)
