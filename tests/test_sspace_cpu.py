"""StyleSpace without a GPU: the float64 yardstick of tests/sspace_ref.py against torch itself, the option checks, and the
public layout of the style columns."""
import pytest
import torch

import sspace_ref as SR
from oracle import ref_cpu as R
from oodgan import synth

SIZE = 16


def _inputs(B=2, dt=torch.float64):
    P = {k: v.to(dt) for k, v in synth.generator_state(SIZE, seed=5).items()}
    return (P, synth.make_latents(SIZE, B, seed=14).to(dt), synth.make_images(SIZE, B, seed=9).to(dt),
            [n.to(dt) for n in synth.make_noises(SIZE, B, seed=7)])


def test_helper_adam_is_torch_adam():
    """Five steps of the helper's loop (gradient through the replaced biases, the regulariser, Adam written out) against torch.optim.Adam on
    an autograd leaf added to the same biases, float64: the offsets agree to rounding."""
    P, w0, x, noises = _inputs(B=1)
    lam, lr, steps = 0.5, 0.01, 5
    losses, regs, delta, _ = SR.invert(P, SIZE, w0, x, noises, steps, lr=lr, style_reg=lam)
    leaf = torch.zeros(SR.n_rows(P, SIZE), dtype=torch.float64, requires_grad=True)
    opt = torch.optim.Adam([leaf], lr=lr, betas=(0.9, 0.999), eps=1e-8)
    want = []
    for _ in range(steps):
        opt.zero_grad(set_to_none=True)
        tot = R.wplus_loss(SR.forward(P, SIZE, w0[0], leaf, noises), x) + lam * (leaf ** 2).mean()
        tot.backward()
        want.append(float(tot.detach()))
        opt.step()
    e_d = (delta[0] - leaf.detach()).abs().max().item()
    e_l = max(abs(a - b) / b for a, b in zip(losses[:, 0].tolist(), want))
    print(f'helper Adam vs torch.optim.Adam, 5 steps float64: |delta| diff {e_d:.2e} (max |delta| {leaf.detach().abs().max().item():.2e}), loss rel {e_l:.2e}')
    assert e_d <= 1e-12 and e_l <= 1e-12
    assert leaf.detach().abs().max().item() > 1e-3 and regs[0, 0] == 0.0 and regs[-1, 0] > 0.0


def test_zero_offset_is_the_plain_forward():
    """lambda = 0, delta = 0: the helper's loss is oracle.ref_cpu.wplus_loss of the plain forward, image by image, and its gradient is not zero."""
    P, w0, x, noises = _inputs(B=2)
    R_ = SR.n_rows(P, SIZE)
    for b in range(2):
        nz = [n[b:b + 1] for n in noises]
        tot, pix, reg, g = SR.loss_and_grad(P, SIZE, w0[b], torch.zeros(R_, dtype=torch.float64), x[b:b + 1], nz)
        want = float(R.wplus_loss(R.generator_forward(P, w0[b:b + 1], nz, SIZE), x[b:b + 1]))
        assert tot == pix == want and reg == 0.0
        assert g.shape == (R_,) and g.abs().max().item() > 0


def test_offset_gradient_matches_a_finite_difference():
    """dL/ddelta of the helper against a central difference of its own loss in float64, on one row of every layer's slice."""
    P, w0, x, noises = _inputs(B=1)
    R_ = SR.n_rows(P, SIZE)
    d0 = 0.05 * synth.normal('sspace.fd', (R_,), 3).double()
    _, _, _, g = SR.loss_and_grad(P, SIZE, w0[0], d0, x, noises, style_reg=0.3)
    h = 1e-6
    for name, lat, row, n in SR.layout(P, SIZE):
        r = row + n // 3
        e = torch.zeros(R_, dtype=torch.float64)
        e[r] = h
        fd = (SR.loss_and_grad(P, SIZE, w0[0], d0 + e, x, noises, 0.3)[0] - SR.loss_and_grad(P, SIZE, w0[0], d0 - e, x, noises, 0.3)[0]) / (2 * h)
        assert abs(fd - g[r].item()) <= 1e-6 * g.abs().max().item() + 1e-9, (name, fd, g[r].item())


def test_option_checks():
    from oodgan.engine import LATENT_SPACES, check_latent_controls, check_latent_space, check_style_space
    assert 's' in LATENT_SPACES and check_latent_space('s') == 's'
    assert check_style_space('s', 0.25) == 0.25 and check_style_space('w+', 0.0) == 0.0 and check_style_space('s', 0) == 0.0
    # per-layer rates are allowed in 's' (they apply through row_lat); the three controls of the latents are not
    assert check_latent_controls('s', [1.0] * 10, 0.0, 10) == ('s', (1.0,) * 10, 0.0)
    for name, kw in (('delta_reg', dict(delta_reg=0.5)), ('latent_noise', dict(latent_noise=0.05)), ('latent_reg', dict(latent_reg=0.5))):
        with pytest.raises(ValueError, match=name) as ei:
            check_style_space('s', 0.0, **kw)
        assert 'latent_space' in str(ei.value)                  # both options are named
    for space in ('w+', 'w'):
        with pytest.raises(ValueError, match='style_reg') as ei:
            check_style_space(space, 0.5)
        assert 'latent_space' in str(ei.value)
    for bad in (-1.0, float('nan'), float('inf'), 'x', None):
        with pytest.raises(ValueError, match='style_reg'):
            check_style_space('s', bad)
    with pytest.raises(ValueError, match='inversion.style_reg'):
        check_style_space('w', 1.0, prefix='inversion.')


def test_cli_options():
    from oodgan import cli
    inv = {'latent_space': 's', 'style_reg': 0.1, 'layer_lr': [1.0] * 18}
    assert cli.latent_options(inv, 18)['latent_space'] == 's' and cli.style_options(inv) == {'style_reg': 0.1}
    assert cli.style_options({}) == {'style_reg': 0.0}
    for inv, name in (({'latent_space': 's', 'delta_reg': 0.5}, 'inversion.delta_reg'), ({'latent_space': 's', 'latent_noise': 0.05}, 'inversion.latent_noise'),
                      ({'latent_space': 's', 'latent_reg': 1.0}, 'inversion.latent_reg'), ({'style_reg': 0.5}, 'inversion.style_reg'),
                      ({'latent_space': 'w', 'style_reg': 0.5}, 'inversion.style_reg')):
        with pytest.raises(ValueError, match=name):
            cli.style_options(inv)
    # a data set's direction file is a W+ direction: `edit: final` cannot hand it to a StyleSpace fit
    with pytest.raises(ValueError, match='latent_space: s'):
        cli.check_edit_space('final', 's', True, 'smile')
    cli.check_edit_space('final', 's', False)
    cli.check_edit_space('start', 's', True)
    cli.check_edit_space('final', 'w+', True)


def test_inverter_refuses_before_it_touches_the_engine():
    """The constructor checks the options (no engine needed for that)."""
    from oodgan.engine import WPlusInverter
    inv = WPlusInverter(None, latent_space='s', style_reg=0.1, layer_lr=[1.0, 0.0])
    assert inv.latent_space == 's' and inv.style_reg == 0.1
    for kw in (dict(latent_space='s', delta_reg=0.5), dict(latent_space='s', latent_noise=0.1), dict(latent_space='s', latent_reg=0.1),
               dict(style_reg=0.1), dict(latent_space='w', style_reg=0.1)):
        with pytest.raises(ValueError):
            WPlusInverter(None, **kw)
    with pytest.raises(NotImplementedError, match="latent_space 's'"):
        inv._refuse_graph(None)


def test_style_layout_at_64():
    """The layout covers [0, R) without gaps, grouped by ascending latent index, with names that are modules of the state dict; it is the
    yardstick's own layout."""
    from oodgan.modules import Generator, StyleGAN2Generator
    g = Generator(64, 512, 2)
    lay = g.style_layout()
    sd = g.state_dict()
    assert lay == SR.layout(sd, 64)
    assert len(lay) == 2 * 5 + 4            # 9 styled convs + 5 ToRGBs at 64²
    row, last = 0, 0
    for name, lat, r0, n in lay:
        assert r0 == row and n == sd[f'{name}.conv.modulation.bias'].numel() == sd[f'{name}.conv.modulation.weight'].shape[0]
        assert lat >= last and 0 <= lat < g.n_latent
        row, last = row + n, lat
    assert [x[0] for x in lay][:5] == ['conv1', 'to_rgb1', 'convs.0', 'convs.1', 'to_rgbs.0'] and lay[-1][0] == 'to_rgbs.3'
    assert sorted({x[1] for x in lay}) == list(range(g.n_latent))
    assert StyleGAN2Generator(64, 512, 2).style_layout() == lay
    with pytest.raises(NotImplementedError, match='zero-padded'):          # 256² / 0.1875: 48 and 24 channels
        StyleGAN2Generator(256, 512, 2, narrow=0.1875).style_layout()


def test_cli_refuses_a_wplus_direction_for_a_style_fit_before_anything_runs(tmp_path):
    """``run()`` with ``edit: final``, ``latent_space: s``, W+ steps and a data set that names an editing direction: ValueError before the model
    is built or a file is read (no GPU, no network_g, no data root needed to get there); without steps, or with ``edit: start``, the check lets
    the options through (the run then stops where it needs the GPU)."""
    from oodgan import cli
    import numpy as np
    np.save(tmp_path / 'smile.npy', np.ones((18, 512), dtype=np.float32))
    ed = {'direction': 'smile', 'intensity': 1.5}
    opts = dict(name='t', directions_dir=str(tmp_path), datasets={'plain': {'dataroot': 'none'}, 'smile': {'dataroot': 'none', 'editing': ed}},
                inversion={'latent_space': 's', 'edit': 'final', 'wplus_steps': 4})
    assert cli.load_direction(str(tmp_path), ed).dim() > 0 and cli.load_direction(str(tmp_path), None).dim() == 0
    with pytest.raises(ValueError, match="latent_space: s.*'smile'"):
        cli.run(opts)
    if not torch.cuda.is_available():
        for inv in ({'latent_space': 's', 'edit': 'final', 'wplus_steps': 0}, {'latent_space': 's', 'edit': 'start', 'wplus_steps': 4},
                    {'latent_space': 'w+', 'edit': 'final', 'wplus_steps': 4}):
            with pytest.raises(RuntimeError, match='ROCm GPU'):
                cli.run(dict(opts, inversion=inv))
