"""Latent controls and edits of the W+ loop, the parts that need no GPU: the option checks of the engine and of the CLI's
``inversion`` block, and the closed form of the spread term's gradient, which tests/test_hip_latent_controls.py uses as its reference."""
import math

import pytest
import torch

from oodgan import cli
from oodgan.engine import WPlusInverter, check_latent_controls, check_layer_lr, check_latent_space


def test_engine_option_checks():
    inv = WPlusInverter(None)
    assert (inv.latent_space, inv.layer_lr, inv.delta_reg) == ('w+', None, 0.0)
    inv = WPlusInverter(None, latent_space='w+', layer_lr=[1, 0.5, 0], delta_reg=2)
    assert inv.layer_lr == (1.0, 0.5, 0.0) and inv.delta_reg == 2.0
    assert WPlusInverter(None, latent_space='w').latent_space == 'w'
    for bad in ('W', 'z', None, 1, ''):
        with pytest.raises(ValueError, match='latent_space'):
            WPlusInverter(None, latent_space=bad)
    for bad in ([1.0, -0.5], [1.0, float('nan')], [float('inf')], [True, 1.0], ['1'], [], 1.0, 'abc'):
        with pytest.raises(ValueError, match='layer_lr'):
            WPlusInverter(None, layer_lr=bad)
    for bad in (-1.0, float('nan'), float('inf'), 'x', None):
        with pytest.raises(ValueError, match='delta_reg'):
            WPlusInverter(None, delta_reg=bad)
    # one vector per image: no per-layer rates, and the spread is identically zero
    with pytest.raises(ValueError, match='layer_lr'):
        WPlusInverter(None, latent_space='w', layer_lr=[1.0] * 18)
    with pytest.raises(ValueError, match='delta_reg'):
        WPlusInverter(None, latent_space='w', delta_reg=0.5)
    # the length, once the number of layers is known
    assert check_layer_lr([1.0] * 18, 18) == (1.0,) * 18 and check_layer_lr(None, 18) is None
    with pytest.raises(ValueError, match='layer_lr'):
        check_layer_lr([1.0] * 17, 18)
    with pytest.raises(ValueError, match='layer_lr'):
        check_latent_controls('w+', [1.0, 1.0], 0.0, n_layers=18)
    assert check_latent_space('w') == 'w'


def test_cli_latent_options():
    assert cli.latent_options({}) == dict(latent_space='w+', layer_lr=None, delta_reg=0.0)
    assert cli.latent_options({'latent_space': 'w'})['latent_space'] == 'w'
    got = cli.latent_options({'layer_lr': [1, 1, 0], 'delta_reg': 0.5}, n_layers=3)
    assert got == dict(latent_space='w+', layer_lr=[1.0, 1.0, 0.0], delta_reg=0.5)
    for block, name in (({'latent_space': 'wplus'}, 'inversion.latent_space'), ({'layer_lr': [1, -1]}, 'inversion.layer_lr'),
                        ({'layer_lr': [1, float('nan')]}, 'inversion.layer_lr'), ({'layer_lr': 0.5}, 'inversion.layer_lr'),
                        ({'delta_reg': -0.1}, 'inversion.delta_reg'), ({'delta_reg': float('inf')}, 'inversion.delta_reg'),
                        ({'latent_space': 'w', 'layer_lr': [1.0]}, 'inversion.layer_lr'), ({'latent_space': 'w', 'delta_reg': 1.0}, 'inversion.delta_reg')):
        with pytest.raises(ValueError, match=name):
            cli.latent_options(block)
    with pytest.raises(ValueError, match='inversion.layer_lr'):
        cli.latent_options({'layer_lr': [1.0] * 10}, n_layers=18)


def test_cli_edit_option_and_run_checks_before_the_gpu():
    assert cli.edit_option({}) == 'start' and cli.edit_option({'edit': 'start'}) == 'start' and cli.edit_option({'edit': 'final'}) == 'final'
    for bad in ('end', 'Final', True, None, 1):
        with pytest.raises(ValueError, match='inversion.edit'):
            cli.edit_option({'edit': bad})
    # ``run`` checks the block before it asks for a GPU or builds the model
    for block, name in (({'edit': 'last'}, 'inversion.edit'), ({'latent_space': 'q'}, 'inversion.latent_space'),
                        ({'layer_lr': [-1.0]}, 'inversion.layer_lr'), ({'delta_reg': -1}, 'inversion.delta_reg')):
        with pytest.raises(ValueError, match=name):
            cli.run({'name': 'x', 'datasets': {}, 'inversion': block})


@pytest.mark.parametrize('shape', [(2, 18, 512), (1, 4, 37), (2, 1, 512)])
def test_spread_gradient_closed_form(shape):
    """R_b = mean_le (w_le - mean_l w_le)^2: float64 autograd gives dR/dw_le = 2 (w_le - mean_l w_le) / (L D) — the cross terms through the
    mean cancel because sum_l (w_le - mean_l w_le) = 0."""
    B, L, D = shape
    w = torch.randn(shape, dtype=torch.float64, generator=torch.Generator().manual_seed(7)).requires_grad_(True)
    R = ((w - w.mean(dim=1, keepdim=True)) ** 2).mean(dim=(1, 2))
    R.sum().backward()
    closed = 2.0 * (w.detach() - w.detach().mean(dim=1, keepdim=True)) / (L * D)
    assert (w.grad - closed).abs().max().item() <= 1e-15 * max(1.0, closed.abs().max().item())
    if L == 1:
        assert R.abs().max().item() == 0.0 and closed.abs().max().item() == 0.0
    else:
        assert math.isfinite(R.sum().item()) and (R > 0).all()
