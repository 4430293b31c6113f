"""The colour map of the W+ loop without a GPU: the yardstick of tests/color_ref.py against torch autograd of the einsum
formula in float64 — value, the image gradient and dL/dtheta; the free masks; ``ops.color_inverse``; the option checks and refusals of
``oodgan.engine``; the CLI keys; the C ABI keeps its number and carries the new entries."""
import inspect
import os
import re

import pytest
import torch

import color_ref as CR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(16, 16), (37, 53)]


def _case(B, H, W, seed):
    gen = torch.Generator().manual_seed(seed)
    img = torch.randn(B, 3, H, W, generator=gen, dtype=torch.float64)
    x = torch.randn(B, 3, H, W, generator=gen, dtype=torch.float64)
    beta = torch.rand(B, 1, H, W, generator=gen, dtype=torch.float64)
    th = (CR.identity(B, torch.float64) + 0.2 * torch.randn(B, 12, generator=gen, dtype=torch.float64)).float()
    return img, x, beta, th


@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: f'{s[0]}x{s[1]}')
def test_yardstick_is_autograd_of_the_formula(shape):
    """``color_ref.term`` against torch autograd of the einsum formula, float64: loss, gimg and dL/dtheta for B in {1, 3} x four kinds x with
    and without a loss weight: <= 1e-12 of the largest entry."""
    H, W = shape
    for B in (1, 3):
        img, x, beta, th = _case(B, H, W, 100 * H + W + B)
        for kind in CR.KINDS:
            for w in (None, beta):
                loss, gimg, dth, _ = CR.term(img, x, th, kind, 0.5, w)
                l_a, g_a, t_a = CR.autograd_term(img, x, th, kind, 0.5, w)
                e = [(p - q).abs().max().item() / max(q.abs().max().item(), 1e-300) for p, q in ((loss, l_a), (gimg, g_a), (dth, t_a))]
                print(f'{H}x{W} B={B} {kind} beta={w is not None}: loss {e[0]:.1e}, gimg {e[1]:.1e}, dL/dtheta {e[2]:.1e} (bar 1e-12)')
                assert max(e) <= 1e-12
    # grad_mul and grad_div scale the two gradients as the step uses them
    loss, gimg, dth, _ = CR.term(img, x, th, 'huber', 0.5, beta, grad_mul=8.0, grad_div=8.0)
    _, g_a, t_a = CR.autograd_term(img, x, th, 'huber', 0.5, beta)
    assert (gimg - 8.0 * g_a).abs().max() <= 1e-12 * g_a.abs().max() * 8 and (dth - t_a).abs().max() <= 1e-12 * t_a.abs().max()


def test_yardstick_honours_the_free_masks():
    img, x, beta, th = _case(2, 16, 16, 5)
    full = CR.term(img, x, th, 'mse', reg=0.3)[2]
    gain = CR.term(img, x, th, 'mse', free='gain', reg=0.3)[2]
    fixed = [1, 2, 3, 5, 6, 7]
    free = [0, 4, 8, 9, 10, 11]
    assert (gain[:, fixed] == 0).all() and torch.equal(gain[:, free], full[:, free]) and (full[:, fixed] != 0).all()
    assert CR.FREE == {'affine': 0xfff, 'gain': 0xf11} and CR.free_mask('gain').tolist() == [1, 0, 0, 0, 1, 0, 0, 0, 1, 1, 1, 1]
    # the regulariser: its gradient and its sum
    plain = CR.term(img, x, th, 'mse')[2]
    off = th.double() - CR.identity(2, torch.float64)
    assert (full - plain - 0.6 * off).abs().max() <= 1e-15
    assert (CR.term(img, x, th, 'mse')[3] - (off * off).sum(1)).abs().max() <= 1e-15
    # Adam leaves a number that is not free where it is
    t2, m2, v2 = CR.adam(th.double(), full, torch.zeros(2, 12, dtype=torch.float64), torch.zeros(2, 12, dtype=torch.float64), 1, 0.01, free='gain')
    assert torch.equal(t2[:, fixed], th.double()[:, fixed]) and (m2[:, fixed] == 0).all() and (t2[:, free] != th.double()[:, free]).all()
    from oodgan import ops
    assert ops.COLOR_KINDS == CR.FREE


def test_color_inverse_round_trips():
    from oodgan import ops
    th = torch.tensor(CR.THETA_STAR + (CR.IDENTITY,), dtype=torch.float64)
    ti = ops.color_inverse(th)
    assert ti.dtype == th.dtype and (ti - CR.inverse(th)).abs().max() <= 1e-12
    assert (ops.color_inverse(ti) - th).abs().max() <= 1e-12 and torch.equal(ti[2], th[2])
    img = torch.randn(3, 3, 8, 9, generator=torch.Generator().manual_seed(1), dtype=torch.float64)
    e = (CR.apply(CR.apply(img, th), ti) - img).abs().max().item()
    print(f'color_inverse round trip: {e:.2e} (bar 1e-12)')
    assert e <= 1e-12
    assert ops.color_inverse(th.float()).dtype == torch.float32
    singular = th.clone()
    singular[1, 3:6] = singular[1, 0:3] * 2.0
    for bad in (singular, torch.zeros(1, 12, dtype=torch.float64), torch.full((1, 12), float('nan'), dtype=torch.float64),
                torch.tensor([[float('inf')] + list(CR.IDENTITY[1:])], dtype=torch.float64)):
        with pytest.raises(ValueError, match='color_inverse'):
            ops.color_inverse(bad)
    with pytest.raises(ValueError, match='12'):
        ops.color_inverse(torch.zeros(4))


def test_checks_and_refusals():
    from oodgan import engine as E
    assert E.check_color() == (None, 0.002, 0.0) and E.check_color('gain') == ('gain', 0.002, 0.0)
    assert E.check_color('affine', 0, 0.5) == ('affine', 0.0, 0.5) and E.check_color(None, -1, 'x') == (None, 0.002, 0.0)
    with pytest.raises(ValueError, match=re.escape("color must be None or one of ['gain', 'affine'], got 'tone'")):
        E.check_color('tone')
    with pytest.raises(ValueError, match=re.escape("color must be None or one of ['gain', 'affine'], got True")):
        E.check_color(True)
    for bad in (dict(color_lr=-0.1), dict(color_lr=float('nan')), dict(color_lr='0.1'), dict(color_lr=True)):
        with pytest.raises(ValueError, match='color_lr'):
            E.check_color('gain', **bad)
    for bad in (dict(color_reg=-1.0), dict(color_reg=float('inf')), dict(color_reg=None)):
        with pytest.raises(ValueError, match='color_reg'):
            E.check_color('affine', **bad)
    with pytest.raises(ValueError, match=re.escape('inversion.color_lr / inversion.color_reg must be finite numbers >= 0, got -1, 0.0')):
        E.check_color('gain', -1, 0.0, 'inversion.')
    E.refuse_color()
    E.refuse_color(loss_region='blend')
    E.refuse_color(loss_region='a loss-weight tensor')
    tail = "the colour map is built for the full-resolution pixel term"
    for kw, what in ((dict(use_graph=True), 'color with use_graph'), (dict(lpips=True), 'color with the LPIPS term'),
                     (dict(ssim=True), 'color with the SSIM term'), (dict(loss_region='fit'), "color with loss_region 'fit'"),
                     (dict(align='similarity'), "color with align 'similarity'"), (dict(pixel_size=32), 'color with pixel_size'),
                     (dict(pixel_filter='bicubic'), "color with pixel_filter 'bicubic'"), (dict(pixel_target=torch.zeros(1)), 'color with pixel_target'),
                     (dict(latent_space='s'), "color with latent_space 's'"), (dict(feature_layer=5), 'color with feature_layer'),
                     (dict(padded=True), 'color with a generator whose channel counts are zero-padded')):
        with pytest.raises(NotImplementedError, match=re.escape(what)) as ei:
            E.refuse_color(**kw)
        assert tail in str(ei.value)
    assert E.check_color_init(None) is None
    t = CR.identity(2)
    assert E.check_color_init(t) is t and E.check_color_init(t, 2, 'cpu') is t
    for bad in (torch.zeros(2, 4), torch.zeros(12), torch.zeros(2, 12, dtype=torch.float64), [[0.0] * 12]):
        with pytest.raises(ValueError, match=re.escape('color_init must be None or a float32 (B, 12) tensor')):
            E.check_color_init(bad)
    with pytest.raises(ValueError, match=re.escape('color_init must be a float32 (3, 12) tensor on cpu')):
        E.check_color_init(t, 3, 'cpu')
    with pytest.raises(ValueError, match='color_init must hold finite values'):
        E.check_color_init(torch.full((2, 12), float('inf')))
    # the constructor checks before anything else happens; the neighbours keep their signatures
    with pytest.raises(ValueError, match='color'):
        E.WPlusInverter(None, color='gamma')
    inv = E.WPlusInverter(None, color='gain', color_lr=0.004, color_reg=0.1)
    assert (inv.color, inv.color_lr, inv.color_reg, inv.last_color) == ('gain', 0.004, 0.1, None)
    assert E.WPlusInverter(None).color is None
    assert list(inspect.signature(E.refuse_align).parameters) == ['use_graph', 'lpips', 'ssim', 'loss_region', 'pixel_filter', 'pixel_target',
                                                                   'latent_space', 'feature_layer', 'padded']


def test_model_invert_names_the_options():
    """``invert`` has **kwargs: the new names must be real parameters, or an unknown ``color`` would be swallowed in silence."""
    from oodgan.arch import ood_faceGAN_e4e
    p = inspect.signature(ood_faceGAN_e4e.invert).parameters
    assert p['color'].default is None and p['color_lr'].default == 0.002 and p['color_reg'].default == 0.0 and p['color_init'].default is None
    from oodgan.engine import WPlusInverter
    assert inspect.signature(WPlusInverter.invert).parameters['color_init'].default is None


def test_cli_keys_are_checked_before_the_gpu():
    from oodgan import cli
    assert cli.color_options({}) == {} and cli.color_options({'loss_region': 'blend'}) == {}
    assert cli.color_options({'color': 'gain'}) == dict(color='gain', color_lr=0.002, color_reg=0.0)
    assert cli.color_options({'color': 'affine', 'color_lr': 0.004, 'color_reg': 0.5, 'loss_region': 'blend', 'pixel_loss': 'huber',
                              'latent_space': 'w', 'mask_dir': '/masks'}) == dict(color='affine', color_lr=0.004, color_reg=0.5)
    on = {'color': 'affine'}
    for block, name in (({'color': 'tone'}, 'inversion.color'), ({'color': True}, 'inversion.color'), ({**on, 'color_lr': -1}, 'inversion.color_lr'),
                        ({**on, 'color_lr': float('nan')}, 'inversion.color_lr'), ({**on, 'color_lr': '0.1'}, 'inversion.color_lr'),
                        ({**on, 'color_reg': -0.5}, 'inversion.color_reg'), ({**on, 'color_reg': float('inf')}, 'inversion.color_reg'),
                        ({'color_lr': 0.01}, 'inversion.color_lr'), ({'color_reg': 0.1}, 'inversion.color_reg')):
        with pytest.raises(ValueError, match=name):
            cli.run({'name': 'x', 'datasets': {}, 'inversion': block})
    for block, name in (({**on, 'ssim_weight': 0.5}, 'SSIM'), ({**on, 'lpips_weight': 0.8}, 'LPIPS'), ({**on, 'loss_region': 'fit'}, 'loss_region'),
                        ({**on, 'align': 'similarity'}, 'align'), ({**on, 'pixel_size': 32}, 'pixel_size'),
                        ({**on, 'pixel_target': 'file'}, 'pixel_target'), ({**on, 'latent_space': 's'}, 'latent_space'),
                        ({**on, 'feature_layer': 5}, 'feature_layer')):
        with pytest.raises(NotImplementedError, match=name):
            cli.run({'name': 'x', 'datasets': {}, 'inversion': block})


def test_abi_keeps_its_number_and_carries_the_entries():
    from ctypes import c_int
    from oodgan import _lib
    assert _lib.ABI_VERSION == 117
    sigs = _lib._SIGS
    assert len(sigs['oodgan_color_pixel_loss_fwd_bwd'][1]) == 15 and len(sigs['oodgan_color_pixel_loss_fwd_bwd_row'][1]) == 17
    assert len(sigs['oodgan_color_step'][1]) == 21 and len(sigs['oodgan_color_apply'][1]) == 7
    assert sigs['oodgan_color_nparts'] == (c_int, [c_int, c_int])
    hdr = open(os.path.join(ROOT, 'include', 'oodgan.h')).read()
    assert '"color"' in hdr
    for name, n in (('oodgan_color_pixel_loss_fwd_bwd', 15), ('oodgan_color_pixel_loss_fwd_bwd_row', 17), ('oodgan_color_step', 21),
                    ('oodgan_color_apply', 7), ('oodgan_color_nparts', 2)):
        decl = re.search(r'int %s\((.*?)\);' % name, hdr, re.S).group(1)
        assert len(decl.split(',')) == n, name
    h = _lib.lib()          # loads without a GPU; bad arguments come back as a status
    assert h.oodgan_version() == 117
    assert h.oodgan_color_apply(None, None, None, 1, 8, 8, None) == -1 and b'color_apply' in h.oodgan_last_error()
    assert h.oodgan_color_nparts(64, 64) == 2 and h.oodgan_color_nparts(16, 16) == 1 and h.oodgan_color_nparts(0, 64) == 0
    assert h.oodgan_dispatch_count(b'color') >= 0
