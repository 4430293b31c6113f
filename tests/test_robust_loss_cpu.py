"""CPU checks of the robust pixel terms' host side: the float64 yardstick of the GPU tests (tests/robust_ref.py) against
torch's own Huber loss, the Charbonnier closed form, autograd and the limits of each rho; the option checker and the CLI's
``inversion.pixel_loss`` / ``inversion.pixel_scale``."""
import pytest
import torch
import torch.nn.functional as F

from robust_ref import KINDS, psi, rho, scale32

SCALES = (1e-6, 0.1, 0.5, 10.0)
BAD_SCALES = [0, -0.5, float('nan'), float('inf'), 'wide']


def _residuals():
    """Seeded float64 residuals of order 1, with exact zeros and both signs of large outliers."""
    from oodgan import synth
    d = synth.normal('robust.cpu', (2, 3, 16, 16), 31).double()
    d[0, 0, 0, :6] = torch.tensor([0.0, -0.0, 25.0, -25.0, 0.5, -0.5], dtype=torch.float64)
    return d


def test_huber_and_charbonnier_equal_their_anchors():
    d = _residuals()
    for s in SCALES:
        want = F.huber_loss(d, torch.zeros_like(d), reduction='none', delta=s)
        assert (rho(d, 'huber', s) - want).abs().max().item() <= 1e-15 * max(1.0, s * 25.0)
        assert torch.equal(rho(d, 'charbonnier', s), torch.sqrt(d ** 2 + s ** 2))


@pytest.mark.parametrize('kind', KINDS)
def test_psi_is_the_derivative_of_rho(kind):
    for s in SCALES:
        d = _residuals().requires_grad_(True)
        rho(d, kind, s).sum().backward()
        d0 = d.detach()
        want = psi(d0, kind, s)
        # element by element, relative to what autograd adds up: psi itself, or for Geman-McClure the two terms d r and d r (d^2/(d^2 + s^2))
        # whose difference it forms (each |d| r; for |d| >> s they cancel to d r^2, which the closed form gets without the cancellation)
        size = d0.abs() * (s * s / (d0 * d0 + s * s)) if kind == 'geman_mcclure' else want.abs()
        assert ((d.grad - want).abs() <= 1e-14 * size).all(), (kind, s)
        assert psi(torch.zeros(3, dtype=torch.float64), kind, s).abs().max().item() == 0.0


def test_limits():
    d = _residuals()
    assert torch.equal(rho(d, 'huber', 1e6), 0.5 * d * d) and torch.equal(psi(d, 'huber', 1e6), d)       # half the squared error
    assert (rho(d, 'charbonnier', 1e-6) - d.abs()).abs().max().item() <= 1e-6                            # the absolute error
    for s in (1e-6, 0.1, 2.0):
        far = torch.tensor([1e4 * s, -1e4 * s, 1e8 * s], dtype=torch.float64)
        assert ((rho(far, 'geman_mcclure', s) - 0.5 * s * s).abs() / (0.5 * s * s)).max().item() <= 2e-8    # saturates at s^2/2 ...
        assert (psi(far, 'geman_mcclure', s).abs() / s).max().item() <= 1e-11                                # ... and stops pulling
    # what a beta = 0 pixel contributes: rho(0) = s for Charbonnier, 0 for the others
    zero = torch.zeros(1, dtype=torch.float64)
    assert rho(zero, 'charbonnier', 0.3).item() == 0.3 and rho(zero, 'huber', 0.3).item() == 0.0 and rho(zero, 'geman_mcclure', 0.3).item() == 0.0
    # through r, no s^4: a scale whose fourth power leaves float32 in either direction
    for s in (1e-12, 1e12):
        one = torch.ones(1, dtype=torch.float32)
        v = rho(one, 'geman_mcclure', s).item()
        assert v == pytest.approx(0.5 * min(1.0, s * s), rel=1e-6)


def test_checker():
    from oodgan.engine import PIXEL_LOSSES, check_pixel_loss
    assert PIXEL_LOSSES == ('mse',) + KINDS
    for name in PIXEL_LOSSES:
        assert check_pixel_loss(name, 0.1) == (name, scale32(0.1))
    assert check_pixel_loss('huber', 2) == ('huber', 2.0)
    for bad in ('l1', 'MSE', '', None, 3):
        with pytest.raises(ValueError, match='pixel_loss'):
            check_pixel_loss(bad, 0.1)
    for bad in BAD_SCALES + [None, True, 1e-30, 1e30]:           # the last two: s^2 is not a normal float32
        with pytest.raises(ValueError, match='pixel_scale'):
            check_pixel_loss('huber', bad)
        with pytest.raises(ValueError, match='pixel_scale'):     # checked for 'mse' too: a bad option is never silently ignored
            check_pixel_loss('mse', bad)
    with pytest.raises(ValueError, match='inversion.pixel_scale'):
        check_pixel_loss('huber', 0, 'inversion.pixel_loss', 'inversion.pixel_scale')


def test_inverter_takes_and_rejects_the_options():
    from oodgan.engine import WPlusInverter
    inv = WPlusInverter(None)
    assert (inv.pixel_loss, inv.pixel_scale) == ('mse', scale32(0.1))
    inv = WPlusInverter(None, pixel_loss='geman_mcclure', pixel_scale=0.3)
    assert (inv.pixel_loss, inv.pixel_scale) == ('geman_mcclure', scale32(0.3))
    with pytest.raises(ValueError, match='pixel_loss'):
        WPlusInverter(None, pixel_loss='l1')
    for bad in BAD_SCALES:
        with pytest.raises(ValueError, match='pixel_scale'):
            WPlusInverter(None, pixel_loss='charbonnier', pixel_scale=bad)


def _opts(**inv):
    return {'name': 'x', 'datasets': {}, 'network_g': {'type': 'ood_faceGAN_e4e'}, 'inversion': inv}


@pytest.mark.parametrize('bad', BAD_SCALES)
def test_cli_rejects_a_bad_pixel_scale_before_it_asks_for_a_gpu(bad):
    from oodgan import cli
    with pytest.raises(ValueError, match='inversion.pixel_scale'):
        cli.run(_opts(pixel_loss='huber', pixel_scale=bad))


def test_cli_rejects_a_bad_pixel_loss_before_it_asks_for_a_gpu():
    from oodgan import cli
    for bad in ('l1', 'Huber', 7):
        with pytest.raises(ValueError, match='inversion.pixel_loss'):
            cli.run(_opts(pixel_loss=bad))


def test_abi_refuses_a_bad_kind_or_scale_without_a_gpu():
    """Status -1 and a message, before anything is launched (the pointers are never read)."""
    from oodgan import _lib, ops
    h = _lib.lib()
    one = 1                                                       # a non-null stand-in pointer
    before = _lib.dispatch_count('robust')
    plain = lambda kind, s: h.oodgan_robust_loss_fwd_bwd(one, one, None, None, None, one, one, 1, 3, 16, kind, s, 1, 1.0, None)
    row = lambda kind, s: h.oodgan_robust_loss_fwd_bwd_row(one, one, None, None, None, one, one, one, 4, 1, 3, 16, kind, s, 1, 1.0, None)
    for call in (plain, row):
        for kind in (0, 4, -1):
            assert call(kind, 0.5) == -1 and b'kind' in h.oodgan_last_error()
        for s in (0.0, -1.0, float('nan'), float('inf'), 1e-30, 1e30):
            for kind in ops.ROBUST_KINDS.values():
                assert call(kind, s) == -1 and b'scale' in h.oodgan_last_error()
    assert _lib.dispatch_count('robust') == before
