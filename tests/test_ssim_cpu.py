"""CPU checks of the SSIM loss term's host side: the float64 yardstick of the GPU tests (tests/ssim_ref.py) against
``imgio.calculate_ssim`` — which tests/test_imgio.py pins to the reference function — and the CLI's ``inversion.ssim_weight``."""
import pytest
import torch

from ssim_ref import ssim, ssim_loss


def _pairs(H, W):
    """Seeded [0,255] float images (1,3,H,W): a 'far' pair (independent) and a 'near' pair (the second + small noise)."""
    from oodgan import synth
    S = max(H, W)
    y = 127.5 * (synth.make_images(S, 1, seed=21)[:, :, :H, :W].double() + 1.0)
    far = 127.5 * (synth.make_images(S, 1, seed=22)[:, :, :H, :W].double() + 1.0)
    near = y + 127.5 * 0.05 * synth.normal('ssim.cpu', (1, 3, H, W), 23).double()
    return {'far': (far, y), 'near': (near, y)}


@pytest.mark.parametrize('H,W', [(64, 64), (37, 37), (64, 48)])
def test_yardstick_equals_the_reported_metric(H, W):
    from oodgan import imgio
    for kind, (v, y) in _pairs(H, W).items():
        got = ssim(v, y).item()
        want = imgio.calculate_ssim(v[0].permute(1, 2, 0).numpy(), y[0].permute(1, 2, 0).numpy(), crop_border=0, test_y_channel=False)
        print(f'{kind} {H}x{W}: SSIM {want:.6f}, |yardstick - calculate_ssim| = {abs(got - want):.2e}')
        assert abs(got - want) <= 1e-8
        # and the loss form on generator-range images is 1 - that
        assert abs(ssim_loss(v / 127.5 - 1.0, y / 127.5 - 1.0).item() - (1.0 - want)) <= 1e-8
    assert ssim(y, y).item() == pytest.approx(1.0, abs=1e-12)


@pytest.mark.parametrize('bad', [-1, float('nan'), float('inf'), 'much'])
def test_cli_rejects_a_bad_ssim_weight_before_it_asks_for_a_gpu(bad):
    from oodgan import cli
    with pytest.raises(ValueError, match='ssim_weight'):
        cli.run({'name': 'x', 'datasets': {}, 'network_g': {'type': 'ood_faceGAN_e4e'}, 'inversion': {'ssim_weight': bad}})


def test_inverter_rejects_a_bad_ssim_weight():
    from oodgan.engine import WPlusInverter
    for bad in (-0.5, float('nan'), float('inf')):
        with pytest.raises(ValueError, match='ssim_weight'):
            WPlusInverter(None, ssim_weight=bad)
    assert WPlusInverter(None).ssim_weight == 0.0 and WPlusInverter(None, ssim_weight=0.25).ssim_weight == 0.25
