"""``lpips_size``, the parts that need no GPU: the option's checker, the inverter's constructor, the CLI key and the ABI's
refusals."""
import pytest


def test_checker_accepts_and_refuses():
    from oodgan.engine import LPIPS_MIN_SIZE, LPIPS_POOL_FACTORS, check_lpips_size
    assert LPIPS_POOL_FACTORS == (1, 2, 4, 8, 16) and LPIPS_MIN_SIZE == 64
    assert check_lpips_size(None) is None and check_lpips_size(None, 1024) is None
    for size, image in ((256, 1024), (1024, 1024), (512, 1024), (128, 1024), (64, 1024), (64, 128), (64, 64), (256, 256)):
        assert check_lpips_size(size, image) == size
    assert check_lpips_size(256) == 256                              # the image size is not known yet: the type and the floor only
    for bad in (True, False, 256.0, '256', [256], 2.5):
        with pytest.raises(ValueError, match='lpips_size'):
            check_lpips_size(bad, 1024)
        with pytest.raises(ValueError, match='lpips_size'):
            check_lpips_size(bad)
    for bad, image in ((32, 1024), (0, 1024), (-256, 1024),          # below the floor
                       (96, 1024), (300, 1024), (100, 256),          # not a divisor
                       (32, 1024), (64, 2048),                       # a quotient of 32
                       (2048, 1024), (512, 256)):                    # larger than the image
        with pytest.raises(ValueError, match='lpips_size'):
            check_lpips_size(bad, image)
    with pytest.raises(ValueError, match='inversion.lpips_size'):
        check_lpips_size(96, 1024, 'inversion.lpips_size')


def test_inverter_takes_and_rejects_the_option():
    from oodgan.engine import WPlusInverter
    assert WPlusInverter(None).lpips_size is None
    assert WPlusInverter(None, lpips_size=256).lpips_size == 256
    for bad in (True, 256.0, '256', 32):
        with pytest.raises(ValueError, match='lpips_size'):
            WPlusInverter(None, lpips_size=bad)


def _opts(out_size=None, **inv):
    g = {'type': 'ood_faceGAN_e4e'}
    if out_size is not None:
        g['out_size'] = out_size
    return {'name': 'x', 'datasets': {}, 'network_g': g, 'inversion': inv}


@pytest.mark.parametrize('bad', [True, 256.0, '256', 32, 0])
def test_cli_rejects_a_bad_lpips_size_before_it_asks_for_a_gpu(bad):
    from oodgan import cli
    with pytest.raises(ValueError, match='inversion.lpips_size'):
        cli.run(_opts(lpips_weight=0.8, lpips_size=bad))


@pytest.mark.parametrize('bad,out_size', [(96, 1024), (2048, 1024), (64, 2048), (512, 256)])
def test_cli_checks_lpips_size_against_the_generator_size_it_is_given(bad, out_size):
    from oodgan import cli
    with pytest.raises(ValueError, match='inversion.lpips_size'):
        cli.run(_opts(out_size=out_size, lpips_weight=0.8, lpips_size=bad))


def test_abi_refuses_bad_factors_and_shapes_without_a_gpu():
    """Status -1 and a message before anything is launched (the pointers are never read); the counter counts accepted calls only."""
    from oodgan import _lib
    h = _lib.lib()
    ptr = 64                                                          # a non-null, 16-byte aligned stand-in pointer
    before = _lib.dispatch_count('area_pool')
    fwd = lambda BC, H, W, f, x=ptr: h.oodgan_area_pool_fwd(x, ptr, ptr, BC, H, W, f, None)
    bwd = lambda BC, H, W, f, x=ptr: h.oodgan_area_pool_bwd_add(ptr, x, BC, H, W, f, None)
    for call in (fwd, bwd):
        for f in (1, 3, 5, 32, 0, -2):
            assert call(3, 96, 96, f) == -1 and b'factor' in h.oodgan_last_error()
        for H, W, f in ((6, 9, 2), (7, 8, 2), (8, 12, 8), (16, 24, 16), (10, 8, 4)):
            assert call(3, H, W, f) == -1 and b'multiple' in h.oodgan_last_error()
        assert call(0, 8, 8, 2) == -1 and call(3, 0, 8, 2) == -1
        assert call(3, 8, 8, 2, 68) == -1 and b'aligned' in h.oodgan_last_error()      # 4-byte aligned: no float2 rows
        assert call(3, 8, 8, 4, 72) == -1 and b'aligned' in h.oodgan_last_error()      # 8-byte aligned: no float4 rows
        assert call(3, 8, 8, 2, None) == -1
    assert _lib.dispatch_count('area_pool') == before
