"""``pixel_size``, the parts that need no GPU: the float64 yardstick against autograd, the option's checker, the inverter's
constructor, the CLI key, the ABI's refusals and the identity the low-resolution use rests on."""
import pytest
import torch
import torch.nn.functional as F

import pixsize_ref as PR


def _inputs(B, C, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    img, x = torch.randn(B, C, H, W, generator=g), torch.randn(B, C, H, W, generator=g)
    beta = torch.sigmoid(2.0 * torch.randn(B, 1, H, W, generator=g))
    beta[:, :, : H // 4, : W // 4] = 0.0
    beta[:, :, -(H // 4):, -(W // 4):] = 1.0
    return img, x, beta


@pytest.mark.parametrize('f', [2, 4, 8, 16])
@pytest.mark.parametrize('kind', PR.KINDS)
def test_reference_gradient_is_autograd_in_float64(kind, f):
    """The closed-form gradient of pixsize_ref (window broadcast of gscale * psi, times beta w.r.t. G) against autograd through
    avg_pool2d and rho, without and with a loss weight; w.r.t. the composite it is autograd's gradient at c."""
    B, C, H, W = 2, 3, 32, 48
    img, x, beta = _inputs(B, C, H, W, 7)
    gmul, s = 1024.0, 0.5
    for w in (None, beta):
        a = img.double().clone().requires_grad_(True)
        r = PR.residual(a, x.double(), f, None if w is None else w.double())
        loss = PR.rho(r, kind, PR.robust_ref.scale32(s)).mean(dim=(1, 2, 3))
        (gmul * loss.sum()).backward()
        l_ref, g_ref, c_ref, r_ref = PR.loss_and_grad(img, x, f, kind, s, w, gmul, wrt='gen')
        assert torch.equal(r_ref, r.detach()) and torch.allclose(l_ref, loss.detach(), rtol=1e-14, atol=0)
        assert (g_ref - a.grad).abs().max().item() <= 1e-13 * a.grad.abs().max().item()
        if w is not None:
            c = c_ref.clone().requires_grad_(True)          # the loss as a function of the composite: r = P(c) - P(x)
            lc = PR.rho(F.avg_pool2d(c, f) - F.avg_pool2d(x.double(), f), kind, PR.robust_ref.scale32(s)).mean(dim=(1, 2, 3))
            (gmul * lc.sum()).backward()
            _, gc_ref, _, _ = PR.loss_and_grad(img, x, f, kind, s, w, gmul, wrt='composite')
            assert (gc_ref - c.grad).abs().max().item() <= 1e-12 * c.grad.abs().max().item()
            assert ((lc.detach() - l_ref).abs() / l_ref).max().item() <= 1e-12


@pytest.mark.parametrize('f', [2, 4, 8, 16])
def test_pooling_a_nearest_upsampled_image_returns_the_image(f):
    """What the low-resolution use rests on: every window of the nearest-upsampled image holds f^2 copies of one value v.  In exact
    arithmetic (float64 inputs that are float32 values: k*v is exact for k <= f^2) the pool returns v bit for bit; the fp32 sum in the
    kernel's row-major order returns it to within the summation bound (f^2 - 1) * 2^-24 * |v| — 3v is already rounded — and the scaling
    by 1/f^2 adds nothing."""
    g = torch.Generator().manual_seed(3)
    small = torch.randn(2, 3, 16, 24, generator=g)
    up = F.interpolate(small, scale_factor=f, mode='nearest')
    assert up.shape == (2, 3, 16 * f, 24 * f) and torch.equal(PR.unpool(small, f), up)
    assert torch.equal(F.avg_pool2d(up.double(), f), small.double())
    bound = (f * f - 1) * 2.0 ** -24 * small.double().abs()
    assert ((F.avg_pool2d(up, f).double() - small.double()).abs() <= bound).all()
    acc = torch.zeros_like(small)                              # the kernel's order: row-major, one fp32 add per pixel
    for dy in range(f):
        for dx in range(f):
            acc = acc + up[:, :, dy::f, dx::f]
    err = ((acc * (1.0 / (f * f))).double() - small.double()).abs()
    print(f'f={f}: fp32 row-major pool of the upsampled image vs the image: max rel {(err / small.double().abs()).max().item():.2e}')
    assert (err <= bound).all()


def test_checker_accepts_and_refuses():
    from oodgan.engine import PIXEL_POOL_FACTORS, check_pixel_size
    assert PIXEL_POOL_FACTORS == (1, 2, 4, 8, 16)
    assert check_pixel_size(None) is None and check_pixel_size(None, 1024) is None
    for size, image in ((512, 1024), (256, 1024), (128, 1024), (64, 1024), (16, 64), (4, 64), (2, 32), (1, 16), (16, 256)):
        assert check_pixel_size(size, image) == size
    for image in (1024, 256, 64, 16):
        assert check_pixel_size(image, image) is None          # factor 1: today's path
    assert check_pixel_size(256) == 256 and check_pixel_size(8) == 8      # the image size is not known yet: the type only
    for bad in (True, False, 256.0, '256', [256], 2.5):
        with pytest.raises(ValueError, match='pixel_size'):
            check_pixel_size(bad, 1024)
        with pytest.raises(ValueError, match='pixel_size'):
            check_pixel_size(bad)
    for bad, image in ((0, 1024), (-256, 1024),                # not positive
                       (96, 1024), (300, 1024), (100, 256),    # not a divisor
                       (32, 1024), (64, 2048), (2, 64),        # a quotient of 32
                       (2048, 1024), (512, 256)):              # larger than the image
        with pytest.raises(ValueError, match='pixel_size'):
            check_pixel_size(bad, image)
    with pytest.raises(ValueError, match='inversion.pixel_size'):
        check_pixel_size(96, 1024, 'inversion.pixel_size')


def test_inverter_takes_and_rejects_the_option():
    from oodgan.engine import WPlusInverter
    assert WPlusInverter(None).pixel_size is None
    assert WPlusInverter(None, pixel_size=256).pixel_size == 256
    for bad in (True, 256.0, '256', 0, -4):
        with pytest.raises(ValueError, match='pixel_size'):
            WPlusInverter(None, pixel_size=bad)


def _opts(out_size=None, **inv):
    g = {'type': 'ood_faceGAN_e4e'}
    if out_size is not None:
        g['out_size'] = out_size
    return {'name': 'x', 'datasets': {}, 'network_g': g, 'inversion': inv}


def _no_model(opts):
    raise AssertionError('the model was built before inversion.pixel_size was checked')


@pytest.mark.parametrize('bad', [True, 256.0, '256', 0, -8])
def test_cli_rejects_a_bad_pixel_size_before_it_builds_a_model(bad, monkeypatch):
    from oodgan import cli
    monkeypatch.setattr(cli, 'load_model', _no_model)
    with pytest.raises(ValueError, match='inversion.pixel_size'):
        cli.run(_opts(pixel_size=bad))


@pytest.mark.parametrize('bad,out_size', [(96, 1024), (2048, 1024), (32, 1024), (512, 256)])
def test_cli_checks_pixel_size_against_the_generator_size_it_is_given(bad, out_size, monkeypatch):
    from oodgan import cli
    monkeypatch.setattr(cli, 'load_model', _no_model)
    with pytest.raises(ValueError, match='inversion.pixel_size'):
        cli.run(_opts(out_size=out_size, pixel_size=bad))


def test_abi_refuses_bad_arguments_without_a_gpu():
    """Status -1 and a message before anything is launched (the pointers are never read); the counter counts accepted calls only."""
    from oodgan import _lib
    h = _lib.lib()
    ptr = 64                                                    # a non-null, 16-byte aligned stand-in pointer
    before = _lib.dispatch_count('pooled_pixel')

    def call(f=4, H=16, W=16, img=ptr, target=None, tpool=ptr, beta=None, gimg=ptr, comp=None, kind=0, scale=0.5, B=2, C=3):
        return h.oodgan_pooled_pixel_loss_fwd_bwd(img, target, tpool, beta, gimg, comp, ptr, ptr, B, C, H, W, f, kind, scale, 1, 1.0, None)

    def refused(word, **kw):
        assert call(**kw) == -1 and word in h.oodgan_last_error(), (kw, h.oodgan_last_error())

    for f in (1, 3, 5, 32, 0, -2):
        refused(b'factor', f=f)
    for H, W, f in ((6, 9, 2), (7, 8, 2), (8, 12, 8), (16, 24, 16), (10, 8, 4)):
        refused(b'multiple', H=H, W=W, f=f)
    refused(b'shape', B=0)
    refused(b'shape', C=0)
    refused(b'shape', H=0)
    refused(b'aligned', f=2, img=68)                            # 4-byte aligned: no float2 rows
    refused(b'aligned', f=4, img=72)                            # 8-byte aligned: no float4 rows
    refused(b'aligned', f=4, gimg=72)
    refused(b'aligned', f=8, target=ptr, tpool=None, beta=72)
    refused(b'aligned', f=8, target=72, tpool=None, beta=ptr)
    refused(b'aligned', f=16, target=ptr, tpool=None, beta=ptr, comp=8)
    refused(b'composite', comp=ptr)                             # comp without beta
    refused(b'kind', kind=4)
    refused(b'kind', kind=-1)
    for s in (0.0, -1.0, float('nan'), float('inf'), 1e-30):
        refused(b'scale', kind=1, scale=s)
    assert call(kind=0, scale=0.0, H=0) == -1                   # the square reads no scale: the refusal is the shape's
    refused(b'target', target=ptr, tpool=ptr)                   # without beta: both
    refused(b'target', target=None, tpool=None)                 # without beta: neither
    refused(b'target', target=ptr, tpool=None)                  # without beta the pooled one is the one read
    refused(b'target', beta=ptr, target=ptr, tpool=ptr)         # with beta: both
    refused(b'target', beta=ptr, target=None, tpool=None)       # with beta: neither
    refused(b'target', beta=ptr, target=None, tpool=ptr)        # with beta the full one is the one read
    assert call(img=None) == -1
    assert h.oodgan_pooled_pixel_loss_fwd_bwd_row(ptr, None, ptr, None, ptr, None, ptr, ptr, None, 4, 2, 3, 16, 16, 4, 0, 0.5, 1, 1.0, None) == -1
    assert h.oodgan_pooled_pixel_loss_fwd_bwd_row(ptr, None, ptr, None, ptr, None, ptr, ptr, ptr, 0, 2, 3, 16, 16, 4, 0, 0.5, 1, 1.0, None) == -1
    assert _lib.dispatch_count('pooled_pixel') == before
    # the scratch a call needs: one partial per block of 256 threads x 4 / 2 / 1 / 1 windows; 0 for a factor the kernel does not have
    n = h.oodgan_pooled_pixel_loss_nparts
    assert [n(3 * 256 * 256, f) for f in (2, 4, 8, 16)] == [192, 384, 768, 768] and n(1, 16) == 1 and n(1025, 2) == 2
    assert n(100, 3) == 0 and n(0, 4) == 0
