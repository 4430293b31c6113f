"""``pixel_filter`` / ``pixel_target``, the parts that need no GPU: the tap tables against torch's and PIL's antialiased
resizers, the float64 yardstick against autograd, the options' checkers, the inverter's constructor, the CLI keys and the ABI's refusals."""
import pytest
import torch
import torch.nn.functional as F

import resample_ref as RR

SHAPES = ((32, 32), (32, 64), (64, 64))


def _table64(filt, H, f):
    """The float64 table ``ops.resample_tables`` rounds: its own code path up to the rounding (float64 in, no float32 step)."""
    from oodgan import ops
    k = ops._filter_taps(filt, f)
    T = k.numel()
    i = f * torch.arange(H // f)[:, None] - (T - f) // 2 + torch.arange(T)[None, :]
    A = k[None, :] * ((i >= 0) & (i < H))
    return A / A.sum(dim=1, keepdim=True)


@pytest.mark.parametrize('f', RR.FACTORS)
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: f'{s[0]}x{s[1]}')
@pytest.mark.parametrize('filt', ['bilinear', 'bicubic'])
def test_tables_are_torchs_antialiased_resize_in_float64(filt, shape, f):
    """The definition (tests/resample_ref.py, dense float64) and the package's float64 taps against ``F.interpolate(antialias=True,
    align_corners=False)`` on float64 images within 1e-12; the float32 table is that table rounded once (half an ulp of a weight <= 1)."""
    from oodgan import ops
    H, W = shape
    x = torch.randn(2, 3, H, W, dtype=torch.float64, generator=torch.Generator().manual_seed(11))
    want = F.interpolate(x, size=(H // f, W // f), mode=filt, antialias=True, align_corners=False)
    Dy, Dx = RR.dense_from_taps(filt, H, f), RR.dense_from_taps(filt, W, f)
    err = (RR.view(x, Dy, Dx) - want).abs().max().item()
    Py, Px = (RR.dense_from_table(_table64(filt, L, f), L, f) for L in (H, W))
    err_pkg = (RR.view(x, Py, Px) - want).abs().max().item()
    print(f'{filt} {H}x{W} F={f}: definition vs torch {err:.1e}, package taps vs torch {err_pkg:.1e}')
    assert err <= 1e-12 and err_pkg <= 1e-12
    for L in (H, W):
        A = ops.resample_tables(filt, L, f)
        assert A.dtype == torch.float32 and A.shape == (L // f, RR.SUPPORT[filt] * f) and A.device.type == 'cpu'
        assert torch.equal(A, _table64(filt, L, f).float())


@pytest.mark.parametrize('f', RR.FACTORS)
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: f'{s[0]}x{s[1]}')
def test_lanczos3_is_pils_resize(shape, f):
    """``lanczos3`` (and bicubic once more) against PIL's mode-'F' ``resize``, whose own arithmetic is float32: bar 1e-6."""
    Image = pytest.importorskip('PIL.Image')
    import numpy as np
    H, W = shape
    x = torch.randn(H, W, dtype=torch.float64, generator=torch.Generator().manual_seed(13)).float()
    for filt, mode in (('lanczos3', Image.LANCZOS), ('bicubic', Image.BICUBIC)):
        want = torch.from_numpy(np.array(Image.fromarray(x.numpy(), mode="F").resize((W // f, H // f), mode))).double()
        got = RR.view(x.double(), RR.dense_from_table(_table64(filt, H, f), H, f), RR.dense_from_table(_table64(filt, W, f), W, f))
        err = (got - want).abs().max().item()
        print(f'{filt} {H}x{W} F={f}: vs PIL {err:.1e}')
        assert err <= 1e-6


@pytest.mark.parametrize('f', RR.FACTORS)
def test_every_row_sums_to_one_and_drops_what_lies_outside(f):
    from oodgan import ops
    g = torch.Generator().manual_seed(5)
    for filt in ('bilinear', 'bicubic', 'lanczos3', (0.25 + torch.rand(4 * f, generator=g)).tolist()):
        for H in (16, 32, 64):
            A = ops.resample_tables(filt, H, f)
            n, T = A.shape
            assert (A.sum(dim=1) - 1).abs().max().item() <= 1e-6
            i = f * torch.arange(n)[:, None] - (T - f) // 2 + torch.arange(T)[None, :]
            assert (A[(i < 0) | (i >= H)] == 0).all()
            RR.dense_from_table(A, H, f)                           # asserts the same, tap by tap


def test_tables_refuse_bad_arguments():
    from oodgan import ops
    assert ops.RESAMPLE_FILTERS == {'bilinear': 2, 'bicubic': 4, 'lanczos3': 6}
    for bad in ('box', 'lanczos', 'nearest', None, 3):
        with pytest.raises((ValueError, TypeError, RuntimeError)):
            ops.resample_tables(bad, 32, 4)
    for F_ in (1, 3, 32, True, 4.0):
        with pytest.raises(ValueError, match='factor'):
            ops.resample_tables('bicubic', 32, F_)
    for H in (0, 30, 2, 32.0):
        with pytest.raises(ValueError, match='multiple'):
            ops.resample_tables('bicubic', H, 4)
    for taps in ([1.0] * 7, [1.0] * 32, [[1.0] * 8], [float('nan')] * 8):
        with pytest.raises(ValueError, match='tap'):
            ops.resample_tables(taps, 32, 4)
    with pytest.raises(ValueError, match='weight'):
        ops.resample_tables([1.0, -1.0] * 4, 32, 4)
    assert ops.resample_tables([1.0] * 8, 32, 4).shape == (8, 8)


@pytest.mark.parametrize('kind', RR.KINDS)
def test_reference_gradient_is_autograd_in_float64(kind):
    """The closed-form gradient of resample_ref (Dy^T psi Dx) against autograd through the dense matrices and rho."""
    from oodgan import ops
    B, C, H, W, f = 2, 3, 32, 64, 4
    g = torch.Generator().manual_seed(7)
    img, y = torch.randn(B, C, H, W, generator=g), torch.randn(B, C, H // f, W // f, generator=g)
    Ay, Ax = ops.resample_tables('lanczos3', H, f), ops.resample_tables('lanczos3', W, f)
    gmul, s = 1024.0, 0.5
    a = img.double().clone().requires_grad_(True)
    r = RR.view(a, RR.dense_from_table(Ay, H, f), RR.dense_from_table(Ax, W, f)) - y.double()
    loss = RR.rho(r, kind, RR.robust_ref.scale32(s)).mean(dim=(1, 2, 3))
    (gmul * loss.sum()).backward()
    l_ref, g_ref, r_ref, _ = RR.loss_and_grad(img, y, Ay, Ax, f, kind, s, gmul)
    assert torch.equal(r_ref, r.detach()) and torch.allclose(l_ref, loss.detach(), rtol=1e-14, atol=0)
    assert (g_ref - a.grad).abs().max().item() <= 1e-13 * a.grad.abs().max().item()


def test_checkers_accept_and_refuse():
    from oodgan.engine import PIXEL_FILTERS, check_pixel_filter, check_pixel_target
    assert PIXEL_FILTERS == ('box', 'bilinear', 'bicubic', 'lanczos3')
    assert check_pixel_filter(None) is None and check_pixel_filter('box') is None
    for name in PIXEL_FILTERS[1:]:
        assert check_pixel_filter(name) == name
    for bad in ('lanczos', 'nearest', 'BICUBIC', '', 3, True, ['bicubic']):
        with pytest.raises(ValueError, match='pixel_filter'):
            check_pixel_filter(bad)
    with pytest.raises(ValueError, match='inversion.pixel_filter'):
        check_pixel_filter('cubic', 'inversion.pixel_filter')
    x = torch.zeros(2, 3, 64, 64)
    assert check_pixel_target(None, x, None) == (None, None) and check_pixel_target(None, x, 16) == (None, 16)
    for n in (32, 16, 8, 4):
        y = torch.zeros(2, 3, n, n)
        got, size = check_pixel_target(y, x, None)
        assert got is y and size == n and check_pixel_target(y, x, n)[1] == n
    for bad in (torch.zeros(1, 3, 16, 16), torch.zeros(2, 1, 16, 16), torch.zeros(2, 3, 16, 8), torch.zeros(2, 3, 64, 64), torch.zeros(2, 3, 2, 2),
                torch.zeros(2, 3, 24, 24), torch.zeros(2, 3, 16, 16, dtype=torch.float64), torch.zeros(3, 16, 16), [[0.0]], 'file'):
        with pytest.raises(ValueError, match='pixel_target'):
            check_pixel_target(bad, x, None)
    with pytest.raises(ValueError, match='pixel_size'):
        check_pixel_target(torch.zeros(2, 3, 16, 16), x, 32)


def test_inverter_takes_and_rejects_the_options():
    from oodgan.engine import WPlusInverter
    assert WPlusInverter(None).pixel_filter is None and WPlusInverter(None, pixel_filter='box').pixel_filter is None
    assert WPlusInverter(None, pixel_size=64, pixel_filter='lanczos3').pixel_filter == 'lanczos3'
    for bad in ('cubic', 4, True):
        with pytest.raises(ValueError, match='pixel_filter'):
            WPlusInverter(None, pixel_filter=bad)


def _opts(out_size=None, datasets=None, **inv):
    g = {'type': 'ood_faceGAN_e4e'}
    if out_size is not None:
        g['out_size'] = out_size
    return {'name': 'x', 'datasets': datasets or {}, 'network_g': g, 'inversion': inv}


def _no_model(opts):
    raise AssertionError('the model was built before the pixel_filter / pixel_target keys were checked')


@pytest.mark.parametrize('inv,word', [(dict(pixel_filter='cubic', pixel_size=256), 'inversion.pixel_filter'),
                                      (dict(pixel_filter=3, pixel_size=256), 'inversion.pixel_filter'),
                                      (dict(pixel_filter='bicubic'), 'inversion.pixel_size'),
                                      (dict(pixel_target='files'), 'inversion.pixel_target'),
                                      (dict(pixel_target=True), 'inversion.pixel_target'),
                                      (dict(pixel_filter='bicubic', pixel_size=256, loss_region='blend'), 'loss_region'),
                                      (dict(pixel_filter='lanczos3', pixel_size=256, mask_dir='/nowhere'), 'mask_dir'),
                                      (dict(pixel_target='file', loss_region='blend'), 'loss_region')])
def test_cli_rejects_bad_keys_before_it_builds_a_model(inv, word, monkeypatch):
    from oodgan import cli
    monkeypatch.setattr(cli, 'load_model', _no_model)
    with pytest.raises(ValueError, match=word):
        cli.run(_opts(out_size=1024, **inv))


def test_cli_pixel_target_sizes_without_a_gpu():
    """The refusals of ``pixel_target: file`` come before anything touches the device."""
    import numpy as np
    from oodgan import cli
    small, big = np.zeros((64, 64, 3)), np.zeros((256, 256, 3))
    for bad, word in (([small, big], 'one size'), ([big, big], 'generator size'), ([np.zeros((64, 32, 3))] * 2, 'square'),
                      ([np.zeros((96, 96, 3))] * 2, 'side n'), ([np.zeros((8, 8, 3))], 'side n')):
        with pytest.raises(ValueError, match=word):
            cli.pixel_target_from_files(bad, ['a.png', 'b.png'], 256)


def test_ops_refuse_without_a_gpu():
    """``beta`` with ``resample`` and the other host-side refusals need tensors on the device first: on a CPU tensor the product path says so."""
    from oodgan import ops
    x = torch.zeros(1, 3, 16, 16)
    with pytest.raises(RuntimeError, match='ROCm'):
        ops.pixel_loss_grad(x, x, pool=4, resample=(torch.zeros(4, 16), torch.zeros(4, 16)))
    with pytest.raises(RuntimeError, match='ROCm'):
        ops.resample(x, torch.zeros(4, 16), torch.zeros(4, 16), 4)


def test_abi_refuses_bad_arguments_without_a_gpu():
    """Status -1 and a message before anything is launched (the pointers are never read); the counter counts accepted calls only."""
    from oodgan import _lib
    h = _lib.lib()
    ptr = 64                                                    # a non-null stand-in pointer
    before = _lib.dispatch_count('resampled_pixel')

    def call(F_=4, s=4, H=16, W=16, img=ptr, tview=ptr, Ay=ptr, Ax=ptr, gimg=ptr, rs=ptr, part=ptr, loss=ptr, kind=0, scale=0.5, B=2, C=3):
        return h.oodgan_resampled_pixel_loss_fwd_bwd(img, tview, Ay, Ax, gimg, rs, part, loss, B, C, H, W, F_, s, kind, scale, 1.0, None)

    def refused(word, **kw):
        assert call(**kw) == -1 and word in h.oodgan_last_error(), (kw, h.oodgan_last_error())

    for f in (1, 3, 5, 32, 0, -2):
        refused(b'factor', F_=f)
    for s in (0, 1, 3, 5, 8, -2):
        refused(b'support', s=s)
    for H, W, f in ((6, 9, 2), (7, 8, 2), (8, 12, 8), (16, 24, 16), (10, 8, 4)):
        refused(b'multiple', H=H, W=W, F_=f)
    refused(b'shape', B=0)
    refused(b'shape', C=0)
    refused(b'shape', C=-3)
    refused(b'shape', H=0)
    refused(b'tables', Ay=None)
    refused(b'tables', Ax=None)
    refused(b'kind', kind=4)
    refused(b'kind', kind=-1)
    for sc in (0.0, -1.0, float('nan'), float('inf'), 1e-30):
        refused(b'scale', kind=1, scale=sc)
    assert call(kind=0, scale=0.0, H=0) == -1                   # the square reads no scale: the refusal is the shape's
    for kw in (dict(img=None), dict(tview=None), dict(rs=None), dict(part=None), dict(loss=None)):
        refused(b'bad args', **kw)
    row = h.oodgan_resampled_pixel_loss_fwd_bwd_row
    assert row(ptr, ptr, ptr, ptr, ptr, ptr, ptr, ptr, None, 4, 2, 3, 16, 16, 4, 4, 0, 0.5, 1.0, None) == -1        # no row_dev
    assert row(ptr, ptr, ptr, ptr, ptr, ptr, ptr, ptr, ptr, 0, 2, 3, 16, 16, 4, 4, 0, 0.5, 1.0, None) == -1         # no rows
    assert row(ptr, ptr, ptr, ptr, ptr, ptr, ptr, ptr, ptr, 4, 2, 3, 16, 16, 4, 5, 0, 0.5, 1.0, None) == -1 and b'support' in h.oodgan_last_error()
    fwd = h.oodgan_resample_fwd
    for args, word in (((ptr, ptr, ptr, ptr, 6, 16, 16, 3, 4), b'factor'), ((ptr, ptr, ptr, ptr, 6, 16, 16, 4, 3), b'support'),
                       ((ptr, ptr, ptr, ptr, 6, 18, 16, 4, 4), b'multiple'), ((ptr, None, ptr, ptr, 6, 16, 16, 4, 4), b'tables'),
                       ((ptr, ptr, ptr, ptr, 0, 16, 16, 4, 4), b'shape'), ((None, ptr, ptr, ptr, 6, 16, 16, 4, 4), b'bad args'),
                       ((ptr, ptr, ptr, None, 6, 16, 16, 4, 4), b'bad args')):
        assert fwd(*args, None) == -1 and word in h.oodgan_last_error(), (args, h.oodgan_last_error())
    assert _lib.dispatch_count('resampled_pixel') == before
    # the scratch a call needs: one partial per tile (64 pixels wide, 128 at F = 16) and plane; 0 for a factor or plane the kernels do not have
    n = h.oodgan_resampled_pixel_loss_nparts
    assert [n(3, 1024, 1024, f) for f in (2, 4, 8, 16)] == [768, 768, 768, 192] and n(3, 32, 64, 16) == 3 and n(1, 128, 128, 2) == 4
    assert n(3, 64, 64, 3) == 0 and n(0, 64, 64, 4) == 0 and n(3, 66, 64, 4) == 0 and n(3, 0, 64, 4) == 0
