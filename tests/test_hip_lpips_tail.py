"""The part of csrc/lpips.hip after the convolutions — lpips_prep, lpips_img_grad, lpips_head (modes 0, 1, 2), add_mask with its tail kernel and
lpips_finish — one by one through the C ABI against the float64 references of tests/stream_ref.py.

Exact where the data allow it: dyadic a, b0, shift and scale for prep and img_grad, power-of-two tap sizes for finish, the float32 CPU expression bit
for bit for add_mask.  Bars, each from the number format and relative to the sum of |terms| of the expression (the results cancel):
  * lpips_prep with the real SHIFT / SCALE: `a * img` 1, `+ b0` 1, `- sh` 1, `* is` 1: 4 * 2^-24 * (|a x| + |b0| + |shift|) / scale;
  * lpips_head: stream_ref.head_roundings, a first-order count in which sqrtf and the division are one rounding each (the library is built with
    correctly rounded sqrt and division), and no more than HEAD_CAP = 16 (the rule of feature_modulation's FUSE bar: at least 4 x the largest
    error measured on the MI355X, 4.2 for out, 2.04 for mode 0, 0.57 for part, and at most 16 * 2^-24);
  * lpips_finish with tap sizes that are no powers of two: (ceil(nparts / 64) + 6 + 1 + ntaps) * 2^-24 * sum |terms|."""
import ctypes

import pytest
import torch

import stream_data as D
import stream_ref as S
import tail_ref as T

pytestmark = pytest.mark.gpu

F64 = torch.float64
SENT = -12345.0
GUARD = 64
U = S.U
HEAD_CAP = 16.0
REAL_SHIFT, REAL_SCALE = (-.030, -.088, -.188), (.458, .448, .450)          # lpips.ScalingLayer


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'gpu tests need a ROCm device'
    return torch.device('cuda:0')


def lib():
    from oodgan import _lib
    return _lib.lib()


def stream():
    from oodgan import ops
    return ops._stream()


def P(t, off=0):
    return None if t is None else ctypes.c_void_p(t.data_ptr() + 4 * off)


def host(t):
    return t.detach().cpu()


def guarded(dev, n, fill=SENT):
    return torch.full((n + GUARD,), fill, dtype=torch.float32, device=dev)


def guard_ok(buf, n, fill=SENT):
    return bool((host(buf)[n:] == fill).all())


def last_error():
    m = lib().oodgan_last_error()
    return m.decode() if m else ''


def f3(v):
    return (ctypes.c_float * 3)(*v)


# ----------------------------------------------------------------------------- lpips_prep, lpips_img_grad
PREP_SHAPES = [
    pytest.param(1, 16, 16, id='prep-1x16x16-smallest'),
    pytest.param(2, 16, 20, id='prep-2x16x20'),
    pytest.param(1, 20, 16, id='prep-1x20x16'),
    pytest.param(1, 420, 420, id='prep-1x420x420-second-grid-stride-trip'),
]


def _prep(dev, img, a, b0, shift, scale):
    B, _, H, W = img.shape
    n = B * 48 * (H // 4 + 1) * (W // 4 + 1)
    out = guarded(dev, n)
    imgd = img.to(dev)          # referenced until the synchronize
    rc = lib().oodgan_lpips_prep(P(imgd), P(out), B, H, W, a, b0, f3(shift), f3(scale), stream())
    torch.cuda.synchronize()
    return rc, out, n


@pytest.mark.parametrize('B,H,W', PREP_SHAPES)
def test_lpips_prep(dev, B, H, W):
    assert (B * 48 * (H // 4 + 1) * (W // 4 + 1) > 2048 * 256) == (H == 420)
    img = D.prep_image(B, H, W)
    p = D.DYADIC_PREP
    ref, _, inside = S.lpips_prep(img, p['a'], p['b0'], p['shift'], p['scale'])
    rc, out, n = _prep(dev, img, p['a'], p['b0'], p['shift'], p['scale'])
    assert rc == 0, last_error()
    assert guard_ok(out, n)
    got = host(out)[:n].view(ref.shape)
    assert torch.equal(got.to(F64), ref), (B, H, W)
    assert inside.sum() == B * 3 * H * W and bool((got[~inside].view(torch.int32) == 0).all()), 'pad cells are +0'
    # the real ScalingLayer constants and the [0,1] -> [-1,1] map
    imgr = T.normal((B, 3, H, W), 10010 + H).clamp(-3, 3) / 6 + 0.5
    ref, mag, inside = S.lpips_prep(imgr, 2.0, -1.0, REAL_SHIFT, REAL_SCALE)
    rc, out, n = _prep(dev, imgr, 2.0, -1.0, REAL_SHIFT, REAL_SCALE)
    assert rc == 0 and guard_ok(out, n)
    got = host(out)[:n].view(ref.shape)
    err = (got.to(F64) - ref).abs()
    ratio = (err[inside] / (U * mag[inside])).max().item()
    print(f'lpips_prep {B}x{H}x{W} real constants: max err / (2^-24 sum|terms|) = {ratio:.3f} (limit 4)')
    assert ratio <= 4.0
    assert bool((got[~inside].view(torch.int32) == 0).all())


def test_lpips_prep_refusals(dev):
    for H, W in ((12, 16), (18, 16), (16, 12), (16, 18)):          # below 16; no multiple of 4
        img = D.prep_image(1, H, W)
        rc, out, n = _prep(dev, img, 2.0, -1.0, REAL_SHIFT, REAL_SCALE)
        assert rc == -1 and 'lpips_prep' in last_error(), (H, W)
        assert bool((host(out) == SENT).all()), (H, W)


@pytest.mark.parametrize('B,H,W', PREP_SHAPES)
def test_lpips_img_grad(dev, B, H, W):
    assert (B * 3 * H * W > 2048 * 256) == (H == 420)
    Hs, Ws = H // 4 + 1, W // 4 + 1
    g48 = T.ints((B, 48, Hs, Ws), 10400 + H + W)
    g0 = T.ints((B, 3, H, W), 10401 + H + W, 1, 4)          # non-zero: the kernel adds to it
    a, coef, scale = 2.0, 0.5, D.DYADIC_PREP['scale']
    ref = S.lpips_img_grad(g48, g0, a, coef, scale)
    n = g0.numel()
    gimg = guarded(dev, n)
    gimg[:n] = g0.reshape(-1).to(dev)
    g48d = g48.to(dev)
    rc = lib().oodgan_lpips_img_grad(P(g48d), P(gimg), B, H, W, a, coef, f3(scale), stream())
    torch.cuda.synchronize()
    assert rc == 0, last_error()
    assert guard_ok(gimg, n)
    assert torch.equal(host(gimg)[:n].view(g0.shape).to(F64), ref), (B, H, W)
    # the adjoint pair on the device: <prep(x) with b0 = shift = 0, g> == <x, img_grad(g)>, both sides exact on this data
    img = D.prep_image(B, H, W)
    rc, out, m = _prep(dev, img, a, 0.0, (0.0, 0.0, 0.0), scale)
    assert rc == 0
    lhs = (host(out)[:m].to(F64) * g48.reshape(-1).to(F64)).sum()
    rhs = (img.to(F64) * (host(gimg)[:n].view(g0.shape).to(F64) - g0.to(F64)) / coef).sum()
    assert lhs == rhs, (lhs, rhs)


# ----------------------------------------------------------------------------- lpips_head
HEAD_SHAPES = [
    pytest.param(2, 3, 1, id='head-2x3x1-C-below-8-HW-below-32'),
    pytest.param(1, 13, 33, id='head-1x13x33-C-not-multiple-of-8-second-block-of-one-pixel'),
    pytest.param(2, 64, 49, id='head-2x64x49'),
    pytest.param(1, 16, 64, id='head-1x16x64-two-full-blocks'),
]


def _head(dev, f0, n1, w, coef, mode):
    B, C, HW = f0.shape
    nblk = lib().oodgan_lpips_head_nparts(HW)
    assert nblk == -(-HW // S.HEAD_PIX)
    out, part = guarded(dev, f0.numel()), guarded(dev, B * nblk)
    fd, nd, wd = f0.to(dev), None if mode == 0 else n1.to(dev), None if mode == 0 else w.to(dev)          # referenced until the synchronize
    rc = lib().oodgan_lpips_head(P(fd), P(nd), P(wd), P(out), None if mode == 0 else P(part), B, C, HW, coef, mode, stream())
    torch.cuda.synchronize()
    assert rc == 0, last_error()
    assert guard_ok(out, f0.numel())
    if mode == 0:
        assert bool((host(part) == SENT).all())
    else:
        assert guard_ok(part, B * nblk)
    return host(out)[:f0.numel()].view(f0.shape), host(part)[:B * nblk].view(B, nblk)


@pytest.mark.parametrize('mode', [0, 1, 2])
@pytest.mark.parametrize('B,C,HW', HEAD_SHAPES)
def test_lpips_head(dev, B, C, HW, mode):
    f0, n1, w = D.head_data(B, C, HW, mode)
    coef = 0.25
    zero_px = (f0 * f0).sum(1) == 0          # (B, HW)
    assert zero_px[B - 1, HW - 1] and (n1[B - 1, :, HW - 1] != 0).all()
    if mode == 2 and HW > 1:
        assert (f0 < 0).any() and (f0 == 0).any()
    ref = S.lpips_head(f0, n1, w, coef, mode)
    out, part = _head(dev, f0, n1, w, coef, mode)
    assert torch.isfinite(out).all(), 'no NaN at the pixel with |f0| = 0'
    if mode == 0:
        limit = min(S.head_roundings(C, 'norm'), HEAD_CAP)
        ratio = ((out.to(F64) - ref['out']).abs() / (U * ref['out_mag']).clamp_min(1e-300)).max().item()
        assert ratio <= limit, (B, C, HW, ratio, limit)
        assert bool((out[f0 == 0] == 0).all())
        print(f'lpips_head mode 0 {B}x{C}x{HW}: max err / (2^-24 |ref|) = {ratio:.3f} (limit {limit})')
        return
    limit = min(S.head_roundings(C, 'out'), HEAD_CAP)
    ratio = ((out.to(F64) - ref['out']).abs() / (U * ref['out_mag']).clamp_min(1e-300)).max().item()
    assert ratio <= limit, (B, C, HW, mode, ratio, limit)
    # the s == 0 convention: out = coef * r * (-2 w n1), the second term dropped — against the closed form, not only the reference
    zb, zp = B - 1, HW - 1
    want0 = coef * (1.0 / S.f32(1e-10)) * (-2.0 * w.to(F64) * n1[zb, :, zp].to(F64))
    if mode == 1:
        assert ((out[zb, :, zp].to(F64) - want0).abs() <= 4 * U * want0.abs()).all()          # 1.f / eps, 2 w df, * r, * coef
    else:
        assert bool((out[f0 <= 0] == 0).all()), 'mode 2: the ReLU mask !(f > 0)'
        assert bool((out[f0 <= 0].view(torch.int32) == 0).all())
    limit_p = min(S.head_roundings(C, 'part'), HEAD_CAP)
    ratio_p = ((part.to(F64) - ref['part']).abs() / (U * ref['part_mag']).clamp_min(1e-300)).max().item()
    assert ratio_p <= limit_p, (B, C, HW, mode, ratio_p, limit_p)
    assert part.shape == (B, -(-HW // 32))
    print(f'lpips_head mode {mode} {B}x{C}x{HW}: out {ratio:.3f} (limit {limit}), part {ratio_p:.3f} (limit {limit_p}) in units of 2^-24 sum|terms|')


# ----------------------------------------------------------------------------- add_mask
@pytest.mark.parametrize('n', [3, 8, 4099, 2097159], ids=['n3-tail-only', 'n8-no-tail', 'n4099', 'n2097159-second-trip-and-tail'])
def test_add_mask(dev, n):
    assert (n // 4 > 2048 * 256) == (n == 2097159)
    y0, add = T.normal((n,), 10500 + n % 97), T.normal((n,), 10501 + n % 97)
    if n == 3:
        mask = torch.tensor([-1.0, 0.5, -0.0])          # three elements: the fourth kind, +0, is in the other cases
    else:
        mask = T.ints((n,), 10502 + n % 97, -2, 2)
        mask[0::5] = 0.0
        mask[1::7] = -0.0
        mask[2], mask[3] = -1.0, 2.0
        mask[n - 1] = -0.0 if n % 2 else 1.0          # the last element: masked in one case, live in the other
        mask[n - 2] = 0.5
        assert (mask.view(torch.int32) == 0).any()
    assert (mask.view(torch.int32) == -2 ** 31).any() and (mask > 0).any() and (mask < 0).any()
    y = guarded(dev, n)
    y[:n] = y0.to(dev)
    ad, md = guarded(dev, n, 7.0), guarded(dev, n, 7.0)          # the guard of the mask is positive: an element past the end would be added
    ad[:n], md[:n] = add.to(dev), mask.to(dev)
    rc = lib().oodgan_add_mask(P(y), P(ad), P(md), n, stream())
    torch.cuda.synchronize()
    assert rc == 0, last_error()
    assert guard_ok(y, n)
    want = S.add_mask(y0, add, mask)
    assert torch.equal(host(y)[:n].view(torch.int32), want.view(torch.int32)), n


def test_add_mask_refuses_misaligned_pointers(dev):
    n = 16
    y, ad, md = guarded(dev, n), guarded(dev, n, 1.0), guarded(dev, n, 1.0)
    for oy, oa, om in ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 1)):
        rc = lib().oodgan_add_mask(P(y, oy), P(ad, oa), P(md, om), n, stream())
        torch.cuda.synchronize()
        assert rc == -1 and 'aligned' in last_error()
        assert bool((host(y) == SENT).all())


# ----------------------------------------------------------------------------- lpips_finish
FINISH_CASES = [
    pytest.param([130], id='finish-1-tap-130'),
    pytest.param([1, 64, 70], id='finish-3-taps-1-64-70'),
    pytest.param([130, 70, 64, 1, 130], id='finish-5-taps'),
]


def _finish(dev, parts, hw, table, row_dev, nrows, B):
    n = len(parts)
    pd = [p.to(dev).contiguous() for p in parts]
    parr = (ctypes.c_void_p * n)(*[p.data_ptr() for p in pd])
    narr = (ctypes.c_int * n)(*[p.shape[1] for p in parts])
    harr = (ctypes.c_long * n)(*hw)
    rc = lib().oodgan_lpips_finish(parr, narr, harr, n, P(table), P(row_dev), nrows, B, stream())
    torch.cuda.synchronize()
    assert rc == 0, last_error()


@pytest.mark.parametrize('nparts', FINISH_CASES)
def test_lpips_finish(dev, nparts):
    B = 3
    parts = D.finish_parts(nparts, B)
    worst = 0.0
    for hw in ((64, 16, 4, 1024, 256), (3969, 729, 169, 49, 36)):
        hw = hw[:len(nparts)]
        ref, mag = S.lpips_finish(parts, hw)
        # a fresh (B,) destination
        dst = guarded(dev, B)
        _finish(dev, parts, hw, dst, None, 1, B)
        assert guard_ok(dst, B)
        # row 2 of a 4-row table through row_dev
        table = guarded(dev, 4 * B)
        _finish(dev, parts, hw, table, torch.tensor([2], dtype=torch.int32, device=dev), 4, B)
        assert guard_ok(table, 4 * B)
        tb = host(table)[:4 * B].view(4, B)
        assert bool((tb[[0, 1, 3]] == SENT).all()), 'the other rows keep their sentinel'
        assert torch.equal(tb[2], host(dst)[:B])
        if hw[0] == 64:
            assert torch.equal(tb[2].to(F64), ref), (nparts, hw)
        else:
            # lpips_finish_kernel: `s += a.part[t][..]` ceil(nparts / 64), wave_sum 6, `* a.inv_hw[t]` 1, `tot +=` ntaps
            limit = -(-max(nparts) // 64) + 6 + 1 + len(nparts)
            ratio = ((tb[2].to(F64) - ref).abs() / (U * mag)).max().item()
            assert ratio <= limit, (nparts, ratio, limit)
            worst = max(worst, ratio / limit)
    print(f'lpips_finish {nparts}: tap sizes that are no powers of two, largest error / bound = {worst:.3f}')
