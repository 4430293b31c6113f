"""The activation kernels of csrc/elementwise.hip — bias_act_fwd (with and without noise), bias_act_bwd + channel_sum, act_bwd_fused (the
"two-pass" reference of tests/test_hip_bwd_producers.py and tests/test_hip_grad2.py) and feature_modulation — against the float64 references of
tests/stream_ref.py, at the smallest shapes that reach each branch.

Data are small integers and powers of two (tests/stream_data.py), so sums are exact in any order and most comparisons are torch.equal.  Bars, each
from the number format:
  * bias_act_fwd / bias_act_bwd with the default slope 0.2 and scale sqrt(2): the sum before the activation is exact, `v * slope` and `* scale` (forward),
    `slope * scale` and `g *= ..` (backward) are two roundings: (2 * 2^-24 + 2^-48) |ref|;
  * act_bwd_fused g_pre on integer data: g is exact and g * factor is one rounding of an exactly representable double product: equal to the
    float64 reference rounded to float32; on random data 7 roundings (count at roundings_gpre);
  * act_bwd_fused r, t: (depth + roundings per term) * 2^-24 * sum |terms| (depth_act, roundings at the checks);
  * channel_sum on random data: depth_channel_sum * 2^-24 * sum |gx|;
  * feature_modulation FUSE: device expf; the bar is 4 x the largest error measured on the MI355X, at most 16 * 2^-24 (FUSE_BAR, LABNOTES.md).
Observed maxima on the MI355X are recorded in LABNOTES.md."""
import ctypes
import math

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
PAD, OFF = 6, 2          # s_rgb and dscale as column blocks: row stride C + 6, offset 2
TWO = 2.0 * U + U * U          # two roundings, relative

# feature_modulation FUSE, relative to |x| + |c1| sigmoid(c0): measured 1.494 * 2^-24 on the MI355X (LABNOTES.md §17); 4 x that, capped at 16 * 2^-24
FUSE_MEASURED = 1.494
FUSE_BAR = min(4.0 * FUSE_MEASURED, 16.0) * U


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'gpu tests need a ROCm device'
    return torch.device('cuda:0')


def lib():
    from oodgan import _lib
    return _lib.lib()


def ck(rc, what=''):
    from oodgan import _lib
    _lib.check(rc, what)


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


def block_in(dev, dense, fill=99.0):
    m = torch.full((dense.shape[0], dense.shape[1] + PAD), fill, dtype=torch.float32)
    m[:, OFF:OFF + dense.shape[1]] = dense
    return m.to(dev)


def to(dev, t):
    return None if t is None else t.to(dev)


# ----------------------------------------------------------------------------- bias_act_fwd
FWD_SHAPES = [
    pytest.param((2, 3, 8, 8), id='fwd-2x3x8x8-vector'),
    pytest.param((2, 3, 5, 7), id='fwd-2x3x5x7-scalar'),
    pytest.param((5, 24), id='fwd-5x24-2d'),
    pytest.param((1, 2, 257, 256), id='fwd-1x2x257x256-capped-grid-second-trip'),
]


def _fwd_abi(dev, x, bias, noise, nw, slope, scale):
    shape = x.shape
    B, C = shape[0], shape[1]
    HW = x.numel() // (B * C)
    y = guarded(dev, x.numel())
    xd, bd, nd, wd = x.to(dev), to(dev, bias), to(dev, noise), to(dev, nw)          # referenced until the synchronize
    ck(lib().oodgan_bias_act_fwd(P(xd), P(bd), P(nd), P(wd), P(y), B, C, HW, 1 if noise is None else noise.shape[0], slope, scale, stream()), 'bias_act_fwd')
    torch.cuda.synchronize()
    assert guard_ok(y, x.numel())
    return host(y)[:x.numel()].view(shape)


@pytest.mark.parametrize('shape', FWD_SHAPES)
def test_bias_act_fwd(dev, shape):
    from oodgan import ops
    B = shape[0]
    if len(shape) == 4:
        assert ((shape[2] * shape[3]) % 4 == 0) == (shape[2] != 5)
        assert (((shape[2] * shape[3] + 3) // 4 + 255) // 256 > 64) == (shape[2] == 257)          # the grid's x is capped at 64 blocks
    worst = 0.0
    noise_kinds = (0, 1, B) if len(shape) == 4 else (0,)
    for nb in dict.fromkeys(noise_kinds):
        d = D.bias_act_data(shape, nb)
        for bias in (d['bias'], None):
            for nw in ((d['nw'], None) if nb else (None,)):
                for slope, scale in ((0.25, 2.0), (0.2, math.sqrt(2.0))):
                    tag = (shape, nb, bias is None, nw is None, slope)
                    ref = S.bias_noise_act(d['x'], bias, d['noise'], nw, slope, scale)
                    got = _fwd_abi(dev, d['x'], bias, d['noise'], nw, slope, scale)
                    if slope == 0.25:
                        assert torch.equal(got.to(F64), ref), tag
                    else:
                        err = (got.to(F64) - ref).abs()
                        assert (err <= TWO * ref.abs()).all(), tag
                        worst = max(worst, (err / (U * ref.abs()).clamp_min(1e-300)).max().item())
                    # the wrappers
                    if nb == 0:
                        assert torch.equal(host(ops.fused_leaky_relu(d['x'].to(dev), to(dev, bias), slope, scale)), got), tag
                    if len(shape) == 4:
                        assert torch.equal(host(ops.bias_noise_act(d['x'].to(dev), to(dev, bias), to(dev, d['noise']), to(dev, nw), slope, scale)), got), tag
    print(f'bias_act_fwd {shape}: default constants, max err / (2^-24 |ref|) = {worst:.3f} (limit 2)')


def test_bias_act_fwd_noise_planes_differ(dev):
    """per-sample noise: sample b reads plane b (distinct planes: plane 0 for every sample would be wrong by whole integers)"""
    d = D.bias_act_data((2, 3, 8, 8), 2)
    assert (d['noise'][0] != d['noise'][1]).any()
    got = _fwd_abi(dev, d['x'], d['bias'], d['noise'], d['nw'], 0.25, 2.0)
    wrong = S.bias_noise_act(d['x'], d['bias'], d['noise'][:1], d['nw'], 0.25, 2.0)
    assert torch.equal(got[0].to(F64), wrong[0]) and not torch.equal(got[1].to(F64), wrong[1])


# ----------------------------------------------------------------------------- bias_act_bwd, channel_sum
BWD_SHAPES = [
    pytest.param((1, 3, 5, 7), -4, 4, id='bwd-n105-one-tail-element'),
    pytest.param((2, 4, 8, 8), -4, 4, id='bwd-2x4x8x8-no-tail-HW-below-256-B2'),
    pytest.param((1, 1, 1, 3), -4, 4, id='bwd-1x1x1x3-n-below-4'),
    pytest.param((2, 3, 17, 19), -4, 4, id='bwd-2x3x17x19-HW-above-256-B2-tail'),
    pytest.param((1, 2, 1025, 1025), -1, 1, id='bwd-1x2x1025x1025-second-trip-and-tail'),
]


def depth_channel_sum(B, HW):
    # channel_sum_kernel: `s += p[i]` B * ceil(HW / 256) additions in a thread, block_sum_256: wave_sum 6 and `red[0] + red[1] + red[2] + red[3]` 3
    return B * -(-HW // 256) + 6 + 3


def _bwd_abi(dev, gy, y, slope, scale, want_bias):
    B, C = gy.shape[0], gy.shape[1]
    n = gy.numel()
    gx = guarded(dev, n)
    gb = guarded(dev, C) if want_bias else None
    gyd, yd = gy.to(dev), y.to(dev)          # referenced until the synchronize
    ck(lib().oodgan_bias_act_bwd(P(gyd), P(yd), P(gx), P(gb), B, C, n // (B * C), slope, scale, stream()), 'bias_act_bwd')
    torch.cuda.synchronize()
    assert guard_ok(gx, n) and (gb is None or guard_ok(gb, C))
    return host(gx)[:n].view(gy.shape), None if gb is None else host(gb)[:C]


@pytest.mark.parametrize('shape,lo,hi', BWD_SHAPES)
def test_bias_act_bwd_and_channel_sum(dev, shape, lo, hi):
    from oodgan import ops
    n = math.prod(shape)
    assert ((n + 3) // 4 > 2048 * 256) == (shape[2] == 1025)
    d = D.bias_bwd_data(shape, lo, hi)
    assert (d['y'] == 0).sum() >= 2
    # exact: slope 0.25, scale 2
    ref = S.bias_act_bwd(d['gy'], d['y'], 0.25, 2.0)
    gx, gb = _bwd_abi(dev, d['gy'], d['y'], 0.25, 2.0, True)
    assert torch.equal(gx.to(F64), ref), shape
    assert torch.equal(gb.to(F64), S.channel_sum(ref)[0]), shape
    gx2, none = _bwd_abi(dev, d['gy'], d['y'], 0.25, 2.0, False)
    assert none is None and torch.equal(gx2, gx)
    wx, wb = ops.fused_leaky_relu_backward(d['gy'].to(dev), d['y'].to(dev), 0.25, 2.0, need_bias_grad=True)
    assert torch.equal(host(wx), gx) and torch.equal(host(wb), gb)
    # default constants: two roundings
    ref = S.bias_act_bwd(d['gy'], d['y'])
    gx, gb = _bwd_abi(dev, d['gy'], d['y'], 0.2, math.sqrt(2.0), True)
    err = (gx.to(F64) - ref).abs()
    assert (err <= TWO * ref.abs()).all(), shape
    # gbias of the kernel's OWN gx
    B, HW = shape[0], shape[2] * shape[3]
    s, a = S.channel_sum(gx)
    ratio = ((gb.to(F64) - s).abs() / (U * a).clamp_min(1e-300)).max().item()
    assert ratio <= depth_channel_sum(B, HW), (shape, ratio)
    print(f'bias_act_bwd {shape}: gx max err / (2^-24 |ref|) = {(err / (U * ref.abs()).clamp_min(1e-300)).max().item():.3f} (limit 2); '
          f'gbias err / (2^-24 sum|gx|) = {ratio:.3f} (limit {depth_channel_sum(B, HW)})')


# ----------------------------------------------------------------------------- act_bwd_fused
ACT_SHAPES = [
    pytest.param(2, 3, 4, 4, id='act-2x3x4x4-vector-one-chunk'),
    pytest.param(1, 2, 5, 7, id='act-1x2x5x7-scalar'),
    pytest.param(1, 2, 50, 82, id='act-1x2x50x82-vector-second-chunk-of-one-quad'),
    pytest.param(1, 1, 17, 241, id='act-1x1x17x241-scalar-second-chunk-of-one-element'),
    pytest.param(2, 2, 64, 128, id='act-2x2x64x128-two-full-chunks'),
]
# (rgb, g_feat, noise: 0 none / 1 shared / 2 per sample, noise_weight, bias, Cols, dscale)
ACT_OPTIONS = [
    (True, True, 2, True, True, True, True),
    (True, True, 1, False, True, False, True),
    (True, False, 0, False, False, True, True),
    (False, True, 1, True, True, False, True),
    (False, True, 0, True, False, True, False),
    (True, True, 2, True, False, False, False),
]


def depth_act(HW):
    # act_bwd_fused_kernel: `acc_r += gp * ycv` in a thread: the vector path adds 4 per trip over ceil(chunk / 1024) trips, the scalar path 1 per trip over
    # ceil(chunk / 256); block_sum_256: wave_sum 6 and `red[0] + red[1] + red[2] + red[3]` 3; reduce_parts' row_sum over the chunks (<= 64: row_sum16) 6
    n = min(HW, S.ACT_CHUNK)
    per_thread = 4 * -(-n // 1024) if HW % 4 == 0 else -(-n // 256)
    return per_thread + 6 + 3 + 6


# roundings of one term, from the lambda `one` of act_bwd_fused_kernel
ROUND_GPRE = 7          # `w0 = w_rgb[..] * rgb_scale` 1, `w0 * r0 + w1 * r1 + w2 * r2` 1 + 2, `sr * t` 1, `gf + ..` 1, `g * (o > 0.f ? ..)` 1
ROUND_YCV = 3           # `o * inv_pos` 1, `- nw * nz` 1 (the product is fused or exact), `- bv` 1
ROUND_T = 5             # w0 1, `w0 * r0 + ..` 1 + 2, `o * t` 1 (fused into the accumulation or not: the addition is in the depth)


def _act_abi(dev, d, rgb, gfeat, noise, nw, bias, cols, dscale):
    out = d['out']
    B, C = out.shape[0], out.shape[1]
    HW = out.numel() // (B * C)
    nparts = lib().oodgan_act_bwd_nparts(HW)
    assert nparts == -(-HW // S.ACT_CHUNK)
    g_pre = guarded(dev, out.numel())
    part_r, part_t, part_m = guarded(dev, B * C * nparts), guarded(dev, B * C * nparts), guarded(dev, B * C * nparts)
    if cols:
        sm, dm = block_in(dev, d['s_rgb']), block_in(dev, d['dscale'])
        sp, ss, dp, dst = P(sm, OFF), C + PAD, P(dm, OFF), C + PAD
    else:
        sm, dm = d['s_rgb'].to(dev), d['dscale'].to(dev)
        sp, ss, dp, dst = P(sm), C, P(dm), C
    nz = to(dev, d['noise']) if noise else None
    rs = S.torgb_scale(C) if d['rgb_scale'] is None else d['rgb_scale']
    # every device tensor stays referenced until the synchronize below
    gfd, od, nwd, bd = to(dev, d['g_feat']) if gfeat else None, out.to(dev), to(dev, d['nw']) if nw else None, to(dev, d['bias']) if bias else None
    grd, wrd = (to(dev, d['g_rgb']), to(dev, d['w_rgb'])) if rgb else (None, None)
    ck(lib().oodgan_act_bwd_fused_max(P(gfd), P(od), P(nz), 1 if nz is None else nz.shape[0], P(nwd), P(bd), P(grd), P(wrd), sp if rgb else None, ss if rgb else 0, rs,
                                      P(g_pre), P(part_r), P(part_t), P(part_m), dp if dscale else None, dst if dscale else 0, B, C, HW, stream()), 'act_bwd_fused_max')
    r, t = guarded(dev, B * C), guarded(dev, B * C)
    ck(lib().oodgan_reduce_parts(P(part_r), P(r), B * C, nparts, 0, stream()), 'reduce')
    if rgb:
        ck(lib().oodgan_reduce_parts(P(part_t), P(t), B * C, nparts, 0, stream()), 'reduce')
    torch.cuda.synchronize()
    for buf, n in ((g_pre, out.numel()), (part_r, B * C * nparts), (part_m, B * C * nparts), (r, B * C)):
        assert guard_ok(buf, n)
    if rgb:
        assert guard_ok(part_t, B * C * nparts)
    else:
        assert bool((host(part_t) == SENT).all()), 'part_rgb is not written without the RGB branch'
    return dict(g_pre=host(g_pre)[:out.numel()].view(out.shape), r=host(r)[:B * C].view(B, C), t=host(t)[:B * C].view(B, C) if rgb else None,
                part_max=host(part_m)[:B * C * nparts].view(B, C, nparts))


def _act_ref(d, rgb, gfeat, noise, nw, bias, dscale):
    return S.act_bwd_fused(d['out'], d['g_feat'] if gfeat else None, d['noise'] if noise else None, d['nw'] if nw else None, d['bias'] if bias else None,
                           d['g_rgb'] if rgb else None, d['w_rgb'], d['s_rgb'], d['rgb_scale'], d['dscale'] if dscale else None)


@pytest.mark.parametrize('B,C,H,W', ACT_SHAPES)
def test_act_bwd_fused_integer_data(dev, B, C, H, W):
    HW = H * W
    worst = 0.0
    for rgb, gfeat, noise, nw, bias, cols, dscale in ACT_OPTIONS:
        d = D.act_data(B, C, H, W, {0: 0, 1: 1, 2: B}[noise])
        assert (d['out'] == 0).sum() >= 2 * B * C
        tag = (B, C, H, W, rgb, gfeat, noise, nw, bias, cols, dscale)
        ref = _act_ref(d, rgb, gfeat, noise, nw, bias, dscale)
        got = _act_abi(dev, d, rgb, gfeat, noise, nw, bias, cols, dscale)
        # g is exact, g * factor one rounding of a double product that is itself exact (24 x 24 bits)
        assert torch.equal(got['g_pre'], ref['g_pre'].to(torch.float32)), tag
        if rgb:
            assert torch.equal(got['t'].to(F64), ref['t']), tag          # integers times powers of two: exact
        # r: g_pre carries 1 rounding here, y_cv ROUND_YCV, their product 1
        limit = depth_act(HW) + 1 + ROUND_YCV + 1
        ratio = ((got['r'].to(F64) - ref['r']).abs() / (U * ref['r_mag']).clamp_min(1e-300)).max().item()
        assert ratio <= limit, (tag, ratio, limit)
        worst = max(worst, ratio / limit)
        assert torch.equal(got['part_max'], S.part_max_of(got['g_pre'], d['dscale'] if dscale else None)), tag
    print(f'act_bwd_fused {B}x{C}x{H}x{W} integer data: r largest error / bound = {worst:.3f}')


@pytest.mark.parametrize('B,C,H,W', ACT_SHAPES)
def test_act_bwd_fused_random_and_wrapper(dev, B, C, H, W):
    """random-normal data with the derived bars; the dense wrapper ops.act_bwd_fused equals the C ABI bit for bit; mul2 of want_scale=True"""
    from oodgan import ops
    HW = H * W
    d = D.act_normal(B, C, H, W, B)
    for rgb in (True, False):
        ref = _act_ref(d, rgb, True, True, True, True, True)
        got = _act_abi(dev, d, rgb, True, True, True, True, True, True)
        e_g = ((got['g_pre'].to(F64) - ref['g_pre']).abs() / (U * ref['g_pre_mag']).clamp_min(1e-300)).max().item()
        assert e_g <= ROUND_GPRE, (B, C, H, W, rgb, e_g)
        lim_r = depth_act(HW) + ROUND_GPRE + ROUND_YCV + 1
        e_r = ((got['r'].to(F64) - ref['r']).abs() / (U * ref['r_mag_full'])).max().item()
        assert e_r <= lim_r, (B, C, H, W, rgb, e_r, lim_r)
        e_t = 0.0
        if rgb:
            lim_t = depth_act(HW) + ROUND_T
            e_t = ((got['t'].to(F64) - ref['t']).abs() / (U * ref['t_mag'])).max().item()
            assert e_t <= lim_t, (B, C, H, W, e_t, lim_t)
        assert torch.equal(got['part_max'], S.part_max_of(got['g_pre'], d['dscale']))
        print(f'act_bwd_fused {B}x{C}x{H}x{W} random rgb={rgb}: g_pre {e_g:.3f} (limit {ROUND_GPRE}), r {e_r:.3f} (limit {lim_r}), t {e_t:.3f} '
              f'(limit {depth_act(HW) + ROUND_T}) in units of 2^-24 sum|terms|')
        dd = {k: to(dev, v) for k, v in d.items() if isinstance(v, torch.Tensor)}
        kw = dict(g_rgb=dd['g_rgb'], w_rgb=dd['w_rgb'], s_rgb=dd['s_rgb']) if rgb else {}
        g_pre, r, t, mul2 = ops.act_bwd_fused(dd['out'], dd['g_feat'], dd['noise'], dd['nw'], dd['bias'], want_scale=True, dscale=dd['dscale'], **kw)
        assert torch.equal(host(g_pre), got['g_pre']) and torch.equal(host(r), got['r']) and (t is None) == (not rgb)
        if rgb:
            assert torch.equal(host(t), got['t'])
        e = T.range_exp(got['part_max'].max().item())
        assert host(mul2).tolist() == [2.0 ** -e, 2.0 ** e], (host(mul2).tolist(), e)
        # Cols for s_rgb and dscale through the wrapper: the same bits
        if rgb:
            g2, r2, t2 = ops.act_bwd_fused(dd['out'], dd['g_feat'], dd['noise'], dd['nw'], dd['bias'], dd['g_rgb'], dd['w_rgb'],
                                           ops.Cols(block_in(dev, d['s_rgb']), OFF, C))
            assert torch.equal(host(g2), got['g_pre']) and torch.equal(host(r2), got['r']) and torch.equal(host(t2), got['t'])


def test_act_bwd_fused_zero_takes_the_negative_branch(dev):
    """out == 0 exactly: factor 0.2 sqrt2, not sqrt2 (an `o >= 0` test would scale these entries by 5)"""
    d = D.act_data(2, 3, 4, 4, 0)
    got = _act_abi(dev, d, False, True, 0, False, False, False, False)
    k = S.ActConsts.kernel()
    zero = d['out'] == 0
    assert zero.sum() >= 12 and (d['g_feat'][zero] != 0).any()
    assert torch.equal(got['g_pre'][zero], (d['g_feat'][zero].to(F64) * k.neg).to(torch.float32))
    assert torch.equal(got['g_pre'][d['out'] > 0], (d['g_feat'][d['out'] > 0].to(F64) * k.pos).to(torch.float32))


# ----------------------------------------------------------------------------- feature_modulation
@pytest.mark.parametrize('full', [True, False], ids=['full-shape', 'Bx C x1x1'])
def test_feature_modulation(dev, full):
    from oodgan import ops
    shape = (2, 5, 10, 10)          # n = 1000
    cshape = shape if full else (2, 5, 1, 1)
    x, c0, c1 = T.ints(shape, 10300), T.ints(cshape, 10301), T.ints(cshape, 10302)
    for mode in ('SFT', 'ADD'):
        ref, _ = S.feature_modulation(x, c0, c1, mode)
        got = ops.feature_modulation(x.to(dev), [None if mode == 'ADD' else c0.to(dev), c1.to(dev)], mod_type=mode)
        assert torch.equal(host(got).to(F64), ref), mode
    xn, c0n, c1n = T.normal(shape, 10310), 3.0 * T.normal(cshape, 10311), T.normal(cshape, 10312)
    c0n.view(-1)[:4] = torch.tensor([0.0, -20.0, 20.0, -87.0])          # sigmoid = 1/2, ~0, ~1, and expf near its largest finite value
    ref, mag = S.feature_modulation(xn, c0n, c1n, 'FUSE')
    got = ops.feature_modulation(xn.to(dev), [c0n.to(dev), c1n.to(dev)], mod_type='FUSE')
    rel = ((host(got).to(F64) - ref).abs() / mag).max().item()
    print(f'feature_modulation FUSE ({"full" if full else "broadcast"}): max err / (|x| + |c1| sigmoid) = {rel / U:.3f} * 2^-24 (bar {FUSE_BAR / U:.2f} * 2^-24)')
    assert rel <= FUSE_BAR
