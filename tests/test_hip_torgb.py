"""The five entry points of csrc/torgb.hip — torgb_fwd_kernel (vector and scalar path), torgb_fwd_small_kernel, torgb_fwd_sform_kernel and
rgb_finish_kernel (one part or several) — against the float64 references of tests/stream_ref.py, at the smallest shapes that reach each branch.

Data: integers in [-4, 4], powers of two for s and ys_scale, integer bias and skip; the FIR kernel is make_kernel([1,3,3,1]) * 4 (dyadic) and an
asymmetric integer 4x4 kernel, which tells a transposed or unflipped tap apart.  For Ci in {16, 64, 256, 1024} 1/sqrt(Ci) is a power of two, every
product and sum is exact in any order (tests/test_stream_ref_cpu.py) and the comparison is torch.equal.  For the other Ci the bar is
(roundings on the longest path) * 2^-24 * sum |terms| per element, the count taken from the kernel's code (roundings_* below).  Every output buffer
carries guard elements behind its end; s is passed dense and as a column block of a wider matrix, and the two must agree bit for bit.
Observed maxima on the MI355X are recorded in LABNOTES.md."""
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
S_PAD, S_OFF = 7, 3          # s and ys_scale as column blocks: row stride Ci + 7, offset 3
EXACT_CI = (16, 64, 256, 1024)


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
    """flat device buffer of n + GUARD elements, all ``fill``"""
    return torch.full((n + GUARD,), fill, dtype=torch.float32, device=dev)


def guard_ok(buf, n, fill=SENT):
    return bool((host(buf)[n:] == fill).all())


def block_in(dev, dense, fill=99.0):
    m = torch.full((dense.shape[0], dense.shape[1] + S_PAD), fill, dtype=torch.float32)
    m[:, S_OFF:S_OFF + dense.shape[1]] = dense
    return m.to(dev)


def last_error():
    m = lib().oodgan_last_error()
    return m.decode() if m else ''


# ----------------------------------------------------------------------------- rounding counts (non power-of-two 1/sqrt(Ci))
def roundings_big(Ci):
    # torgb_fwd_kernel / torgb_fwd_sform_kernel, the path of one conv term: `ws[e] = scale * w[..] * s[..]` 2, `a0[0] += w0 * v.x` its product 1 and
    # the Ci additions of the thread's chain, `o0 = a0[j] + b0` 1, SkipTaps::add `o0 += w[k] * v[k][0]` 4 additions
    return 2 + 1 + Ci + 1 + 4


def roundings_small(Ci):
    # torgb_fwd_small_kernel: `sv = scale * s[..]` 1, `w0 = sv * w[ci]` 1, `a0[0] += w0 * v.x` its product 1 and ceil(Ci / 64) additions in the lane,
    # wave_sum's six `v += __shfl_xor`, `o0 += bias` 1, SkipTaps::add 4 additions
    return 2 + 1 + -(-Ci // 64) + 6 + 1 + 4


def roundings_finish(nparts):
    # rgb_finish_kernel: `o0 += pq[0]` nparts - 1, `o0 += bias[0]` 1, SkipTaps::add 4 additions (a skip term: its product 1 + 4)
    return max(nparts - 1 + 1 + 4, 1 + 4)


def check_y(y, ref, mag, Ci, count, tag):
    """exact for the power-of-two scales, the derived bar otherwise; returns error / (2^-24 mag)"""
    if Ci in EXACT_CI:
        assert torch.equal(y.to(F64), ref), tag
        return 0.0
    err = (y.to(F64) - ref).abs()
    ratio = (err / (U * mag).clamp_min(1e-300)).max().item()
    assert (err <= count * U * mag).all(), (tag, ratio, count)
    return ratio


# ----------------------------------------------------------------------------- torgb_fwd
SMALL = [  # HW <= 4096 and HW % 4 == 0: torgb_fwd_small_kernel
    pytest.param(2, 16, 2, 2, id='small-2x16x2x2-one-quad-idle-lanes-1x1-skip-all-taps-clamped'),
    pytest.param(1, 80, 6, 6, id='small-1x80x6x6-last-block-one-live-wave-quads-straddle-rows'),
    pytest.param(2, 320, 4, 8, id='small-2x320x4x8-five-channel-trips-past-the-unroll'),
    pytest.param(1, 64, 64, 64, id='small-1x64x64x64-boundary-HW-4096'),
    pytest.param(1, 1024, 2, 2, id='small-1x1024x2x2-kMaxCi'),
]
BIG_VEC = [  # HW > 4096, HW % 4 == 0: torgb_fwd_kernel, float4 loads
    pytest.param(1, 16, 66, 64, id='bigvec-1x16x66x64-last-block-partly-filled'),
    pytest.param(2, 24, 70, 62, id='bigvec-2x24x70x62-rows-straddle-unroll-remainder'),
]
BIG_SCALAR = [  # HW % 4 != 0: torgb_fwd_kernel, scalar loads; an odd side admits no skip
    pytest.param(2, 5, 5, 7, id='bigscalar-2x5x5x7'),
    pytest.param(1, 3, 65, 65, id='bigscalar-1x3x65x65-last-thread-owns-one-pixel'),
]


def _torgb_call(dev, d, k4, use_bias, use_skip, cols, scale=None):
    B, Ci, H, W = d['x'].shape
    n = B * 3 * H * W
    y = guarded(dev, n)
    xd, wd = d['x'].to(dev), d['w'].to(dev)
    if cols:
        sm = block_in(dev, d['s'])
        sp, stride = P(sm, S_OFF), Ci + S_PAD
    else:
        sm = d['s'].to(dev)
        sp, stride = P(sm), Ci
    bd = d['bias'].to(dev) if use_bias else None
    kd = k4.to(dev) if use_skip else None
    sk = d['skip'].to(dev) if use_skip else None
    rc = lib().oodgan_torgb_fwd(P(xd), P(wd), sp, stride, P(bd), P(sk), P(kd), P(y), B, Ci, H, W, S.torgb_scale(Ci) if scale is None else scale, stream())
    torch.cuda.synchronize()
    return rc, y, n


def _torgb_case(dev, B, Ci, H, W, small, allow_skip=True):
    from oodgan import ops
    d = D.torgb_data(B, Ci, H, W)
    count = roundings_small(Ci) if small else roundings_big(Ci)
    worst = 0.0
    options = [(True, 'dyadic'), (True, 'asym'), (False, None)] if allow_skip else [(False, None)]
    for use_skip, kn in options:
        k4 = D.fir(kn) if use_skip else None
        for use_bias in (True, False):
            ref, mag = S.torgb(d['x'], d['w'], d['s'], d['bias'] if use_bias else None, d['skip'] if use_skip else None, k4)
            outs = []
            for cols in (False, True):
                rc, y, n = _torgb_call(dev, d, k4, use_bias, use_skip, cols)
                tag = (B, Ci, H, W, kn, use_bias, cols)
                assert rc == 0, (tag, last_error())
                assert guard_ok(y, n), tag
                yh = host(y)[:n].view(B, 3, H, W)
                worst = max(worst, check_y(yh, ref, mag, Ci, count, tag))
                outs.append(yh)
            assert torch.equal(outs[0], outs[1]), ('dense != Cols', B, Ci, H, W, kn, use_bias)
            # the wrapper, with s as ops.Cols(base, off, Ci)
            yw = ops.torgb(d['x'].to(dev), d['w'].to(dev), ops.Cols(block_in(dev, d['s']), S_OFF, Ci), d['bias'].to(dev) if use_bias else None,
                           d['skip'].to(dev) if use_skip else None, None if k4 is None else k4.to(dev))
            assert torch.equal(host(yw), outs[0]), ('ops.torgb != C ABI', B, Ci, H, W, kn, use_bias)
    print(f'torgb {B}x{Ci}x{H}x{W}: max err / (2^-24 sum|terms|) = {worst:.3f} (limit {count if Ci not in EXACT_CI else 0})')


@pytest.mark.parametrize('B,Ci,H,W', SMALL)
def test_torgb_small_kernel(dev, B, Ci, H, W):
    assert H * W <= 4096 and (H * W) % 4 == 0
    _torgb_case(dev, B, Ci, H, W, small=True)


@pytest.mark.parametrize('B,Ci,H,W', BIG_VEC)
def test_torgb_big_kernel_vector_path(dev, B, Ci, H, W):
    assert H * W > 4096 and (H * W) % 4 == 0
    _torgb_case(dev, B, Ci, H, W, small=False)


@pytest.mark.parametrize('B,Ci,H,W', BIG_SCALAR)
def test_torgb_big_kernel_scalar_path(dev, B, Ci, H, W):
    assert (H * W) % 4 != 0
    _torgb_case(dev, B, Ci, H, W, small=False, allow_skip=False)


def test_torgb_refusals(dev):
    """each returns OODGAN_E_ARG (-1) with a message and launches nothing: the output keeps its sentinel"""
    k4 = D.fir('dyadic')
    d = D.torgb_data(1, 1025, 2, 2)
    rc, y, n = _torgb_call(dev, d, k4, True, False, False)
    assert rc == -1 and 'Ci' in last_error() and bool((host(y) == SENT).all())
    for H, W in ((5, 6), (6, 5)):
        d = D.torgb_data(1, 16, H, W)
        rc, y, n = _torgb_call(dev, d, k4, True, True, False)
        assert rc == -1 and 'even' in last_error() and bool((host(y) == SENT).all()), (H, W)
        pbuf = guarded(dev, 2 * 3 * H * W, 1.0)
        sk, kd = d['skip'].to(dev), k4.to(dev)
        for fn, args in ((lib().oodgan_rgb_finish, ()), (lib().oodgan_rgb_finish_parts, (2,))):
            rc = fn(P(pbuf), *args, None, P(sk), P(kd), P(pbuf), 1, H, W, stream())
            torch.cuda.synchronize()
            assert rc == -1 and 'even' in last_error() and bool((host(pbuf) == 1.0).all()), (H, W)
    from oodgan import ops
    for Ci, H, W in ((24, 4, 8), (16, 4, 6)):
        d = D.torgb_data(1, Ci, H, W)
        y = guarded(dev, 3 * H * W)
        ys = ops.SForm(1, 32, H, 8, dev)
        xd, wd, sd = d['x'].to(dev), d['w'].to(dev), d['s'].to(dev)
        rc = lib().oodgan_torgb_fwd_sform(P(xd), P(wd), P(sd), Ci, None, None, None, P(y), ctypes.c_void_p(ys.data_ptr()), None, 0,
                                          1, Ci, H, W, S.torgb_scale(Ci), None, stream())
        torch.cuda.synchronize()
        assert rc == -1 and 'torgb_fwd_sform' in last_error() and bool((host(y) == SENT).all()), (Ci, W)
        assert int(host(ys.data).abs().max()) == 0


# ----------------------------------------------------------------------------- torgb_fwd_sform
SFORM = [
    pytest.param(1, 16, 10, 20, id='sform-1x16x10x20-full-wave-and-partial-wave-one-channel-block-no-prefetch'),
    pytest.param(1, 48, 16, 40, id='sform-1x48x16x40-two-blocks-second-one-full-wave-three-exited'),
]


@pytest.mark.parametrize('B,Ci,H,W', SFORM)
def test_torgb_sform(dev, B, Ci, H, W):
    from oodgan import ops
    HW = H * W
    d = D.torgb_data(B, Ci, H, W)
    # a thread owns 2 pixels, a wave 128, a block 512.  10x20: wave 0 is full (record_vmax), wave 1 holds 36 live lanes (the atomicMax per lane);
    # 16x40: every live wave is full, the last one alone in the second block
    plants = {200: (5, 129), 640: (5, 517)}[HW]
    assert (HW % 128 != 0) == (HW == 200) and (HW - 1) // 128 * 128 <= plants[1] < HW
    worst = 0.0
    for plant in plants:          # the sample's maximum on either route
        x = d['x'].clone()
        x.view(B, Ci, HW)[0, Ci - 1, plant] = -8.0
        ysc = d['ys_scale'].clone()
        ysc[0, Ci - 1] = 4.0
        for use_ysc in (False, True):
            want_ys = x.to(F64) * (ysc.to(F64)[:, :, None, None] if use_ysc else 1.0)
            assert torch.equal(want_ys.to(torch.float16).to(F64), want_ys)
            for use_skip, kn, use_bias in ((True, 'asym', True), (True, 'dyadic', False), (False, None, True)):
                k4 = D.fir(kn) if use_skip else None
                ref, mag = S.torgb(x, d['w'], d['s'], d['bias'] if use_bias else None, d['skip'] if use_skip else None, k4)
                outs = []
                for cols in (False, True):
                    y = guarded(dev, B * 3 * HW)
                    ys = ops.SForm(B, Ci, H, W, dev)
                    vm = torch.zeros(B * 64, dtype=torch.int32, device=dev)
                    sm = block_in(dev, d['s']) if cols else d['s'].to(dev)
                    # ys_scale: None, or a Cols block (the engine's form); with dense s a dense ys_scale too
                    ym = None if not use_ysc else (block_in(dev, ysc) if cols else ysc.to(dev))
                    # every device tensor stays referenced until the synchronize below
                    xd, wd, bd = x.to(dev), d['w'].to(dev), d['bias'].to(dev) if use_bias else None
                    sk, kd = (d['skip'].to(dev), k4.to(dev)) if use_skip else (None, None)
                    rc = lib().oodgan_torgb_fwd_sform(
                        P(xd), P(wd), P(sm, S_OFF if cols else 0), Ci + (S_PAD if cols else 0), P(bd), P(sk), P(kd), P(y), ctypes.c_void_p(ys.data_ptr()),
                        None if ym is None else P(ym, S_OFF if cols else 0), 0 if ym is None else Ci + (S_PAD if cols else 0), B, Ci, H, W, S.torgb_scale(Ci),
                        ctypes.c_void_p(vm.data_ptr()), stream())
                    tag = (B, Ci, H, W, plant, use_ysc, kn, use_bias, cols)
                    assert rc == 0, (tag, last_error())
                    torch.cuda.synchronize()
                    assert guard_ok(y, B * 3 * HW), tag
                    yh = host(y)[:B * 3 * HW].view(B, 3, H, W)
                    worst = max(worst, check_y(yh, ref, mag, Ci, roundings_big(Ci), tag))
                    outs.append(yh)
                    # ys through the project's own S-form reader: hi + lo == x * ys_scale
                    got = host(ops.SFormSaved(ys, None).to_nchw())
                    assert torch.equal(got.to(F64), want_ys), tag
                    vmax = host(vm).view(torch.float32).view(B, 64).amax(1)
                    assert torch.equal(vmax.to(F64), want_ys.abs().amax((1, 2, 3))), (tag, vmax)
                    assert vmax[0].item() == (32.0 if use_ysc else 8.0)
                assert torch.equal(outs[0], outs[1]), ('dense != Cols', B, Ci, H, W)
    print(f'torgb_sform {B}x{Ci}x{H}x{W}: max err / (2^-24 sum|terms|) = {worst:.3f} (limit {roundings_big(Ci) if Ci not in EXACT_CI else 0})')


# ----------------------------------------------------------------------------- rgb_finish / rgb_finish_parts
FINISH = [
    pytest.param(2, 6, 10, True, id='finish-2x6x10-skip'),
    pytest.param(1, 5, 7, False, id='finish-1x5x7-no-skip'),
    pytest.param(1, 726, 724, True, id='finish-1x726x724-second-grid-stride-trip'),
]


def _finish_call(dev, parts, bias, skip, k4, single_entry):
    nparts, B, _, H, W = parts.shape
    n = parts.numel()
    buf = guarded(dev, n)
    buf[:n] = parts.reshape(-1).to(dev)
    bd, sk, kd = (None if t is None else t.to(dev) for t in (bias, skip, k4))
    if single_entry:
        rc = lib().oodgan_rgb_finish(P(buf), P(bd), P(sk), P(kd), P(buf), B, H, W, stream())
    else:
        rc = lib().oodgan_rgb_finish_parts(P(buf), nparts, P(bd), P(sk), P(kd), P(buf), B, H, W, stream())
    torch.cuda.synchronize()
    assert rc == 0, last_error()
    assert guard_ok(buf, n)
    got = host(buf)[:n].view(nparts, B, 3, H, W)
    assert torch.equal(got[1:], parts[1:]), 'parts beyond the first are inputs only'
    return got[0]


@pytest.mark.parametrize('nparts', [1, 2, 5])
@pytest.mark.parametrize('B,H,W,has_skip', FINISH)
def test_rgb_finish(dev, B, H, W, has_skip, nparts):
    assert (B * H * W > 2048 * 256) == (H == 726)          # stream_grid caps the grid at 2048 blocks of 256
    parts = D.rgb_parts(nparts, B, H, W)
    d = D.torgb_data(B, 16, H, W, seed=1)
    for kn in (('asym', 'dyadic') if has_skip else (None,)):
        k4 = None if kn is None else D.fir(kn)
        skip = d['skip'] if has_skip else None
        for bias in (d['bias'], None):
            ref, _ = S.rgb_finish(parts, bias, skip, k4)
            got = _finish_call(dev, parts, bias, skip, k4, False)
            assert torch.equal(got.to(F64), ref), (nparts, B, H, W, kn, bias is None)
            if nparts == 1:
                got1 = _finish_call(dev, parts, bias, skip, k4, True)
                assert torch.equal(got1, got), 'rgb_finish != rgb_finish_parts(1)'
        if H == 726:
            break          # one kernel at the large shape


@pytest.mark.parametrize('nparts', [1, 2, 5])
def test_rgb_finish_wrapper_and_random(dev, nparts):
    """ops.rgb_finish in place on a (nparts,B,3,H,W) / (B,3,H,W) tensor; one random-normal set with the bar roundings_finish * 2^-24 * sum |terms|"""
    from oodgan import ops
    B, H, W = 2, 6, 10
    parts = T.normal((nparts, B, 3, H, W), 9650 + nparts)
    d = D.torgb_normal(B, 16, H, W, seed=2)
    k4 = T.normal((4, 4), 9660)
    ref, mag = S.rgb_finish(parts, d['bias'], d['skip'], k4)
    got = _finish_call(dev, parts, d['bias'], d['skip'], k4, False)
    err = (got.to(F64) - ref).abs()
    ratio = (err / (U * mag)).max().item()
    print(f'rgb_finish random nparts={nparts}: max err / (2^-24 sum|terms|) = {ratio:.3f} (limit {roundings_finish(nparts)})')
    assert ratio <= roundings_finish(nparts)
    pd = parts.to(dev) if nparts > 1 else parts[0].to(dev)
    out = ops.rgb_finish(pd, d['bias'].to(dev), d['skip'].to(dev), k4.to(dev))
    assert out.data_ptr() == pd.data_ptr() and torch.equal(host(out), got)
