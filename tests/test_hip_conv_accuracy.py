"""Every route of the split-f16 3x3 conv (oodgan_conv3x3_f16s, oodgan_upconv_vblur_fform) and the exact-fp32 conv (oodgan_conv3x3) held to
fp32-class accuracy against a float64 reference of the operation (tests/splitf16_ref.py), and the operand producers (S-form, phase-split
S-form, packed split-f16 weights, the `ys` S-form a conv writes for its consumer) held to the invariants of their formats.

The bar of every case is 4 x yardstick, the yardstick = e_model + e32 computed in the test from the reference alone (e_model: the
three-term formula hi*hi + hi*lo + lo*hi evaluated exactly on the split operands, e32: the same formula in float32 on the CPU); one
factor 2 for packed f16 conversions that differ from round-to-nearest on ties, one for another fp32 summation order than the CPU's.
tests/test_splitf16_ref_cpu.py proves that three subtly wrong kernels (a lo term lost for one tap, for the last 16-channel chunk, for
the last 8 output channels) err by at least 10 bars in every case.  Two metrics, e_max = max|d| / max|ref| and e_rms = rms(d) /
rms(ref), on y and on the dot epilogue; every case asserts its dispatch counter, so the kernel named is the kernel that ran.

Calls per case (where the route has them): 'fwd' out_scale + per-sample noise + bias + leaky-ReLU ('fwd_prelu' for the stride-2
routes: out_scale + bias + PReLU, the encoder's use; the transposed routes only have out_scale), 'plain' out_scale only, 'dx' the
input-gradient instance (transposed / flipped packing, dotx, nothing else), 'dx12' the same with data of scale 2^-12 and the in_mul2 pair
of the range control.

Not here: the fused epilogues (`fuse`, `dot_actgrad`, fused ToRGB, x_fform = 2), the two-instruction and hi-only instances and the grouped
stride-2 kernel — existing tests pin each of them to the plain routes at 1e-6 to 2e-5 (test_hip_stripx.py, test_hip_grad2.py,
test_hip_bwd_producers.py, test_hip_ops.py, test_hip_tiny.py), so they inherit this root.

Measured on an MI355X (largest error / yardstick over the calls of a case, per metric; the bar is 4):

| case (route-K-M) | precision | largest e_max | / yardstick | largest e_rms | / yardstick | smallest sabotage (e_max) |
|---|---|---|---|---|---|---|
| s1pp-24-40 | f16s | 4.21e-07 | 1.01 | 2.21e-07 | 0.67 | 7.57e-05 |
| s1pp-512-64 | f16s | 1.24e-06 | 4.00 | 7.30e-07 | 2.46 | 5.14e-05 |
| t2gen-24-40 | f16s | 1.97e-07 | 0.70 | 1.27e-07 | 0.59 | 1.30e-04 |
| t2gen-512-64 | f16s | 8.07e-07 | 2.92 | 4.05e-07 | 1.57 | 5.77e-05 |
| s2gen-24-40 | f16s | 4.52e-07 | 0.94 | 1.84e-07 | 0.65 | 6.38e-05 |
| s2gen-512-64 | f16s | 1.21e-06 | 3.44 | 8.12e-07 | 2.64 | 4.29e-05 |
| s1v2-24-40 | f16s | 3.17e-07 | 0.87 | 1.87e-07 | 0.69 | 7.07e-05 |
| s1v2-40-24 | f16s | 3.21e-07 | 0.92 | 2.40e-07 | 0.87 | 7.30e-05 |
| t2v2-24-40 | f16s | 1.73e-07 | 0.55 | 1.31e-07 | 0.60 | 1.08e-04 |
| s2v2-40-24 | f16s | 4.49e-07 | 1.18 | 2.52e-07 | 0.83 | 5.79e-05 |
| strip-24-20 | f16s | 1.99e-07 | 0.49 | 1.52e-07 | 0.46 | 6.96e-05 |
| strip-32-32 | f16s | 2.49e-07 | 0.60 | 1.94e-07 | 0.47 | 6.71e-05 |
| s1big-80-96 | f16s | 5.99e-07 | 1.34 | 3.10e-07 | 1.10 | 6.12e-05 |
| t2big-48-80 | f16s | 2.55e-07 | 0.91 | 1.58e-07 | 0.70 | 1.41e-04 |
| s2big-48-80 (input gradient) | f16s | 3.71e-07 | 0.84 | 2.43e-07 | 0.80 | 5.74e-05 |
| s2big-48-80-fwd (pad_tl, bias, PReLU) | f16s | 3.77e-07 | 1.12 | 2.21e-07 | 0.83 | 8.60e-05 |
| tiny-s1-512-64 | f16s | 1.71e-07 | 0.51 | 1.51e-07 | 0.48 | 5.06e-05 |
| tiny-s1-64-64 | f16s | 1.46e-07 | 0.47 | 1.29e-07 | 0.42 | 6.54e-05 |
| tiny-s2-512-64 | f16s | 3.29e-07 | 1.01 | 1.63e-07 | 0.53 | 3.31e-05 |
| tiny-s2-64-64 | f16s | 1.52e-07 | 0.44 | 1.42e-07 | 0.45 | 6.61e-05 |
| stripx-32-32 | f16s | 1.90e-07 | 0.42 | 1.36e-07 | 0.45 | 7.72e-05 |
| upvb-48-32 | f16s | 3.70e-07 | 1.08 | 1.92e-07 | 0.74 | 6.18e-05 |
| s1pp-24-40 | f32 | 5.33e-07 | 1.24 | 2.90e-07 | 0.93 | 7.57e-05 |
| s1pp-512-64 | f32 | 1.71e-06 | 5.11 | 1.12e-06 | 3.88 | 5.14e-05 |
| t2gen-24-40 | f32 | 2.70e-07 | 0.95 | 1.44e-07 | 0.67 | 1.30e-04 |
| t2gen-512-64 | f32 | 1.49e-06 | 5.39 | 6.44e-07 | 2.50 | 5.77e-05 |
| s2gen-24-40 | f32 | 5.77e-07 | 1.45 | 2.64e-07 | 0.93 | 6.38e-05 |
| s2gen-512-64 | f32 | 1.71e-06 | 5.31 | 1.17e-06 | 3.56 | 4.29e-05 |

The four K = 512 rows above 4 (s1pp f16s: 4.002, in its 'fwd' call; the three exact-fp32 rows) are correct kernels with ONE fp32 accumulator per output over the whole contraction (splitf16_ref.MEASURED_ABOVE
gives the argument and their bars: 2 x the measured e_max, still under 1/10 of the smallest sabotage).  The first run of this module found one
bug: the tile kernel (s1v2 / s2v2) wrote `ys` from fma(v, out_scale, round(noise_w * noise)) + bias while the y it returned was
fma(noise_w, noise, round(v * out_scale)) + bias — 257 of 23040 records off by up to 2.2e-3 relative where the terms cancel; csrc/conv_f16s_v2.hip
now has one rounding order for all its epilogue paths.
"""
import math

import pytest
import torch

import splitf16_ref as R

pytestmark = pytest.mark.gpu

ROUTES = ('stripx', 'strip', 's1big', 's1v2', 's1pp', 'tiny', 't2big', 't2v2', 't2gen', 's2big', 's2v2', 's2gen', 'upvb')


@pytest.fixture(scope='module')
def dev():
    return torch.device('cuda:0')


def _counts(_lib):
    return {r: _lib.dispatch_count(r) for r in ROUTES if _lib.dispatch_count(r)}


def _to_fform(x):
    B, C, H, W = x.shape
    return x.view(B, C // 16, 16, H, W).permute(0, 1, 3, 4, 2).contiguous().view(B, C, H, W)


def _run(c, call, o, prec, dev):
    """One call on the GPU: (y, dot) as float64 CPU tensors, the dispatch counters it ticked."""
    from oodgan import _lib, ops
    t = lambda v: None if v is None else v.to(dev)
    mul2 = None if o['mul2'] is None else torch.tensor(o['mul2'], dtype=torch.float32, device=dev)
    x, s = t(o['x']), t(o['s'])
    if c.mode == R.UPVB:        # inputs, packing and buffers as tests/test_hip_stripx.py builds them
        assert ops.upconv_vblur_supported(c.B, c.K, c.M, c.H, c.W) and not ops.upconv_vblur_supported(c.B, c.K, c.M, c.H - 1, c.W) \
            and not ops.upconv_vblur_supported(c.B, c.K, c.M, c.H, c.W - 1)
        xs = ops.to_sform(x, s)
        wvb = ops.pack_upconv_vblur(t(o['w']), o['wscale'], t(o['k']))
        assert wvb is not None
        _lib.dispatch_reset()
        y = ops.upconv_vblur_fform(xs, wvb, out_scale=t(o['d']), bias=t(o['bias']), noise=t(o['noise']), noise_weight=t(o['nw']), act=o['act'] == 'lrelu')
        return y.to_nchw().double().cpu(), None, _counts(_lib)
    kw = dict(out_scale=t(o['d']), bias=t(o['bias']), noise=t(o['noise']), noise_weight=t(o['nw']), slope=t(o['slope']), dotx=t(o['dotx']), in_mul2=mul2,
              act={'none': ops.ACT_NONE, 'lrelu': ops.ACT_LRELU, 'prelu': ops.ACT_PRELU}[o['act']])
    w = t(o['w'])
    if o['dotx'] is not None:   # the input-gradient packings: k = the forward conv's output channel (transpose), the adjoint's taps (flip, stride 1)
        flip = c.mode == R.S1
        wsrc = w.transpose(0, 1).flip([2, 3]) if flip else w.transpose(0, 1)
        wpk = ops.pack_conv3x3(wsrc.contiguous(), transpose=True, flip=flip, precision=prec)
    else:
        wpk = ops.pack_conv3x3(w, precision=prec)
    if c.src == 'nchw':
        xin, kw['in_scale'] = x, s
    elif c.src == 'sform':
        xin = ops.to_sform(x, s, mul2)
    elif c.src == 'phases':
        xin = ops.to_sform_phases(x, c.H, c.W, s, mul2)
    elif c.src == 'padtl':
        xin = ops.to_sform_phases(t(o['x_unpadded']), c.H, c.W, s, mul2, pad_tl=True)
    else:
        assert c.src == 'fform' and ops.xf_supported(c.B, c.K, c.M, c.H, c.W)
        xin, kw['in_scale'] = ops.FForm(_to_fform(x)), s
    _lib.dispatch_reset()
    out = ops.conv3x3(xin, wpk, c.M, c.mode, **kw)
    counts = _counts(_lib)
    y, dot = out if o['dotx'] is not None else (out, None)
    if isinstance(y, ops.FForm):
        y = y.to_nchw()
    ho, wo = R.out_hw(c)
    y = y[..., :wo]             # the transposed conv writes pitched rows
    assert y.shape == (c.B, c.M, ho, wo)
    return y.double().cpu(), None if dot is None else dot.double().cpu(), counts


def _check(c, prec, dev, tunable):
    for name, value in c.tun.items():
        tunable(name, value)
    worst = {}
    failures = []
    for call in c.calls:
        o, ref, Y, sab = R.analysis(c.id, call)
        y, dot, counts = _run(c, call, o, prec, dev)
        assert counts == ({c.route: 1} if prec == 'f16s' else {}), (call, counts)      # the kernel named is the kernel that ran
        assert torch.isfinite(y).all()
        e = R.errors(y, dot, ref[0], ref[1])
        for key in sorted(Y):
            smallest = min(s_[key] for s_ in sab.values())
            print(f'{c.id:16s} {prec:4s} {call:9s} {key[0]:3s} e_{key[1]}: {e[key]:.2e}  yardstick {Y[key]:.2e}  ratio {e[key] / Y[key]:.2f}  '
                  f'smallest sabotage {smallest:.2e}')
            worst[key[1]] = max(worst.get(key[1], 0.0), e[key] / Y[key])
            b = R.bar(c.id, prec, call, key, Y)
            assert b <= smallest / 10.0, (call, key, b, smallest)       # the cap: no bar above 1/10 of the smallest sabotage
            if not e[key] <= b:
                failures.append((call, key, e[key], Y[key], b))
    print(f'{c.id:16s} {prec:4s} worst e_max / yardstick {worst["max"]:.2f}   worst e_rms / yardstick {worst["rms"]:.2f}')
    assert not failures, failures


@pytest.mark.parametrize('cid', R.CASE_IDS)
def test_split_f16_route_against_float64(cid, dev, tunable):
    _check(R.CASES[R.CASE_IDS.index(cid)], 'f16s', dev, tunable)


@pytest.mark.parametrize('cid', [c.id for c in R.CASES if c.src == 'nchw'])
def test_exact_fp32_conv_against_float64(cid, dev, tunable):
    """csrc/conv_mfma.hip (precision 'f32') on the fp32 NCHW cases: same reference, same bar (its own error is e32's: fp32 accumulation)."""
    _check(R.CASES[R.CASE_IDS.index(cid)], 'f32', dev, tunable)


# ------------------------------------------------------------------------------------------------ operand producers
def _special_values(x):
    """Plant, in every channel (both lanes of every packed pair): exact f16 ties (1 + 2^-11) * 2^j and (1 + 3 * 2^-11) * 2^j of both signs, and a
    row of values around 2^-6 whose lo halves are f16 subnormals (|lo| <= 2^-17 < 2^-14)."""
    j = torch.arange(-7, 6, dtype=torch.float32)
    n = j.numel()
    x[:, :, 0, :n] = (1 + 2.0 ** -11) * 2.0 ** j
    x[:, :, 1, :n] = -(1 + 3 * 2.0 ** -11) * 2.0 ** j
    x[:, 1::2, 2, :n] = (1 + 2.0 ** -11) * 2.0 ** j        # a tie in one lane of the pair only
    x[:, 0::2, 3, :n] = (1 + 3 * 2.0 ** -11) * 2.0 ** j
    x[:, :, 4, :] = x[:, :, 4, :].sign() * (2.0 ** -6 + x[:, :, 4, :].abs() * 2.0 ** -16)
    return x


def _candidates(x, s, shift, mul):
    """The fp32 value the producers are documented to store, (x * scale + shift) * mul2[1]: with the multiply-add rounded twice and fused."""
    xs = x if s is None else x * s[:, :, None, None]
    if shift is None:
        return [xs * mul]
    fused = ((x.double() * s.double()[:, :, None, None]) + shift.double()[:, :, None, None]).float()
    return [(xs + shift[:, :, None, None]) * mul, fused * mul]


def _assert_split(hi, lo, cands, what):
    """|v - hi| <= 2^-10 |v| and |v - (hi + lo)| <= max(2^-21 |v|, 2^-25) (half the smallest f16 subnormal; the same floor for hi, whose f16
    is subnormal below 2^-14) for one of the candidate fp32 values v."""
    ok = torch.zeros_like(hi, dtype=torch.bool)
    for v in cands:
        v = v.double()
        ok |= ((v - hi).abs() <= torch.clamp(2.0 ** -10 * v.abs(), min=2.0 ** -25)) & ((v - (hi + lo)).abs() <= torch.clamp(2.0 ** -21 * v.abs(), min=2.0 ** -25))
    bad = int((~ok).sum())
    v = cands[0].double()
    assert bad == 0, (what, bad, float(((v - (hi + lo)).abs() / v.abs().clamp_min(2.0 ** -14)).max()))


@pytest.mark.parametrize('variant', ['bare', 'pow2', 'scale', 'shift_mul2'])
@pytest.mark.parametrize('C', [24, 40])
def test_to_sform_records(C, variant, dev):
    """oodgan_to_sform: 'bare' no scale (the planted ties reach the conversion as they are), 'pow2' power-of-two scales and mul2 (still ties),
    'scale' a style, 'shift_mul2' style, shift and range scale."""
    from oodgan import ops
    B, H, W = 2, 9, 37
    x = _special_values(R.synth.normal('prod.x', (B, C, H, W), 1))
    s = shift = mul2 = None
    if variant == 'pow2':
        s, mul2 = 2.0 ** (torch.arange(B * C, dtype=torch.float32).view(B, C) % 5 - 2), (2.0 ** -3, 2.0 ** 3)
    elif variant != 'bare':
        s = R.synth.normal('prod.s', (B, C), 2, 0.3, 1.0)
    if variant == 'shift_mul2':
        shift, mul2 = R.synth.normal('prod.sh', (B, C), 3, 0.5), (2.0 ** -5, 2.0 ** 5)
    t = lambda v: None if v is None else v.to(dev)
    xs = ops.to_sform(x.to(dev), t(s), None if mul2 is None else torch.tensor(mul2, device=dev), shift=t(shift))
    hi, lo, rest = R.decode_sform(xs.data, B, C, H, W)
    assert not rest.any() and not hi[:, C:].any() and not lo[:, C:].any()       # border, tile padding, padded channels
    cands = _candidates(x, s, shift, 1.0 if mul2 is None else mul2[1])
    _assert_split(hi[:, :C], lo[:, :C], cands, variant)
    if variant == 'bare':               # lo really is subnormal in the planted row, and still carries the remainder
        assert bool((lo[:, :C, 4].abs() < 2.0 ** -14).all()) and bool((lo[:, :C, 4] != 0).any())


@pytest.mark.parametrize('pad_tl', [False, True])
@pytest.mark.parametrize('C', [24, 40])
def test_to_sform_phases_records(C, pad_tl, dev):
    """oodgan_to_sform_phases / _padtl for the stride-2 conv with output 9 x 37: with a power-of-two scale (ties stay ties), then style x mul2."""
    from oodgan import ops
    import torch.nn.functional as F
    B, H, W = 2, 9, 37
    hin, win = (2 * H, 2 * W) if pad_tl else (2 * H + 1, 2 * W + 1)
    x = _special_values(R.synth.normal('prod.px', (B, C, hin, win), 4))
    for s, mul2 in ((2.0 ** (torch.arange(B * C, dtype=torch.float32).view(B, C) % 5 - 2), None),
                    (R.synth.normal('prod.ps', (B, C), 5, 0.3, 1.0), (2.0 ** -4, 2.0 ** 4))):
        gp = ops.to_sform_phases(x.to(dev), H, W, s.to(dev), None if mul2 is None else torch.tensor(mul2, device=dev), pad_tl=pad_tl)
        hi, lo, rest = R.decode_sform_phases(gp.data, B, C, H, W)
        assert not rest.any() and not hi[:, C:].any() and not lo[:, C:].any()
        v = _candidates(x, s, None, 1.0 if mul2 is None else mul2[1])[0]
        if pad_tl:                      # the zero row / column of the padding come from the producer
            v = F.pad(v, (1, 0, 1, 0))
            assert not hi[:, :, 0].any() and not hi[:, :, :, 0].any() and not lo[:, :, 0].any() and not lo[:, :, :, 0].any()
        _assert_split(hi[:, :C], lo[:, :C], [v], (pad_tl, mul2))


@pytest.mark.parametrize('transpose,flip', [(False, False), (True, False), (True, True)])
@pytest.mark.parametrize('scale', [1.0, 1.0 / math.sqrt(9 * 24)], ids=['scale1', 'rsqrt216'])
def test_pack_conv3x3_f16s_records(transpose, flip, scale, dev):
    """oodgan_pack_conv3x3_f16s, (Co,Ci) = (40,24): the records hold w * scale * 2^e (pack_f16s_kernel: w * fp32(2^e * scale)), the rows M .. Mp and
    the contraction channels K .. 16*ceil(K/16) are zero, unscale2 = {2^-e, 2^e} with max|w * scale| * 2^e in [512, 1024)."""
    from oodgan import ops
    Co, Ci = 40, 24
    w = R.synth.normal('prod.w', (Co, Ci, 3, 3), 6, 0.07)
    j = torch.arange(-9, -2, dtype=torch.float32)
    w[:7, :, 0, 0] = ((1 + 2.0 ** -11) * 2.0 ** j)[:, None]             # ties when scale is a power of two
    w[7:14, :, 1, 1] = (-(1 + 3 * 2.0 ** -11) * 2.0 ** j)[:, None]
    wpk = ops.pack_conv3x3(w.to(dev), scale, transpose=transpose, flip=flip, precision='f16s')
    un, sc = (float(v) for v in wpk.unscale.cpu())
    assert un * sc == 1.0 and math.frexp(sc)[0] == 0.5
    assert 512.0 <= float((w.double() * scale).abs().max()) * sc < 1024.0
    assert (un, sc) == R.pow2_scale((w * torch.tensor(scale, dtype=torch.float32)).abs().max())
    weff = w.transpose(0, 1) if transpose else w                           # (M,K,3,3): m = output, k = contraction
    if flip:
        weff = weff.flip([2, 3])
    M, K = weff.shape[:2]
    hi, lo = R.decode_wpk(wpk.data, K, M)
    assert hi.shape[0] == 64 and hi.shape[1] == (K + 15) // 16 * 16
    assert not hi[M:].any() and not lo[M:].any() and not hi[:, K:].any() and not lo[:, K:].any()
    v = weff * (torch.tensor(scale, dtype=torch.float32) * sc)
    _assert_split(hi[:M, :K], lo[:M, :K], [v], (transpose, flip, scale))


@pytest.mark.parametrize('route,B,K,M,H,W', [('s1big', 1, 80, 96, 17, 33), ('s1v2', 2, 40, 32, 10, 36)])
def test_ys_sform_written_by_the_conv(route, B, K, M, H, W, dev, tunable):
    """The S-form of act(y) * ys_scale a stride-1 conv writes for its consumer — by the 8-wave kernel from its registers, by the tile kernel
    from its LDS epilogue — obeys the format's inequalities against the returned y; border, tile padding and padded channels stay zero."""
    from oodgan import _lib, ops
    tunable('s1_big_min_items', 1)
    x = R.synth.normal('prod.yx', (B, K, H, W), 7)
    s = R.synth.normal('prod.ys', (B, K), 8, 0.3, 1.0)
    w = R.synth.normal('prod.yw', (M, K, 3, 3), 9, 1.0 / math.sqrt(9 * K))
    d = R.synth.normal('prod.yd', (B, M), 10, 0.3, 1.0)
    s2 = R.synth.normal('prod.ys2', (B, M), 11, 0.3, 1.0)
    nz, bias = R.synth.normal('prod.ynz', (B, 1, H, W), 12), R.synth.normal('prod.yb', (M,), 13, 0.5)
    xs = ops.to_sform(x.to(dev), s.to(dev))
    wpk = ops.pack_conv3x3(w.to(dev), precision='f16s')
    ys = ops.SForm(B, M, H, W, dev)
    _lib.dispatch_reset()
    y = ops.conv3x3(xs, wpk, M, ops.CONV_S1, out_scale=d.to(dev), bias=bias.to(dev), noise=nz.to(dev), noise_weight=torch.tensor([0.37], device=dev),
                    act=ops.ACT_LRELU, ys=ys, ys_scale=s2.to(dev))
    assert _counts(_lib) == {route: 1} and (route != 's1big' or _lib.dispatch_count('s1big_ys') == 1)
    hi, lo, rest = R.decode_sform(ys.data, B, M, H, W)
    assert not rest.any() and not hi[:, M:].any() and not lo[:, M:].any()
    _assert_split(hi[:, :M], lo[:, :M], [y.cpu() * s2[:, :, None, None]], route)
