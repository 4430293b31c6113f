"""The backward producers (csrc/bwd_producers.hip: oodgan_act_bwd_sform, oodgan_act_bwd_sform_f, the blur^T tile kernel and the blur^T strip
walk with its XTRA / PRE / rank-one / hi-only instances) and the two-pass root oodgan_blurT_to_sform_phases held to fp32-class accuracy against a
float64 reference of the operation (tests/bwd_producer_ref.py), at every walk geometry.

The bar of every figure is 4 x yardstick, the yardstick = the float32 model of the same chain on the CPU against the float64 reference, computed
in the test (one factor 2 for FMA contraction, one for another summation order); tests/test_bwd_producer_ref_cpu.py proves that seven subtly
wrong kernels err by at least 10 bars on the figure they touch.  Figures: e_max = max|d| / max|ref| and e_rms = rms(d) / rms(ref) on the record
values hi + lo, on r and on t_sum over (B,C); the relative error of the recorded maximum; for hi-only records what exceeds the half-ulp of f16,
|hi - ref| - 2^-11 |ref|, over max|ref|, held to the fp32 bar of the full records.  Every call also asserts its dispatch counter, exact zeros in
the padded channels and in everything that is not an image record, that a NaN-filled buffer comes back with every image record finite, and that
oodgan_absmax_scale_check keeps flag 0 and publishes exactly pow2_scale(m) of the reference.

The blur kernels are outer([1,2,4,1], [1,3,3,2]) * 4/72 (rank one, neither palindromic nor symmetric: a kernel that flips or swaps its taps
errs by 0.6 of the maximum) and the same with two entries moved (not rank one).  The strip walk runs every call with the launcher's own segments
and with the tunable blurt_seg_rows at 17 (odd: the single-step tail of walk() in every segment, segment starts on odd rows) and H + 1 (one
segment), w32 also at 19 — the segment heights the large layers of the workload have (18, 19, 35, 74) and no unit-test shape reaches by itself.
The window calls repeat one call with the range scale at both ends of [2^-8, 2^15): floor(log2(m * scale)) = -7 (lo halves subnormal; the
yardstick is recomputed, the float32 model makes the same f16 split) and 14, and once 2^20 off, which must be flagged.

Measured on an MI355X (the largest error / yardstick over the calls of a case, per figure; the bar is 4; "records e_max" is the error of the call
with the largest ratio — for w34 a window call with subnormal lo halves, whose yardstick is 2.3e-6; the smallest sabotage is the wrong kernel of
bwd_producer_ref.sabotages that comes closest to its bar, over the case's calls at their own range scale):

| case | segments (blurt_seg_rows) | records e_max | / yardstick | e_rms / y. | hi excess / y. | r e_max / y. | r e_rms / y. | t e_max / y. | t e_rms / y. | m / y. | smallest sabotage |
|---|---|---|---|---|---|---|---|---|---|---|---|
| w32 | 16+16+1 (0) | 2.23e-07 | 1.10 | 0.89 | 0.06 | 1.32 | 1.48 | - | - | 0.68 | C: 47 bars |
| w32 | 17+16 (17) | 2.23e-07 | 1.10 | 0.89 | 0.06 | 1.80 | 1.57 | - | - | 0.68 | C: 47 bars |
| w32 | 19+14 (19) | 2.23e-07 | 1.10 | 0.89 | 0.06 | 1.64 | 1.76 | - | - | 0.68 | C: 47 bars |
| w32 | 33 (33) | 2.23e-07 | 1.10 | 0.89 | 0.06 | 2.12 | 2.08 | - | - | 0.68 | C: 47 bars |
| w64 | 16+16+2 (0) | 2.00e-07 | 0.89 | 0.87 | - | 1.82 | 1.52 | - | - | 0.70 | C: 36 bars |
| w64 | 17+17 (17) | 2.00e-07 | 0.89 | 0.87 | - | 1.84 | 1.62 | - | - | 0.70 | C: 36 bars |
| w64 | 34 (34) | 2.00e-07 | 0.89 | 0.87 | - | 2.18 | 1.81 | - | - | 0.70 | C: 36 bars |
| w34 | 16+16+16 (0) | 2.30e-06 | 1.00 | 1.00 | - | 2.42 | 1.77 | - | - | 0.26 | C: 51 bars |
| w34 | two-pass root | 1.50e-07 | 1.00 | 1.00 | - | - | - | - | - | - | - |
| w34 | 17+17+14 (17) | 2.30e-06 | 1.00 | 1.00 | - | 2.71 | 1.91 | - | - | 0.26 | C: 51 bars |
| w34 | 48 (48) | 2.30e-06 | 1.00 | 1.00 | - | 2.94 | 3.08 | - | - | 0.26 | C: 51 bars |
| w66 | 16+16+9 (0) | 1.56e-07 | 0.88 | 0.87 | 0.06 | 1.94 | 1.83 | - | - | 1.00 | C: 35 bars |
| w66 | two-pass root | 1.99e-07 | 1.00 | 1.00 | - | - | - | - | - | - | - |
| w66 | 17+17+7 (17) | 1.56e-07 | 0.88 | 0.87 | 0.06 | 2.40 | 1.92 | - | - | 1.00 | C: 35 bars |
| w66 | 41 (41) | 1.56e-07 | 0.88 | 0.87 | 0.06 | 5.59 | 3.16 | - | - | 1.00 | C: 35 bars |
| t2 | - | 1.28e-07 | 0.75 | 0.95 | - | 1.66 | 1.34 | 1.04 | 1.09 | 1.00 | C: 282 bars |
| t18x32 | - | 1.98e-07 | 0.94 | 0.86 | - | 1.14 | 1.16 | 0.72 | 0.99 | 1.00 | C: 45 bars |
| t7x34 | - | 2.48e-07 | 1.00 | 1.00 | - | 1.60 | 2.24 | - | - | 0.88 | C: 52 bars |
| t31x30 | - | 1.69e-07 | 0.72 | 0.86 | - | 1.67 | 1.32 | - | - | 1.00 | C: 52 bars |
| t33x36 | - | 1.13e-07 | 0.60 | 0.85 | - | 1.93 | 1.30 | 0.57 | 0.72 | 0.12 | C: 43 bars |
| p4x4 | - | 8.70e-08 | 1.00 | 1.00 | - | 1.22 | 0.75 | 0.55 | 0.73 | 1.19 | G: 297 bars |
| p8x20 | - | 1.42e-07 | 1.00 | 1.00 | - | 0.99 | 1.03 | 0.95 | 0.82 | 1.00 | G: 322 bars |
| p16x32 | - | 1.12e-07 | 1.00 | 1.00 | - | 1.10 | 1.27 | 1.48 | 1.31 | 0.52 | G: 460 bars |
| p40x36 | - | 1.26e-07 | 1.00 | 1.00 | - | 1.59 | 1.40 | 0.92 | 0.99 | 0.44 | G: 410 bars |
| f48x64 | - | 1.27e-07 | 0.88 | 0.88 | - | 0.61 | 0.76 | 0.98 | 0.82 | 0.41 | G: 425 bars |
| f9x20 | - | 6.63e-08 | 0.82 | 0.85 | - | 1.30 | 1.18 | 1.40 | 1.13 | 0.10 | G: 386 bars |
| f23x28 | - | 1.31e-07 | 0.74 | 0.87 | - | 1.93 | 1.10 | 1.03 | 0.81 | 0.10 | G: 442 bars |

A ratio of 1.00 on the records means the kernel's values are the float32 model's, bit for bit.  The one figure above 4 is e_max of r of the hi-only
PRE call of w66 when the whole height is ONE segment (5.59; 5.32e-7): 328 dependent fp32 additions in one accumulator per thread, against the blocked
sum of the CPU — the same call sits at 1.94 and 2.40 with segments of 16 and 17 rows, its e_rms stays inside the bar.  bwd_producer_ref.MEASURED_ABOVE
gives the argument and its bar: 2 x the measured value, under 1/10 of the smallest sabotage of r.  The first run of this module found no bug in
csrc/bwd_producers.hip or in the two-pass root: the rank-one paths of the strip walk and of the tile kernel, and oodgan_blurT_to_sform_phases,
apply the non-palindromic, non-symmetric kernel in the documented direction.
"""
import pytest
import torch

import bwd_producer_ref as R

pytestmark = pytest.mark.gpu

COUNTERS = ('blurt_strip', 'blurt_tile', 'actbwd_sform', 'actbwd_sform_f')
WANT = {'strip': 'blurt_strip', 'tile': 'blurt_tile', 'plain': 'actbwd_sform', 'fform': 'actbwd_sform_f'}


@pytest.fixture(scope='module')
def dev():
    return torch.device('cuda:0')


def _counts(_lib):
    return {r: _lib.dispatch_count(r) for r in COUNTERS if _lib.dispatch_count(r)}


def _decode(c, k, dst):
    """-> (value (B,C,..) float64, everything that must be exactly zero)."""
    up = c.fam in ('strip', 'tile')
    if k.hi:
        hi, rest = R.decode_sform_phases_hi(dst.data, c.B, c.C, c.H, c.W)
        return hi[:, :c.C], hi, [hi[:, c.C:], rest]
    hi, lo, rest = (R.decode_sform_phases if up else R.decode_sform)(dst.data, c.B, c.C, c.H, c.W)
    return (hi + lo)[:, :c.C], hi + lo, [hi[:, c.C:], lo[:, c.C:], rest]


def _produce(c, k, o, scale_pair, dev, fill=None):
    """One producer call on the GPU -> (dst, r, t, part_max, state) and the counters it ticked."""
    from oodgan import _lib, ops
    t = lambda v: None if v is None else v.to(dev)
    up = c.fam in ('strip', 'tile')
    dst = (ops.SFormPhases if up else ops.SForm)(c.B, c.C, c.H, c.W, dev)
    if fill is not None:
        dst.data.fill_(fill)
    state = torch.tensor(scale_pair, dtype=torch.float32, device=dev)
    kw = dict(g_rgb=t(o['g_rgb']), w_rgb=t(o['w_rgb']), s_rgb=t(o['s_rgb'])) if k.rgb else {}
    if up:
        kw['blur_kernel'] = t(o['k'])
    if k.hi:
        assert ops.blurT_hi_supported(c.H, c.W)
        kw['hi_only'] = True
    out = t(o['out'])
    if k.pre:
        link = ops.DotActGrad()
        link.dot_part, link.scale = t(o['dot_part']), t(o['dot_scale'])
        kw['dot_of'] = link
    if c.fam == 'fform':
        out = ops.FForm(t(R.encode_fform(o['out'])))
        assert torch.equal(out.to_nchw().cpu(), o['out'])           # oodgan_from_fform: the round trip is exact
    _lib.dispatch_reset()
    r, ts, part_m = ops.act_bwd_producer(out, t(o['g_feat']), t(o['noise']), t(o['nw']), t(o['bias']), t(o['d']), state, dst, **kw)
    counts = _counts(_lib)
    torch.cuda.synchronize()
    return dst, r, ts, part_m, state, counts


def _check_scale(part_m, state, m, want_flag, dev):
    from oodgan import ops
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    ops.absmax_scale_check(part_m, state, flag)
    assert flag.item() == want_flag, flag.item()
    assert tuple(state.cpu().tolist()) == R.pow2_scale(m), (state.cpu().tolist(), R.pow2_scale(m))


def _figures(tag, cid, call_id, seg, win, e, Y, failures, worst):
    for key in sorted(e):
        y = Y[('rec', 'max') if key == ('hi', 'excess') else key]
        b = R.bar_of(cid, call_id, seg, win, key, Y)
        print(f'{tag:44s} {key[0]:3s} {key[1]:6s}: {e[key]:.2e}  yardstick {y:.2e}  ratio {e[key] / y:.2f}')
        worst[key] = max(worst.get(key, 0.0), e[key] / y)
        if not e[key] <= b:
            failures.append((tag, key, e[key], y, b))


def _check(c, seg, dev, tunable, twopass=False):
    from oodgan import _lib, ops
    if c.fam == 'strip':
        tunable('blurt_seg_rows', seg)
    failures, worst = [], {}
    for k in c.calls:
        for win in ((None, 'lo', 'hi') if c.window and k is c.calls[0] else (None,)):
            o, mul2, ref, Y = R.analysis(c.id, k.id, win)
            tag = f'{c.id} {k.id} seg={seg} win={win}'
            dst, r, ts, part_m, state, counts = _produce(c, k, o, mul2, dev)
            assert counts == {WANT[c.fam]: 1}, (tag, counts)                # the kernel named is the kernel that ran
            val, full, zeros = _decode(c, k, dst)
            assert torch.isfinite(full).all(), tag
            for z in zeros:                                                 # padded channels, border, tile padding, unused plane halves
                assert not z.any(), tag
            assert (ts is not None) == k.rgb
            got = dict(rec=val, r=r.double().cpu(), t_sum=None if ts is None else ts.double().cpu(), m=float(part_m.max().item()))
            _figures(tag, c.id, k.id, seg, win, R.errors(got, ref, k.hi), Y, failures, worst)
            _check_scale(part_m, state, ref['m'], 0, dev)
            # every record is written: a NaN-filled buffer comes back with all image records finite, and with the same bits
            dst2 = _produce(c, k, o, mul2, dev, fill=float('nan'))[0]
            _, full2, _ = _decode(c, k, dst2)
            assert torch.isfinite(full2).all() and torch.equal(full2, full), tag
            if c.window and win is None and k is c.calls[0]:
                # one more call with the scale 2^20 off (m * scale = 2^-11, below the window): flagged, and the published next scale is still the right one
                off = (mul2[0] * 2.0 ** 20, mul2[1] * 2.0 ** -20)
                _, _, _, pm, st, _ = _produce(c, k, o, off, dev)
                _check_scale(pm, st, ref['m'], 1, dev)
        if twopass and k.twopass:
            # the two-pass root on this call's g_pre (PRE: g_feat is g_pre): the same records from oodgan_blurT_to_sform_phases
            o, mul2, ref, Y = R.analysis(c.id, k.id, None)
            t = lambda v: v.to(dev)
            tag = f'{c.id} {k.id} two-pass'
            for fill in (None, float('nan')):
                buf = ops.SFormPhases(c.B, c.C, c.H, c.W, dev)
                if fill is not None:
                    buf.data.fill_(fill)
                _lib.dispatch_reset()
                ops.blurT_to_sform_phases(t(o['g_feat']), t(o['k']), t(o['d']), torch.tensor(mul2, dtype=torch.float32, device=dev), out=buf)
                assert _counts(_lib) == {}
                hi, lo, rest = R.decode_sform_phases(buf.data, c.B, c.C, c.H, c.W)
                assert torch.isfinite(hi).all() and torch.isfinite(lo).all(), tag
                if fill is None:
                    assert not rest.any() and not hi[:, c.C:].any() and not lo[:, c.C:].any(), tag
                    e = {key: v for key, v in R.errors(dict(rec=(hi + lo)[:, :c.C], r=ref['r'], t_sum=ref['t_sum'], m=ref['m']), ref).items() if key[0] == 'rec'}
                    _figures(tag, c.id, 'two-pass', seg, None, e, Y, failures, worst)
    print(f'SUMMARY {c.id} seg={seg} ' + ' '.join(f'{key[0]}.{key[1]}={v:.2f}' for key, v in sorted(worst.items())))
    assert not failures, failures


def _params(fam):
    return [pytest.param(c.id, seg, id=f'{c.id}-seg{seg}') for c in R.CASES if c.fam == fam for seg in c.segs]


@pytest.mark.parametrize('cid,seg', _params('strip'))
def test_blurT_strip_walk_against_float64(cid, seg, dev, tunable):
    """Every template instance (XTRA x PRE) with the rank-one and the general kernel, hi-only records, per-sample / shared / no noise, no bias,
    at the launcher's own segments and at blurt_seg_rows = 17, H + 1 (w32: also 19); with the default segments also the two-pass root."""
    _check(R.case(cid), seg, dev, tunable, twopass=seg == 0)


@pytest.mark.parametrize('cid,seg', _params('tile'))
def test_blurT_tile_kernel_against_float64(cid, seg, dev, tunable):
    _check(R.case(cid), seg, dev, tunable)


@pytest.mark.parametrize('cid,seg', _params('plain'))
def test_act_bwd_sform_against_float64(cid, seg, dev, tunable):
    _check(R.case(cid), seg, dev, tunable)


@pytest.mark.parametrize('cid,seg', _params('fform'))
def test_act_bwd_sform_f_against_float64(cid, seg, dev, tunable):
    _check(R.case(cid), seg, dev, tunable)
