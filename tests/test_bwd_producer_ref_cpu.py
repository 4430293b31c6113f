"""The float64 model of the backward producers (tests/bwd_producer_ref.py) checked on the CPU: the float32 model stays inside one bar of the
reference on every figure (the two cannot both be wrong the same way), every wrong kernel of ``sabotages`` errs by at least 10 bars on the
figure it touches, the range scale of every call is unambiguous, the layout coders are inverses, and every listed case has the geometry its
comment claims — from the launcher's arithmetic re-stated in Python.  No GPU."""
import math

import pytest
import torch

import bwd_producer_ref as R
import splitf16_ref as S

CALLS = [(c.id, k.id) for c in R.CASES for k in c.calls]


def _wins(c, k):
    return (None, 'lo', 'hi') if c.window and k is c.calls[0] else (None,)


def _geo(c, seg):
    return R.strip_geometry(c.B, c.C, c.H, c.W, seg) if c.fam == 'strip' else dict(seg_rows=None, nseg=1)


def _touched(name, e):
    what = R.TOUCHES[name]
    keys = [k for k in e if k[0] == what or (what == 'rec' and k[0] == 'hi')]
    assert keys, (name, sorted(e))
    return keys


@pytest.mark.parametrize('cid,call_id', CALLS)
def test_model_within_one_bar_and_sabotages_beyond_ten(cid, call_id):
    c = R.case(cid)
    k = R.call_of(c, call_id)
    seen = set()
    for win in _wins(c, k):
        o, mul2, ref, Y = R.analysis(cid, call_id, win)
        # the range scale: a power-of-two pair, the maximum where the call wants it, and not within 2^-20 of a power of two (the fp32 maximum
        # of a kernel then has the same exponent: the next published scale is unambiguous)
        m = float(ref['m'])
        assert mul2[0] * mul2[1] == 1.0 and math.frexp(mul2[1])[0] == 0.5
        lg = math.floor(math.log2(m * mul2[1]))
        assert lg == (9 if win is None else R.WINDOWS[win]), (win, lg)
        f = math.frexp(m)[0]                                     # in [0.5, 1)
        assert f - 0.5 > 2.0 ** -20 and 1.0 - f > 2.0 ** -20, m
        assert 2.0 ** -8 <= m * mul2[1] < 2.0 ** 15             # inside the window of oodgan_absmax_scale_check
        # the model: finite, and inside ONE bar on every figure (the hi-only excess included)
        mod = R.model32(o, mul2[1], k.hi)
        assert all(bool(torch.isfinite(v).all()) for v in mod.values() if v is not None)
        e = R.errors(mod, ref, k.hi)
        assert set(e) == (set(Y) - {('rec', 'max'), ('rec', 'rms')}) | {('hi', 'excess')} if k.hi else set(e) == set(Y)
        for key, v in e.items():
            assert v <= R.bar(key, Y), (win, key, v, R.bar(key, Y))
        # the bar table of measured exceptions may not outgrow a tenth of the smallest sabotage; every sabotage that exists: >= 10 bars
        for seg in c.segs:
            g = _geo(c, seg)
            sab = R.sabotages(o, mul2[1], ref, c.fam, k.hi, c.W, g['seg_rows'], g['nseg'])
            for name, es in sab.items():
                if win == 'lo' and name in 'CEG':
                    continue        # at the low end of the window the lo half itself is a few subnormal bits: losing it costs what the yardstick costs
                seen.add(name)
                for key in _touched(name, es):
                    b = max(R.bar_of(cid, call_id, sg, win, key, Y) for sg in c.segs)        # the widest bar the figure has at any segment setting
                    assert es[key] >= 10.0 * b, (win, seg, name, key, es[key], b)
        if k.twopass and win is None:
            sab = R.sabotages(o, mul2[1], ref, 'twopass', False, c.W)
            assert set(sab) == ({'A', 'C', 'E'} if k.kern == 'r1' else {'C', 'E'})
            for name, es in sab.items():
                for key in _touched(name, es):
                    assert es[key] >= 10.0 * R.bar(key, Y), (name, key)
    # which sabotages a call must have had
    want = {'F'}
    if c.fam in ('strip', 'tile'):
        want |= (set() if k.hi else {'C', 'E'}) | ({'A'} if k.kern == 'r1' else set())
    if c.fam == 'strip':
        want |= {'D'} | ({'B'} if 2 * c.W > 64 else set())
    if c.fam in ('plain', 'fform'):
        want |= {'G'}
    assert seen == want, (seen, want)


def test_measured_above_stays_under_a_tenth_of_the_smallest_sabotage():
    """Every recorded exception names a figure that exists, lies above 4 x yardstick (else it has no place in the table), and its bar, 2 x the
    measured value, is at most 1/10 of the smallest error any wrong kernel of that call has on that figure (over the case's segment settings: the
    one-segment walk itself has no segment boundary to get wrong)."""
    for (cid, call_id, seg, win, what, metric), meas in R.MEASURED_ABOVE.items():
        c = R.case(cid)
        k = R.call_of(c, call_id)
        assert seg in c.segs and metric == 'max'
        o, mul2, ref, Y = R.analysis(cid, call_id, win)
        assert meas > R.bar((what, metric), Y)
        hits = []
        for sg in c.segs:
            g = _geo(c, sg)
            for name, es in R.sabotages(o, mul2[1], ref, c.fam, k.hi, c.W, g['seg_rows'], g['nseg']).items():
                if R.TOUCHES[name] == what:
                    hits.append(es[(what, metric)])
        assert hits and 2.0 * meas <= min(hits) / 10.0, (cid, call_id, hits)


def test_blur_kernels_take_the_path_they_are_meant_for():
    r1, gen, sym = R.blur_kernel('r1'), R.blur_kernel('gen'), R.blur_kernel('sym')
    assert abs(float(r1.sum()) - 4.0) < 1e-6
    assert R.is_rank_one_strip(r1) and R.is_rank_one_tile(r1) and R.is_rank_one_strip(sym) and R.is_rank_one_tile(sym)
    assert not R.is_rank_one_strip(gen) and not R.is_rank_one_tile(gen)
    # neither palindromic nor symmetric: every flip and the transpose are other kernels
    for other in (torch.flip(r1, [0]), torch.flip(r1, [1]), torch.flip(r1, [0, 1]), r1.t()):
        assert float((other - r1).abs().max()) > 0.05
    assert torch.equal(torch.flip(sym, [0]), sym) and torch.equal(sym.t(), sym)
    # the point of the kernel: with the vertical taps reversed the symmetric kernel gives the SAME g2, this one does not
    g = R.synth.normal('bwdprod.flip', (1, 2, 8, 8), 3).double()
    for k, same in ((sym, True), (r1, False)):
        kf = torch.flip(k, [0, 1]).double()
        a, b = R._blurT(g, kf), R._blurT(g, torch.flip(kf, [0]))
        assert (float((a - b).abs().max()) == 0.0) == same
        assert same or float((a - b).abs().max() / a.abs().max()) > 0.3


def test_reference_blur_is_the_adjoint_of_the_forward_blur():
    """g2 = blur^T(g): <blur(z), g> == <z, g2> for the forward Blur(pad=(1,1)) of the up-sampling layer, z of size (2H+1) x (2W+1):
    blur(z)[y,x] = sum_{a,b} kflip[a][b] * z[y+a-1][x+b-1] (upfirdn2d: a true convolution with the kernel).  Pins the direction of both axes of
    the reference against an operation written differently."""
    import torch.nn.functional as F
    k = R.blur_kernel('r1').double()
    kflip = torch.flip(k, [0, 1])
    z = R.synth.normal('bwdprod.adj.z', (1, 3, 9, 13), 1).double()
    g = R.synth.normal('bwdprod.adj.g', (1, 3, 8, 12), 2).double()
    fwd = F.conv2d(F.pad(z.reshape(3, 1, 9, 13), (1, 1, 1, 1)), kflip.reshape(1, 1, 4, 4)).reshape(1, 3, 8, 12)
    g2 = R._blurT(g, k)          # the adjoint correlates with the UNflipped kernel ...
    assert abs(float((fwd * g).sum() - (z * g2).sum())) <= 1e-12 * float((fwd * g).abs().sum())
    # ... (the producers take a kernel argument kk and apply flip(kk): the engine hands them kk = flip(k))


def test_layout_coders_are_inverses():
    B, C, H, W = 2, 24, 5, 33
    KC, Hq, Wq = S.sp_dims(C, H, W)
    hi = R.synth.normal('bwdprod.lay.hi', (B, C, 2 * H + 1, 2 * W + 1), 1).half()
    buf = R.encode_sform_phases_hi(hi, B, C, H, W)
    assert buf.numel() == B * KC * 4 * Hq * Wq * 32             # a hi-only buffer has the size of the full-record buffer
    got, rest = R.decode_sform_phases_hi(buf, B, C, H, W)
    assert torch.equal(got[:, :C], hi.double()) and not got[:, C:].any() and not rest.any()
    assert got.numel() + rest.numel() == buf.numel()
    # decoding random records and encoding the image part again reproduces the image part
    rnd = R.synth.normal('bwdprod.lay.rnd', (buf.numel(),), 2).half()
    g2, r2 = R.decode_sform_phases_hi(rnd, B, C, H, W)
    back, _ = R.decode_sform_phases_hi(R.encode_sform_phases_hi(g2[:, :C].half(), B, C, H, W), B, C, H, W)
    assert torch.equal(back[:, :C], g2[:, :C]) and g2.numel() + r2.numel() == rnd.numel()
    # the first 16 bytes of record (i,j) = (1,2) of plane (b,kc,py,px) = (1,0,1,0): channels 0-7 of pixel (3,4) of sample 1
    unit = ((1 * KC + 0) * 4 + 2) * (Hq * Wq * 4) + (1 * Wq + 2) * 2
    assert torch.equal(buf[unit * 8:unit * 8 + 8], hi[1, 0:8, 3, 4])
    # F-form
    x = R.synth.normal('bwdprod.lay.f', (2, 32, 3, 5), 3)
    f = R.encode_fform(x)
    assert f.shape == x.shape and torch.equal(R.decode_fform(f), x)
    assert torch.equal(R.encode_fform(R.decode_fform(f)), f)
    assert float(f.reshape(-1)[((1 * 2 + 1) * 15 + 7) * 16 + 3]) == float(x[1, 19, 1, 2])       # (b, c, p) = (1, 19, 7)


# what each case is in the table for — the test fails if the case does not have this geometry
STRIP_GEO = {
    # (seg setting) -> rows per segment; extra / nstrips / KC; quads of the last strip, whether it has a right halo column
    'w32': dict(KC=2, extra=1, nstrips=1, last_quads=16, last_right_halo=False, rows={0: [16, 16, 1], 17: [17, 16], 19: [19, 14], 33: [33]}),
    'w64': dict(KC=1, extra=0, nstrips=3, last_quads=0, last_right_halo=False, rows={0: [16, 16, 2], 17: [17, 17], 34: [34]}),
    'w34': dict(KC=2, extra=0, nstrips=2, last_quads=1, last_right_halo=False, rows={0: [16, 16, 16], 17: [17, 17, 14], 48: [48]}),
    'w66': dict(KC=3, extra=0, nstrips=3, last_quads=1, last_right_halo=False, rows={0: [16, 16, 9], 17: [17, 17, 7], 41: [41]}),
}
TILE_GEO = {'t2': (1, 1, 1), 't18x32': (3, 2, 5), 't7x34': (2, 2, 2), 't31x30': (2, 1, 8), 't33x36': (1, 2, 9)}        # KC, tiles_x, tiles_y
CHUNKS = {'p4x4': (0, 16), 'p8x20': (0, 160), 'p16x32': (1, 0), 'p40x36': (2, 416), 'f48x64': (6, 0), 'f9x20': (0, 180), 'f23x28': (1, 132)}


def test_case_list_reaches_every_branch():
    strip = [c for c in R.CASES if c.fam == 'strip']
    assert [c.id for c in strip] == list(STRIP_GEO)
    inst = set()
    for c in strip:
        want = STRIP_GEO[c.id]
        assert set(c.segs) == set(want['rows']) and 0 in c.segs and 17 in c.segs and c.H + 1 in c.segs
        for seg in c.segs:
            g = R.strip_geometry(c.B, c.C, c.H, c.W, seg)
            assert g['strip_ok'] and g['rows'] == want['rows'][seg], (c.id, seg, g)
            assert g['steps'] == [r + 2 for r in g['rows']] and g['tail'] == [r % 2 == 1 for r in g['rows']]
            assert all(r >= 16 for r in g['rows'][:-1]) and sum(g['rows']) == c.H + 1
            for key in ('KC', 'extra', 'nstrips', 'last_quads', 'last_right_halo'):
                assert g[key] == want[key], (c.id, key, g[key])
        assert R.strip_geometry(c.B, c.C, c.H, c.W, c.H + 1)['nseg'] == 1
        assert all(not k.rgb and k.kern is not None for k in c.calls) and max(2 * c.H, 2 * c.W) <= 132 and c.B <= 2 and c.C <= 48
        inst |= {(bool(STRIP_GEO[c.id]['extra']), k.pre, k.kern, k.hi) for k in c.calls}
    # segment geometry: 17 puts the tail step in every full segment and segment starts on odd rows; the defaults have a one-row segment (w32),
    # a clipped even one (w64), none clipped (w34) and an odd clipped one (w66)
    assert all(R.strip_geometry(c.B, c.C, c.H, c.W, 17)['tail'][0] for c in strip)
    assert (c := R.case('w34')).C % 16 != 0 and R.case('w66').C // 16 == 3
    # all four template instances (XTRA x PRE), each with the rank-one and with the general kernel; hi-only on the XTRA instance and on w66
    for xtra in (False, True):
        for pre in (False, True):
            for kern in ('r1', 'gen'):
                assert any(i[:3] == (xtra, pre, kern) for i in inst), (xtra, pre, kern)
    assert any(k.hi for k in R.case('w32').calls) and any(k.hi for k in R.case('w66').calls)
    noises = {k.noise for c in strip for k in c.calls}
    assert noises == {'per', 'shared', None} and sum(not k.bias for c in strip for k in c.calls) == 1
    assert any(k.noise == 'shared' for k in R.case('w64').calls)            # shared noise needs B > 1 to differ from per-sample noise
    # PRE calls keep a kernel-side term of r: noise or bias present
    assert all(k.noise is not None or k.bias for c in strip for k in c.calls if k.pre)
    # the two-pass root runs at w34 and w66 with both kernels
    assert {(c.id, k.kern) for c in strip for k in c.calls if k.twopass} == {('w34', 'r1'), ('w34', 'gen'), ('w66', 'r1'), ('w66', 'gen')}
    assert all(k.pre for c in R.CASES for k in c.calls if k.twopass)
    # tile kernel: what keeps each case off the strip walk, and the tile counts
    tile = [c for c in R.CASES if c.fam == 'tile']
    assert [c.id for c in tile] == list(TILE_GEO)
    for c in tile:
        g = R.tile_geometry(c.C, c.H, c.W)
        assert (g['KC'], g['tiles_x'], g['tiles_y']) == TILE_GEO[c.id] and c.W % 2 == 0
        assert all(k.rgb or c.H < 32 or c.W < 32 for k in c.calls) and all(not k.pre and not k.hi for k in c.calls)
    assert R.case('t18x32').W == 32 and R.case('t31x30').H + 1 == 32 and R.case('t33x36').H >= 32 and R.case('t33x36').W >= 32
    assert {k.kern for c in tile for k in c.calls} == {'r1', 'gen'}
    # act_bwd_sform / _f: chunks of 512 pixels
    for c in R.CASES:
        if c.fam in ('plain', 'fform'):
            assert R.plain_chunks(c.H, c.W) == CHUNKS[c.id] and c.W % 4 == 0
        if c.fam == 'plain':
            assert {k.rgb for k in c.calls} == {True, False}
        if c.fam == 'fform':
            assert c.C % 16 == 0 and all(k.rgb and k.kern is None for k in c.calls)
    plain = [k for c in R.CASES if c.fam == 'plain' for k in c.calls]
    assert sum(k.noise == 'shared' for k in plain) == 1 and sum(k.noise is None and not k.bias for k in plain) == 1
    assert [c.id for c in R.CASES if c.window] == ['w34', 'p40x36']
