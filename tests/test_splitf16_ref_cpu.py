"""The float64 model of the split-f16 convs (tests/splitf16_ref.py) checked on its own, without a GPU: the three-term formula stays
inside its derived bound, every sabotage the GPU test must catch is at least 10 x that test's bar (4 x yardstick) for y and for
dot, and the layout decoders invert independent encoders bit for bit."""
import pytest
import torch

import splitf16_ref as R

BAR_FACTOR = 4.0        # tests/test_hip_conv_accuracy.py: bar = 4 x yardstick
MIN_RATIO = 10.0        # smallest sabotage error / bar


_case = R.analysis


@pytest.mark.parametrize('cid', R.CASE_IDS)
def test_three_term_formula_within_its_bound(cid):
    """|model - ref| <= 3 * 2^-22 * conv(|x|, |w|) elementwise on the raw accumulators: each operand keeps 22 bits (hi 11, lo 11: relative
    error 2^-22 each), the dropped lo*lo term is 2^-22 of the product, the fp32 product x * in_scale adds 2^-24."""
    c = R.CASES[R.CASE_IDS.index(cid)]
    for call in c.calls:
        o, ref, _, _ = _case(cid, call)
        bound = 3 * 2.0 ** -22 * R.conv_raw(o['mode'], R.true_input(o).abs(), R.true_weight(o).abs())
        err = (R.model_raw(o) - ref[2]).abs()
        print(f'{cid:18s} {call:9s} largest |model - ref| / conv(|x|,|w|) = {float((err / bound).max()) * 3 * 2.0 ** -22:.2e} (bound {3 * 2.0 ** -22:.2e})')
        assert bool((err <= bound).all()), (call, float((err / bound).max()))


@pytest.mark.parametrize('cid', R.CASE_IDS)
def test_every_sabotage_is_ten_bars_away(cid):
    """The cap of the GPU test: no bar may exceed 1/10 of the case's smallest sabotage error; the bar it uses, 4 x yardstick, stays below
    that for both metrics, for y and for dot."""
    c = R.CASES[R.CASE_IDS.index(cid)]
    for call in c.calls:
        _, _, Y, sab = _case(cid, call)
        for key, y in Y.items():
            smallest = min(s[key] for s in sab.values())
            print(f'{cid:18s} {call:9s} {key[0]:3s} e_{key[1]}: yardstick {y:.2e}  smallest sabotage {smallest:.2e}  ratio to the bar {smallest / (BAR_FACTOR * y):.0f}')
            assert smallest >= MIN_RATIO * BAR_FACTOR * y, (call, key, y, {k: s[key] for k, s in sab.items()})


def test_measured_bars_stay_under_the_cap():
    """The routes whose bar is 2 x their measured error (splitf16_ref.MEASURED_ABOVE): above 4 x yardstick, and at most 1/10 of the smallest
    sabotage error of that call."""
    for (cid, prec, call, what, metric), measured in R.MEASURED_ABOVE.items():
        assert prec in ('f16s', 'f32') and call in R.CASES[R.CASE_IDS.index(cid)].calls
        _, _, Y, sab = _case(cid, call)
        key = (what, metric)
        b = R.bar(cid, prec, call, key, Y)
        assert b == 2.0 * measured and measured > BAR_FACTOR * Y[key]
        assert MIN_RATIO * b <= min(s[key] for s in sab.values()), (cid, prec, call, key, b)


def test_pow2_scale_rule():
    for m in (1e-7, 0.37, 1.0, 511.9, 512.0, 1023.9, 1024.0, 3e4):
        un, sc = R.pow2_scale(m)
        assert un * sc == 1.0 and 512.0 <= m * sc < 1024.0
    assert R.pow2_scale(0.0) == (1.0, 1.0) and R.pow2_scale(float('inf')) == (1.0, 1.0)


def test_split_keeps_22_bits_and_derives_lo_from_the_stored_hi():
    j = torch.arange(-10, 9, dtype=torch.float32)
    ties = torch.cat([(1 + 2.0 ** -11) * 2.0 ** j, (1 + 3 * 2.0 ** -11) * 2.0 ** j, R.synth.normal('split.v', (4096,), 1, 300.0)])
    hi, lo = R.split(ties)
    v = ties.double()
    assert bool(((v - hi).abs() <= 2.0 ** -11 * v.abs()).all())
    assert bool(((v - (hi + lo)).abs() <= torch.clamp(2.0 ** -22 * v.abs(), min=2.0 ** -25)).all())
    # the ties round to even, and lo carries the whole remainder
    assert bool((hi[:19] == 2.0 ** j.double()).all()) and bool((lo[:19] == 2.0 ** (j.double() - 11)).all())


@pytest.mark.parametrize('C,H,W', [(24, 9, 37), (40, 9, 37)])
def test_decoders_invert_the_encoders(C, H, W):
    B = 2
    hi, lo = R.split16(R.synth.normal('dec.x', (B, C, H, W), 1, 100.0))
    buf = R.encode_sform(hi, lo, B, C, H, W)
    dh, dl, rest = R.decode_sform(buf, B, C, H, W)
    assert torch.equal(dh[:, :C], hi.double()) and torch.equal(dl[:, :C], lo.double())
    assert not dh[:, C:].any() and not dl[:, C:].any() and not rest.any()
    assert torch.equal(R.encode_sform(dh[:, :C].half(), dl[:, :C].half(), B, C, H, W), buf)
    hi, lo = R.split16(R.synth.normal('dec.p', (B, C, 2 * H + 1, 2 * W + 1), 2, 100.0))
    buf = R.encode_sform_phases(hi, lo, B, C, H, W)
    dh, dl, rest = R.decode_sform_phases(buf, B, C, H, W)
    assert torch.equal(dh[:, :C], hi.double()) and torch.equal(dl[:, :C], lo.double())
    assert not dh[:, C:].any() and not dl[:, C:].any() and not rest.any()
    M, K = 40, C
    hi, lo = R.split16(R.synth.normal('dec.w', (M, K, 3, 3), 3, 300.0))
    buf = R.encode_wpk(hi, lo, K, M)
    dh, dl = R.decode_wpk(buf, K, M)
    assert torch.equal(dh[:M, :K], hi.double()) and torch.equal(dl[:M, :K], lo.double())
    assert not dh[M:].any() and not dl[M:].any() and not dh[:, K:].any() and not dl[:, K:].any()
    # a marker in every buffer position comes back exactly once: the decoders are permutations
    ids = torch.arange(buf.numel(), dtype=torch.float64)
    a, b_ = R.decode_wpk(ids, K, M)
    assert torch.equal(torch.sort(torch.cat([a.reshape(-1), b_.reshape(-1)])).values, ids)
