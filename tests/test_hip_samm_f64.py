"""The SAMM / SAIM kernels (csrc/samm.hip) against float64, element by element, at the shapes where their loops branch.

Metric.  tests/samm_ref.py holds, for every op, the operation in plain torch (``ref``: float64 is the reference, float32 the band) and a
per-element scale A (``scale``): the same expression with every product and sum taken over absolute values, plus the hand-derived terms
of rstd, the activations and the resamplers (derivations beside the functions).  r = max_e |y_e - ref64_e| / (2^-24 A_e); where A_e = 0
the element must be equal.  The statistics that a fused pass returns are those of the float32 tensor it stored, so they are measured
against the float64 statistics of that tensor (samm_ref.measure).

Bars.  The bar of an op is 4 x the largest r of its float32 torch reference over the op's cases, rounded up to a power of two (the kernels
sum in another order, and the device's tanhf / expf / rsqrtf may be a few ulp further off than the CPU's), and for a case never above
n + 2, the any-order worst case of its n terms (samm_ref.terms).  The float32 r were measured on the CPU (test_float32_band prints them):

    op                  float32 r  bar       MI355X    op                  float32 r  bar   MI355X
    instnorm_stats      1.22       8         1.66      conv3x3_fewout      3.13       16    2.48
    affine_apply_stats  2.81       16        2.43      conv3x3_fewout2     6.28       32    2.48 (fewout_quad 1 and 0 alike)
    align_input_stats   1.62       8         2.79      align_head          2.38 *     16    2.98
    affine_apply        2.81       16 (5)    1.89      field_compose       1.22       8     1.00
    align_input         0.154      1         0.154     warp_blend          1.23       8     1.23
    instnorm_coeffs     1.93       8 (5)     1.61      mask_blend          0.159      1     0.159
    conv1x1             8.86       64 (K+3)  8.82      resize_nearest      bit-exact  0     bit-exact
    se_gate             1.38       8         1.38      resize_bilinear     0.426      2     0.427
    conv3x3_small       5.49       32 (9K+4) 3.67      resize_bicubic_ac   0.924      4     0.924
                                                       avgpool             13.0       64    4.37
    (in brackets: the n + 2 cap where it is the smaller one.  MI355X: the kernel's largest r over the op's cases, measured after the bars
    were fixed; no bar depends on it.  Every kernel is within 1.8x of its float32 torch counterpart.)
    * over the outputs >= 2^-126.  torch's float32 sigmoid returns 0 for sigmoid(-88.8) = 2.7e-39 and sigmoid(-100) = 3.7e-44 (r = 4.2e6 with
      them): the float32 band has nothing to say there, and the bar is the cap of an activation, 14 + 2.

Mutants (deliberately wrong float32 references; each must reach 100 x bar on at least one case — a condition on the inputs), smallest
over the ops that carry them, largest r over that op's cases:
    one-pass variance 2.4e5; last element of a plane dropped 5.3e5 (avgpool window) .. 2.2e7; element 4*256 counted twice 1.9e6; res ignored
    7.3e5; diff ignored 9.6e5; gamma / beta ignored 9.7e6; a channel dropped (last, 31, 32, 64) 8.3e6; bias dropped 1.5e7; SE last channel /
    hidden unit 32 / last hidden unit 5.9e8; ReLU omitted 4.0e10; shift applied to the padding 7.3e6; conv tap (2,2) dropped at channel
    7 / 8 / last 1.1e6; last column read as padding 1.4e7; 1x1 shortcut's last channel 1.4e7; sigmoid on channel 1 7e44; clip before the
    composition 4.3e4 (mask_blend, bar 1); alpha composed in the other order 3.5e5; field with s == S skipped 4.4e4; align_corners flipped
    4.4e5; source index off by one at the last row / column 1.4e5 (nearest: not equal); channel 8 of the warp dropped 8.4e6; pooling
    window end floor instead of ceil 3.0e6; nearest-exact instead of nearest: not equal.

Findings.
  * align_head returned sigmoid(v) = 0 for v < -88.72: expf(-v) overflows in 1 / (1 + expf(-v)), while the true values, 2.7e-39 at -88.8 and
    3.7e-44 at -100, are float32 numbers.  r = 3.9e6 .. 4.2e6 on all three cases (each holds +-88.8 and +-100; the figure is that of the same
    formula in float32 on the CPU) against a bar of 16.  The kernel now returns expf(v) below -87, where 1 + expf(v) rounds to 1, and is
    unchanged above: r = 2.98 on the MI355X.
  * align_input_stats was NOT bit-identical to align_input + instnorm_stats on the scalar path (HW % 4 != 0) once a thread makes more than one
    trip (HW > 256; the earlier test's only such shape was 9 x 13): at HW = 4099 the means of the IN(enc) planes differed in the last bits
    (-9.2692e-07 against -9.2133e-07).  __fmul_rn is a plain product to the compiler, which folded it into the running sum (v_fmac), so the
    sum was not that of the stored values.  The sums of that pass now go through add_rounded (contraction off); the float4 path, which every
    shape of the workload takes, compiled to the same instructions before and after.  test_fused_statistics_equal_two_passes holds it.
  * conv1x1: every row of the batch of eight (wide form) is bit-equal to the same image alone (narrow form), as samm.hip says.
  * conv3x3_fewout2 with fewout_quad = 0 and 1 is bit-equal exactly where the quad form cannot run (M != 3, M2 not in (0, 3), W % 4 != 0).
    Where it runs (1024 @32x32, 64 @20x44, 72 @13x36, 512 @128x128) the outputs differ in the last bits: the quad form adds two channels of a
    stage per wave and the four waves at the end.  No comment in samm.hip claims equality; each setting is held to the bar
    (quad 1.71 / one-pixel 2.38 at 64 @20x44).

The GPU part takes 5 s on the MI355X, the CPU part 7 s."""
import pytest
import torch

import samm_ref as S

gpu = pytest.mark.gpu

# op: (bar, float32 r it was derived from, r measured on the MI355X afterwards: a record, no test reads it)
BARS = {
    'instnorm_stats': (8, 1.22, 1.66), 'affine_apply_stats': (16, 2.81, 2.43), 'align_input_stats': (8, 1.62, 2.79),
    'affine_apply': (16, 2.81, 1.89), 'align_input': (1, 0.154, 0.154), 'instnorm_coeffs': (8, 1.93, 1.61), 'conv1x1': (64, 8.86, 8.82),
    'se_gate': (8, 1.38, 1.38), 'conv3x3_small': (32, 5.49, 3.67), 'conv3x3_fewout': (16, 3.13, 2.48), 'conv3x3_fewout2': (32, 6.28, 2.48),
    'align_head': (16, 2.38, 2.98), 'field_compose': (8, 1.22, 1.0), 'warp_blend': (8, 1.23, 1.23), 'mask_blend': (1, 0.159, 0.159),
    'resize_nearest': (0, 0.0, 0.0), 'resize_bilinear': (2, 0.426, 0.427), 'resize_bicubic_ac': (4, 0.924, 0.924), 'avgpool': (64, 13.0, 4.37),
}
MUTANT_FACTOR = 100
SENTINEL = -12345.0


def bar(op, inp):
    return min(BARS[op][0], S.terms(op, inp) + 2) if BARS[op][0] else 0


def _ids(op):
    return [S.case_id(c) for c in S.CASES[op]]


# ------------------------------------------------------------------ (a) the reference and the bars (CPU)
def _band(op, case):
    inp, ref64, A = S.case_bundle(op, case)
    y32 = S.ref(op, inp, S.F32)
    if op == 'align_head':      # the band of the outputs float32 torch can represent at all (see the module docstring)
        y32 = (torch.where(ref64[0].abs() < S.TINY, ref64[0], y32[0].double()),)
    return S.measure(op, case, y32)


@pytest.mark.parametrize('op', S.OPS)
def test_float32_band(op):
    """The float32 reference against the float64 one: finite on every case, and inside the band its bar was derived from."""
    band = {S.case_id(case): _band(op, case) for case in S.CASES[op]}
    worst = max(band.values())
    print(f'[{op}] float32 r: ' + ' '.join(f'{k}={v:.3g}' for k, v in band.items()) + f' | worst {worst:.3g}, bar {BARS[op][0]}')
    assert all(v == v and v != S.INF for v in band.values()), band
    assert set(BARS) == set(S.OPS)
    b = BARS[op][0]
    assert b == S.pow2ceil(4 * BARS[op][1]) or op == 'resize_nearest', 'the bar is 4 x the recorded float32 r, rounded up to a power of two'
    # the recorded r is at most b / 4 by construction; another CPU's float32 kernels may sum in another order: twice that, no more
    assert worst <= b / 2, f'the float32 reference left the band its bar was derived from: {worst} > {b} / 2'
    for case in S.CASES[op]:
        inp = S.case_bundle(op, case)[0]
        assert bar(op, inp) <= max(S.terms(op, inp) + 2, 0)
    if op == 'align_head':
        inp, ref64, A = S.case_bundle(op, S.CASES[op][1])
        full = S.r_value(S.ref(op, inp, S.F32), ref64, A)
        print(f'[align_head] float32 torch with the outputs below 2^-126: r = {full:.3g}')
        assert full > 1e6


@pytest.mark.parametrize('op', S.OPS)
def test_mutants_are_exposed(op):
    """Every wrong reference of the op is at least 100 bars away from the float64 reference on one of the op's cases."""
    best = {m: 0.0 for m in S.MUTANTS[op]}
    for case in S.CASES[op]:
        if (op, case) in S.HEAVY:
            continue
        inp = S.case_bundle(op, case)[0]
        for m, fn in S.MUTANTS[op].items():
            with torch.no_grad():
                best[m] = max(best[m], S.measure(op, case, tuple(fn(inp))))
    print(f'[{op}] mutants: ' + '; '.join(f'{m} {v:.3g}' for m, v in best.items()))
    need = MUTANT_FACTOR * max(BARS[op][0], 1)
    weak = {m: v for m, v in best.items() if not v >= need}
    assert not weak, (weak, need)


def test_cases_sit_on_both_sides_of_every_branch():
    """The dispatch conditions of csrc/samm.hip, restated: each has a case on either side."""
    def wide(B, K, M, HW):          # M > 16 && ceil(HW/256) * ceil(M/64) * B >= 1024
        return M > 16 and -(-HW // 256) * -(-M // 64) * B >= 1024
    assert {wide(*c) for c in S.CASES['conv1x1']} == {True, False}
    assert wide(8, 33, 65, 16129) and not wide(1, 33, 65, 16129)
    assert {c[0] % 4 == 0 for c in S.CASES['instnorm_stats']} == {True, False} and any(c[0] > 4096 for c in S.CASES['instnorm_stats'])

    def wave(case):                 # (ceil(Hin/Hout) + 1) * (ceil(Win/Wout) + 1) >= 128
        _, (Hi, Wi), (Ho, Wo) = case
        return (-(-Hi // Ho) + 1) * (-(-Wi // Wo) + 1) >= 128
    assert {wave(c) for c in S.CASES['avgpool']} == {True, False}
    assert any(wave(c) and c[0] * c[2][0] * c[2][1] > 2048 * 4 for c in S.CASES['avgpool'])          # the wave kernel's grid-stride loop
    assert any(c[0] * c[2][0] * c[2][1] > 2048 * 256 for c in S.CASES['resize_bilinear'])
    assert any(3 * B * HW > 2048 * 256 for B, HW in S.CASES['align_head'])
    assert any(c[1] ** 2 > 1024 * 256 for c in S.CASES['mask_blend']) and any(c[0][-1] == c[1] for c in S.CASES['mask_blend'])
    assert any(c[0] > 64 * 256 for c in S.CASES['affine_apply']) and any(c[0] > 64 * 256 for c in S.CASES['align_input'])

    def quad(c):                    # fewout_quad && M == 3 && (!w11t || M2 == 3) && W % 4 == 0
        return c[2] == 3 and c[8] in (0, 3) and c[4] % 4 == 0
    assert {quad(c) for c in S.CASES['conv3x3_fewout2']} == {True, False}


# ------------------------------------------------------------------ (b) the kernels (GPU)
@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


def run_hip(op, inp, dev):
    from oodgan import encoder_hip, samm

    def d(name):
        t = inp.get(name)
        return None if t is None else t.to(dev)

    if op == 'instnorm_stats':
        st = samm.instnorm_stats(d('x'))
        return st[..., 0], st[..., 1]
    if op == 'affine_apply_stats':
        y, st = samm.affine_apply_stats(d('x'), d('sc'), d('sh'), d('res'))
        return y, st[..., 0], st[..., 1]
    if op == 'align_input_stats':
        y, st = samm.align_input_stats(d('gen'), d('enc'), d('st_gen'), d('st_enc'), diff=bool(inp['diff']))
        return y, st[..., 0], st[..., 1]
    if op == 'affine_apply':
        return (samm.affine_apply(d('x'), d('sc'), d('sh'), d('res')),)
    if op == 'align_input':
        return (samm.align_input(d('gen'), d('enc'), d('st_gen'), d('st_enc'), diff=bool(inp['diff'])),)
    if op == 'instnorm_coeffs':
        return samm.instnorm_coeffs(d('stats'), d('gamma'), d('beta'))
    if op == 'conv1x1':
        return (samm.conv1x1(d('x'), d('w'), d('bias')),)
    if op == 'se_gate':
        return (samm.se_gate(d('stats'), d('w1'), d('w2')),)
    if op == 'conv3x3_small':
        return (samm.conv3x3_small(d('x'), d('w'), d('in_sc'), d('in_sh'), d('slope')),)
    if op == 'conv3x3_fewout':
        return (samm.conv3x3_fewout(d('x'), d('w'), d('in_sc'), d('in_sh'), d('slope')),)
    if op == 'conv3x3_fewout2':
        wt, w11t = samm.fewout_weights(d('w'), d('w11'))
        y, y2 = samm.conv3x3_fewout2(d('x'), wt, inp['w'].shape[0], d('in_sc'), d('in_sh'), slope=d('slope'), w11t=w11t,
                                     M2=inp['w11'].shape[0] if 'w11' in inp else 0)
        return (y,) if y2 is None else (y, y2)
    if op == 'align_head':
        return (samm.align_head(d('x'), inp['scale']),)
    if op == 'field_compose':
        if inp['mode'] == 0:
            return (samm.field_add(d('acc'), d('cur'), inp['scale']),)
        return (samm.field_upsample_add(d('prev'), d('cur')),)
    if op == 'warp_blend':
        return (samm.warp_blend(d('target'), d('field')),)
    if op == 'mask_blend':
        a, out = samm.mask_blend([f.to(dev) for f in inp['fields']], d('x'), d('gen'), size=inp['S'])
        return (a,) if out is None else (a, out)
    if op == 'resize_nearest':
        if 'extra' in inp:
            # out is a wider tensor: pitch and offset; the columns outside the written window stay as they were
            _, pitch, xoff = inp['extra']
            (Ho, Wo), x = inp['size'], d('x')
            out = torch.full(x.shape[:2] + (Ho, pitch), SENTINEL, device=dev)
            samm.resize_nearest(x, (Ho, Wo), out=out, xoff=xoff)
            outside = torch.ones(pitch, dtype=torch.bool, device=dev)
            outside[xoff:xoff + Wo] = False
            assert (out[..., outside] == SENTINEL).all(), 'resize_nearest wrote outside its window'
            return (out[..., xoff:xoff + Wo],)
        return (samm.resize_nearest(d('x'), inp['size']),)
    if op == 'resize_bilinear':
        return (samm.resize_bilinear(d('x'), inp['size']),)
    if op == 'resize_bicubic_ac':
        return (encoder_hip._resize_bicubic_ac(d('x'), inp['size'], add=d('add')),)
    if op == 'avgpool':
        return (samm.avgpool(d('x'), inp['size']),)
    raise KeyError(op)


def _check(op, case, dev, tag=''):
    inp = S.case_bundle(op, case)[0]
    ys = run_hip(op, inp, dev)
    torch.cuda.synchronize()
    r, b = S.measure(op, case, ys), bar(op, inp)
    print(f'SAMM_F64 {op}{tag} {S.case_id(case)} r={r:.4g} bar={b}')
    assert r <= b, f'{op}{tag} {S.case_id(case)}: r = {r:.4g} > bar {b}'
    return ys


def _make_op_test(op):
    @gpu
    @pytest.mark.parametrize('case', S.CASES[op], ids=_ids(op))
    def test(dev, case):
        _check(op, case, dev)
    test.__name__ = test.__qualname__ = f'test_{op}_vs_float64'
    test.__doc__ = f'oodgan.samm {op}: r <= bar against the float64 reference on every case of samm_ref.CASES[{op!r}].'
    return test


for _op in S.OPS:
    if _op != 'conv3x3_fewout2':
        globals()[f'test_{_op}_vs_float64'] = _make_op_test(_op)


@gpu
@pytest.mark.parametrize('case', S.CASES['conv3x3_fewout2'], ids=_ids('conv3x3_fewout2'))
def test_fewout2_quad_settings(dev, tunable, case):
    """conv3x3_fewout2 under fewout_quad = 1 and 0, each against float64.  Where the quad form cannot run (M != 3, M2 not in (0, 3) or
    W % 4 != 0) both settings are the same kernel and bit-equal.  Where it runs, the two forms sum in different orders (per wave two of a
    stage's eight channels, the four waves added at the end, against one accumulator walking all eight): they are NOT bit-equal — no
    comment in samm.hip claims it — and each setting is held to the bar."""
    out = {}
    for q in (1, 0):
        tunable('fewout_quad', q)
        out[q] = _check('conv3x3_fewout2', case, dev, f'[quad={q}]')
    same = all(torch.equal(a, b) for a, b in zip(out[0], out[1]))
    quad_runs = case[2] == 3 and case[8] in (0, 3) and case[4] % 4 == 0
    print(f'SAMM_F64 fewout_quad 0 vs 1 {S.case_id(case)}: quad form runs: {quad_runs}, bit-equal: {same}')
    if not quad_runs:
        assert same


@gpu
def test_conv1x1_rows_of_the_wide_form_equal_the_narrow_form(dev):
    """Both forms add the products in the order of k into one accumulator per output ("same results", samm.hip): every row of the batch of
    eight, which takes the wide form, is bit-equal to the same image alone, which takes the narrow one."""
    from oodgan import samm
    case = (8, 33, 65, 16129)
    inp = S.case_bundle('conv1x1', case)[0]
    x, w, b = inp['x'].to(dev), inp['w'].to(dev), inp['bias'].to(dev)
    y = samm.conv1x1(x, w, b)
    for k in range(8):
        assert torch.equal(y[k:k + 1], samm.conv1x1(x[k:k + 1].contiguous(), w, b)), f'row {k}'


@gpu
@pytest.mark.parametrize('HW', S.STAT_HW)
def test_fused_statistics_equal_two_passes(dev, HW):
    """affine_apply_stats / align_input_stats are bit-identical to affine_apply / align_input followed by instnorm_stats, on both the
    float4 and the scalar path and across the trip boundary (HW = 4096, 4099, 4100), with and without res, diff 0 and 1."""
    from oodgan import samm
    for res in (False, True):
        inp = S.case_bundle('affine_apply_stats', (HW, False, res))[0]
        x, sc, sh = inp['x'].to(dev), inp['sc'].to(dev), inp['sh'].to(dev)
        r = None if inp['res'] is None else inp['res'].to(dev)
        y0 = samm.affine_apply(x, sc, sh, r)
        y1, st1 = samm.affine_apply_stats(x, sc, sh, r)
        assert torch.equal(y0, y1) and torch.equal(samm.instnorm_stats(y0), st1)
    for diff in (0, 1):
        inp = S.case_bundle('align_input_stats', (HW, False, diff))[0]
        g, e, sg, se = (inp[k].to(dev) for k in ('gen', 'enc', 'st_gen', 'st_enc'))
        a0 = samm.align_input(g, e, sg, se, diff=bool(diff))
        a1, st1 = samm.align_input_stats(g, e, sg, se, diff=bool(diff))
        assert torch.equal(a0, a1) and torch.equal(samm.instnorm_stats(a0), st1)


# ------------------------------------------------------------------ refusals
@pytest.fixture
def outputs(monkeypatch):
    """Every tensor the wrappers allocate for their results while the test runs, pre-filled with a sentinel."""
    made = []
    real = {'empty': torch.empty, 'empty_like': torch.empty_like}

    def wrap(name):
        def alloc(*a, **k):
            t = real[name](*a, **k)
            t.fill_(SENTINEL)
            made.append(t)
            return t
        return alloc

    for name in real:
        monkeypatch.setattr(torch, name, wrap(name))
    return made


def _refused(call, outputs, exc=RuntimeError, allocates=True):
    """The wrapper raises, and what it had allocated for the result is untouched: a refusal returns before any launch."""
    del outputs[:]
    with pytest.raises(exc):
        call()
    torch.cuda.synchronize()
    assert bool(outputs) == allocates
    assert all((t == SENTINEL).all() for t in outputs)


@gpu
def test_refusals_leave_the_output_untouched(dev, outputs):
    from oodgan import samm
    n = lambda *shape: S.normal(shape, 5).to(dev)
    # affine_apply / align_input: the planes are grid.y, B * C <= 65535
    x = n(1, 65536, 1, 1)
    _refused(lambda: samm.affine_apply(x, n(1, 65536), n(1, 65536)), outputs)
    _refused(lambda: samm.align_input(x, x, n(1, 65536, 2), n(1, 65536, 2)), outputs)
    # se_gate: C <= 1024 (the means in LDS), Cr <= 64
    _refused(lambda: samm.se_gate(n(3, 1025, 2), n(8, 1025), n(1025, 8)), outputs)
    _refused(lambda: samm.se_gate(n(3, 64, 2), n(65, 64), n(64, 65)), outputs)
    # conv3x3_small: K <= 8 && M <= 8
    _refused(lambda: samm.conv3x3_small(n(1, 9, 5, 5), n(3, 9, 3, 3)), outputs)
    _refused(lambda: samm.conv3x3_small(n(1, 3, 5, 5), n(9, 3, 3, 3)), outputs)
    # few-output convs: M <= 4; the prepared-weight form K % 8 == 0
    _refused(lambda: samm.conv3x3_fewout(n(1, 16, 5, 5), n(5, 16, 3, 3)), outputs)
    wt = torch.zeros(12, 9, 4, device=dev)
    _refused(lambda: samm.conv3x3_fewout2(n(1, 12, 5, 5), wt, 3), outputs)
    wt16 = torch.zeros(16, 9, 4, device=dev)
    _refused(lambda: samm.conv3x3_fewout2(n(1, 16, 5, 5), wt16, 5), outputs)
    # mask_blend: 1 .. 4 fields; out needs x and gen
    f = [n(1, 3, s, s) for s in (4, 8, 16, 32, 64)]
    _refused(lambda: samm.mask_blend([], size=64), outputs, (RuntimeError, IndexError), allocates=False)
    _refused(lambda: samm.mask_blend(f, size=128), outputs)
    _refused(lambda: samm.mask_blend(f[:2], gen=n(1, 3, 64, 64), size=64), outputs)
    # avgpool: Hout <= Hin
    _refused(lambda: samm.avgpool(n(1, 2, 4, 8), (5, 3)), outputs)
