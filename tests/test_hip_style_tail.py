"""The style, backward-tail and range-scale kernels (csrc/style.hip, csrc/bwd_tail.hip, csrc/fwd_range.hip, the reduction and abs-max kernels
of csrc/elementwise.hip and csrc/bwd_producers.hip) one by one against the float64 references of tests/tail_ref.py, at the smallest shapes
that reach each branch of their loops.

Exact where possible.  The data are small integers (values in [-4, 4]; powers of two for scale, scale2, d and q), so every float32 product and
sum is exact in any order and the comparison with float64 is torch.equal (tests/test_tail_ref_cpu.py checks that the sets are in that
regime).  A tolerance appears in three places only, each derived from the number format:
  * rsqrt of the demodulation: 2^-22 relative (two float32 roundings + a 1-ulp rsqrtf), the accumulator being exact;
  * style_affine with 1/sqrt(S) not a power of two (S = 80, 33, 100): 3 * 2^-24 * (|acc*scale| + |bias*lr_mul|) per element (the scale's
    conversion to float and the two roundings of the epilogue);
  * one random-normal set per reduction kernel: depth * 2^-24 * sum_j |p_j|, depth = the longest chain of additions an element passes
    through (depth16 / depth_wave / depth_cols below, beside the lines of code they come from).
Observed maxima on the MI355X are recorded in LABNOTES.md."""
import ctypes
import math

import pytest
import torch

import tail_ref as T

pytestmark = pytest.mark.gpu

F64 = torch.float64
SENT = -12345.0
U = T.U


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
    """device pointer to float / int32 element ``off`` of t"""
    return ctypes.c_void_p(t.data_ptr() + 4 * off)


def host(t):
    return t.detach().cpu()


def eq64(out, ref64):
    """the float32 device result equals the float64 reference exactly"""
    return torch.equal(host(out).to(F64), ref64)


def block_in(dev, dense, stride, off, fill=SENT):
    """a (B, stride) device matrix filled with ``fill`` whose columns [off, off+n) hold ``dense`` (B, n)"""
    m = torch.full((dense.shape[0], stride), fill, dtype=torch.float32)
    m[:, off:off + dense.shape[1]] = dense
    return m.to(dev)


def outside_untouched(mat, off, n, fill=SENT):
    m = host(mat).clone()
    m[:, off:off + n] = fill
    return bool((m == fill).all())


# ----------------------------------------------------------------------------- data (CPU; shared with tests/test_tail_ref_cpu.py)
SA_L = 3


def sa_data(B, S, R):
    """integer latent (B, 3, S), weights (R, S), bias (R,): slices of one set per S"""
    return T.ints((33, SA_L, S), 1000 + S)[:B].contiguous(), T.ints((1100, S), 2000 + S)[:R].contiguous(), T.ints((1100,), 3000 + S)[:R].contiguous()


def sa_uniform_row_lat(R):
    return [(2 * t + 1) % SA_L for t in range(R // 16) for _ in range(16)]


SAB_R, SAB_L, SAB_START = 1100, 4, [0, 16, 16, 1056, 1100]


def sab_data(B, S):
    return T.ints((17, SAB_R), 4000)[:B].contiguous(), T.ints((SAB_R, S), 2000 + S)


def demod_data(B, Ci, Co):
    """s (B,Ci) integers, wsq (Co,Ci) integers in [0,4], d (B,Co) powers of two, r (B,Co) integers, gs0 (B,Ci) non-zero integers"""
    s = T.ints((3, 1030), 5000)[:B, :Ci].contiguous()
    wsq = T.ints((1030, 1030), 5001, 0, 4)[:Co, :Ci].contiguous()
    d = T.pow2((3, 1030), 5002, -1, 1)[:B, :Co].contiguous()
    r = T.ints((3, 1030), 5003)[:B, :Co].contiguous()
    gs0 = T.ints((3, 1030), 5004, 1, 4)[:B, :Ci].contiguous()
    return s, wsq, d, r, gs0


DEMOD_SCALE = 0.125          # a power of two
RED_NPARTS = [1, 15, 16, 17, 63, 64, 65, 511, 512, 513, 1000]
RED_BC = [(1, 1), (1, 3), (2, 2), (1, 5), (2, 65)]          # B*C = 1, 3, 4, 5, 130: the row % 4 edges of the four-rows-per-wave path


def red_data(B, C, n, seed=0):
    return T.ints((2, 65, 1000), 6000 + seed)[:B, :C, :n].contiguous()


# (nparts, nparts2): the second operand on the other side of 64, in both directions, and both short (quad with a second operand)
RED_SECOND = [(15, 513), (513, 15), (64, 65), (65, 64), (17, 63)]


def exact_term_sets():
    """name -> (..., n) float32 products that a kernel sums, for the largest case of every exact comparison below"""
    out = {}

    def put(name, t64):
        t32 = t64.to(torch.float32)
        assert torch.equal(t32.to(F64), t64), name          # every product is itself a float32 number
        out[name] = t32

    for S in (16, 64, 256):
        lat, w, _ = sa_data(33, S, 80)
        put(f'style_affine S={S}', lat.to(F64)[:, sa_uniform_row_lat(80), :] * w.to(F64))
    for S in (64, 256):
        gs, w = sab_data(17, S)
        put(f'style_affine_bwd S={S}', gs.to(F64)[:, None, 16:1056] * w.to(F64).t()[None, :, 16:1056])
    wt = T.ints((64, 32, 3, 3), 7001)
    put('weight_sqsum', (wt.to(F64) ** 2).reshape(64, 32, 9))
    s, wsq, d, r, _ = demod_data(3, 1030, 5)
    put('demod_fwd', (s.to(F64) ** 2)[:, None, :] * wsq.to(F64)[None])
    s, wsq, d, r, _ = demod_data(3, 130, 1030)
    put('demod_bwd', ((r * d * d).to(F64))[:, None, :] * wsq.to(F64).t()[None])
    put('reduce', red_data(2, 65, 1000).to(F64))
    put('reduce accumulate', torch.cat([T.ints((2, 65, 1), 6100).to(F64), red_data(2, 65, 1000).to(F64)], 2))
    sc2 = T.pow2((2, 65), 6200)
    put('reduce second operand', torch.cat([red_data(2, 65, 513).to(F64), sc2.to(F64)[..., None] * red_data(2, 65, 513, 1).to(F64)], 2))
    return out


# ----------------------------------------------------------------------------- style_affine forward
def _sa_check(dev, lat, w, bias, rl, lr_mul, tag):
    from oodgan import ops
    S = w.shape[1]
    out = ops.style_affine(lat.to(dev), w.to(dev), None if bias is None else bias.to(dev),
                           None if rl is None else torch.tensor(rl, dtype=torch.int32, device=dev), lr_mul)
    ref, bound = T.style_affine(lat, w, bias, rl, lr_mul)
    if S in (16, 64, 256):          # 1/sqrt(S) is a power of two: exact
        assert eq64(out, ref), tag
        return 0.0
    err = (host(out).to(F64) - ref).abs()
    assert (err <= 3 * U * bound).all(), (tag, (err / (U * bound).clamp_min(1e-300)).max().item())
    return (err / (U * bound).clamp_min(1e-300)).max().item()


@pytest.mark.parametrize('S', [16, 64, 80, 256])
def test_style_affine_mfma(dev, S):
    worst = 0.0
    for B in (1, 5, 16, 17, 33):
        for R in (16, 48, 80):          # 80: a partly filled last block of four tiles
            lat, w, bias = sa_data(B, S, R)
            rl = sa_uniform_row_lat(R)
            for rl_, bias_, lr_mul in [(rl, bias, 1.0), (None, bias, 0.5), (rl, None, 0.5), (None, None, 1.0)]:
                worst = max(worst, _sa_check(dev, lat, w, bias_, rl_, lr_mul, (B, R, S, rl_ is None, bias_ is None, lr_mul)))
    print(f'style_affine mfma S={S}: max err / (2^-24 bound) = {worst:.3f} (limit 3)')


@pytest.mark.parametrize('S', [33, 64, 100])
def test_style_affine_generic(dev, S):
    worst = 0.0
    for B in (1, 5, 17):
        for R in (17, 20):
            lat, w, bias = sa_data(B, S, R)
            rl = ([1] * 7 + [0] * 6 + [2] * 7)[:R]          # changes inside the first group of 16 rows
            for rl_, bias_, lr_mul in [(rl, bias, 1.0), (None, None, 0.5), (rl, None, 0.5)]:
                worst = max(worst, _sa_check(dev, lat, w, bias_, rl_, lr_mul, (B, R, S, rl_ is None, bias_ is None, lr_mul)))
    print(f'style_affine generic S={S}: max err / (2^-24 bound) = {worst:.3f} (limit 3)')


MIXED = [(32, [0] * 8 + [1] * 24), (48, [2] * 20 + [0] * 28)]


@pytest.mark.parametrize('R,rl', MIXED, ids=['R32', 'R48'])
def test_style_affine_mixed_tile(dev, R, rl):
    """R % 16 == 0 and S % 16 == 0 select the MFMA kernel; a tile whose 16 rows read two latents must still be right"""
    for B in (5, 17):
        for S in (64, 80):
            lat, w, bias = sa_data(B, S, R)
            _sa_check(dev, lat, w, bias, rl, 1.0, (B, R, S))
            _sa_check(dev, lat, w, None, rl, 0.5, (B, R, S))


def test_style_affine_mixed_tile_leaves_uniform_tiles_alone(dev):
    """random data: the uniform tiles of a launch that also holds a mixed tile equal, bit for bit, the same tiles of an all-uniform launch"""
    from oodgan import ops
    B, S, R = 17, 64, 48
    lat, w, bias = T.normal((B, SA_L, S), 11).to(dev), T.normal((R, S), 12).to(dev), T.normal((R,), 13).to(dev)
    mixed = torch.tensor([2] * 20 + [0] * 28, dtype=torch.int32, device=dev)          # tile 1 is mixed; tiles 0 and 2 are uniform
    unif = torch.tensor([2] * 16 + [1] * 16 + [0] * 16, dtype=torch.int32, device=dev)
    a, b = host(ops.style_affine(lat, w, bias, mixed)), host(ops.style_affine(lat, w, bias, unif))
    assert torch.equal(a[:, :16], b[:, :16]) and torch.equal(a[:, 32:], b[:, 32:])
    ref, bound = T.style_affine(host(lat), host(w), host(bias), host(mixed).tolist())
    # a 64-term float32 dot product in any order: (64 + 2) * 2^-24 * sum of absolute values is the any-order worst case
    absacc = torch.einsum('brk,rk->br', host(lat).to(F64).abs()[:, host(mixed).long(), :], host(w).to(F64).abs()) / 8 + host(bias).to(F64).abs()
    assert ((a.to(F64) - ref).abs() <= 66 * U * absacc).all()


# ----------------------------------------------------------------------------- style_affine backward
@pytest.mark.parametrize('S', [64, 100, 256])
def test_style_affine_backward(dev, S):
    """R = 1100 rows over L = 4 latents: an empty latent (zeros must be WRITTEN), one of 1040 rows (two chunks of SAB_CHUNK = 1024, the second a
    16-row tail) and one of 44 rows (not a multiple of the 16 row groups); B crosses the 8-row batch tile"""
    from oodgan import ops
    worst = 0.0
    ls = torch.tensor(SAB_START, dtype=torch.int32, device=dev)
    for B in (1, 5, 8, 9, 17):
        gs, w = sab_data(B, S)
        gsd, wd = gs.to(dev), w.to(dev)
        for grad_div in (1.0, 4.0):
            ref = T.style_affine_backward(gs, w, SAB_START, SAB_L, 1.0, grad_div)
            glat = torch.full((B, SAB_L, S), SENT, device=dev)
            ck(lib().oodgan_style_affine_bwd(P(gsd), P(wd), P(ls), P(glat), B, SAB_L, S, SAB_R, (1.0 / math.sqrt(S)) / grad_div, stream()))
            outs = [glat]
            if B in (5, 17):
                outs.append(ops.style_affine_backward(gsd, wd, ls, SAB_L, 1.0, grad_div))
            for o in outs:
                assert torch.equal(host(o)[:, 1], torch.zeros(B, S)), (B, S, 'empty latent')
                if S in (64, 256):
                    assert eq64(o, ref), (B, S, grad_div)
                else:
                    err = (host(o).to(F64) - ref).abs()
                    assert (err <= 3 * U * ref.abs()).all(), (B, S, grad_div)
                    worst = max(worst, (err / (U * ref.abs()).clamp_min(1e-300)).max().item())
    print(f'style_affine_backward S={S}: max err / (2^-24 |ref|) = {worst:.3f} (limit 3)')


# ----------------------------------------------------------------------------- weight_sqsum, demod forward
@pytest.mark.parametrize('Co,Ci,k', [(5, 7, 3), (64, 32, 3), (3, 300, 1)])
def test_weight_sqsum(dev, Co, Ci, k):
    from oodgan import ops
    w = T.ints((Co, Ci, k, k), 7000 + k + Co)
    assert eq64(ops.weight_sqsum(w.to(dev)), T.weight_sqsum(w))


DF_CI = [1, 63, 64, 65, 511, 512, 513, 1030]          # the 64-lane and 512-per-trip edges of demod_dot
DF_CASES = [(B, Ci, Co) for Ci in DF_CI for Co in (1, 3, 5) for B in (1, 3)]
DS_PAD, DS_OFF, DD_PAD, DD_OFF = 7, 3, 5, 2          # s and d are column blocks of wider matrices


def _demod_fwd_case(dev, B, Ci, Co):
    s, wsq, _, _, _ = demod_data(B, Ci, Co)
    return dict(B=B, Ci=Ci, Co=Co, s=block_in(dev, s, Ci + DS_PAD, DS_OFF, 99.0), wsq=wsq.to(dev),
                d=torch.full((B, Co + DD_PAD), SENT, device=dev), ref=T.demod_fwd(s, wsq, DEMOD_SCALE))


def _demod_fwd_verify(c, tag):
    d = host(c['d'])[:, DD_OFF:DD_OFF + c['Co']].to(F64)
    rel = ((d - c['ref']).abs() / c['ref']).max().item()
    assert rel <= 2.0 ** -22, (tag, c['B'], c['Ci'], c['Co'], rel)
    assert outside_untouched(c['d'], DD_OFF, c['Co']), tag
    return rel


def test_demod_fwd_single_and_batch(dev):
    from oodgan import _lib, ops
    singles = [_demod_fwd_case(dev, *c) for c in DF_CASES]
    for c in singles:
        ck(lib().oodgan_demod_fwd(P(c['s'], DS_OFF), c['Ci'] + DS_PAD, P(c['wsq']), P(c['d'], DD_OFF), c['Co'] + DD_PAD, c['B'], c['Ci'], c['Co'],
                                  DEMOD_SCALE, stream()))
    worst = max(_demod_fwd_verify(c, 'single') for c in singles)
    # 37 jobs of mixed sizes in one call: two launches (kMaxDemod = 36)
    order = [(7 * i) % len(DF_CASES) for i in range(37)]
    assert len(set(order)) == 37
    batch = [_demod_fwd_case(dev, *DF_CASES[i]) for i in order]
    jobs = (_lib.DemodFwdJob * 37)(*[_lib.DemodFwdJob(P(c['s'], DS_OFF), P(c['wsq']), P(c['d'], DD_OFF), c['Ci'] + DS_PAD, c['Co'] + DD_PAD, c['B'], c['Ci'],
                                                     c['Co'], DEMOD_SCALE) for c in batch])
    ck(lib().oodgan_demod_fwd_batch(jobs, 37, stream()))
    for i, c in zip(order, batch):
        _demod_fwd_verify(c, 'batch')
        assert torch.equal(host(c['d']), host(singles[i]['d'])), ('batch != single', DF_CASES[i])          # both call demod_dot
    # the dense wrapper
    s, wsq, _, _, _ = demod_data(3, 513, 5)
    assert torch.equal(host(ops.demod(s.to(dev), wsq.to(dev), DEMOD_SCALE)), host(singles[DF_CASES.index((3, 513, 5))]['d'])[:, DD_OFF:DD_OFF + 5])
    print(f'demod_fwd: max relative error = {worst / 2.0 ** -24:.3f} * 2^-24 (limit 4)')


# ----------------------------------------------------------------------------- demod backward
DB_CASES = [(B, Ci, Co) for Ci in (1, 63, 64, 65, 130) for Co in (1, 3, 4, 5, 1024, 1030) for B in (1, 3)]
GS_PAD, GS_OFF = 6, 3


def _demod_bwd_case(dev, B, Ci, Co, random=False):
    if random:
        s, wsq, d, r, gs0 = (T.normal((B, Ci), 1), T.normal((Co, Ci), 2) ** 2, T.normal((B, Co), 3).abs() + 0.1, T.normal((B, Co), 4), T.normal((B, Ci), 5))
    else:
        s, wsq, d, r, gs0 = demod_data(B, Ci, Co)
    return dict(B=B, Ci=Ci, Co=Co, s=block_in(dev, s, Ci + DS_PAD, DS_OFF, 99.0), wsq=wsq.to(dev), d=block_in(dev, d, Co + DD_PAD, DD_OFF, 99.0),
                r=r.to(dev), gs=block_in(dev, gs0, Ci + GS_PAD, GS_OFF), gs0=gs0, ref=gs0.to(F64) + T.demod_bwd(s, wsq, d, r, DEMOD_SCALE))


def _demod_bwd_single(c):
    ck(lib().oodgan_demod_bwd(P(c['s'], DS_OFF), c['Ci'] + DS_PAD, P(c['wsq']), P(c['d'], DD_OFF), c['Co'] + DD_PAD, P(c['r']), P(c['gs'], GS_OFF),
                              c['Ci'] + GS_PAD, c['B'], c['Ci'], c['Co'], DEMOD_SCALE, stream()))


def _demod_bwd_batch(cases):
    from oodgan import _lib
    n = len(cases)
    jobs = (_lib.DemodBwdJob * n)(*[_lib.DemodBwdJob(P(c['s'], DS_OFF), P(c['wsq']), P(c['d'], DD_OFF), P(c['r']), P(c['gs'], GS_OFF), c['Ci'] + DS_PAD,
                                                    c['Co'] + DD_PAD, c['Ci'] + GS_PAD, c['B'], c['Ci'], c['Co'], DEMOD_SCALE) for c in cases])
    ck(lib().oodgan_demod_bwd_batch(jobs, n, stream()))


def _demod_bwd_verify(c, tag):
    assert eq64(c['gs'][:, GS_OFF:GS_OFF + c['Ci']], c['ref']), (tag, c['B'], c['Ci'], c['Co'])          # gs accumulates: prefilled non-zero
    assert outside_untouched(c['gs'], GS_OFF, c['Ci']), tag


def test_demod_bwd_single_and_batch(dev):
    singles = [_demod_bwd_case(dev, *c) for c in DB_CASES]
    for c in singles:
        _demod_bwd_single(c)
        _demod_bwd_verify(c, 'single')
    order = [(7 * i + 3) % len(DB_CASES) for i in range(37)]          # 37 jobs: two launches (kMaxDemod = 36); Co > 1024 among them
    assert len(set(order)) == 37 and any(DB_CASES[i][2] == 1030 for i in order)
    batch = [_demod_bwd_case(dev, *DB_CASES[i]) for i in order]
    _demod_bwd_batch(batch)
    for i, c in zip(order, batch):
        _demod_bwd_verify(c, 'batch')
        assert torch.equal(host(c['gs']), host(singles[i]['gs']))


def test_demod_bwd_batch_equals_single_on_random_data(dev):
    order = [(7 * i + 3) % len(DB_CASES) for i in range(37)]
    singles = [_demod_bwd_case(dev, *DB_CASES[i], random=True) for i in order]
    batch = [_demod_bwd_case(dev, *DB_CASES[i], random=True) for i in order]
    for c in singles:
        _demod_bwd_single(c)
    _demod_bwd_batch(batch)
    for i, a, b in zip(order, singles, batch):
        assert torch.equal(host(a['gs']), host(b['gs'])), DB_CASES[i]
        assert outside_untouched(b['gs'], GS_OFF, b['Ci'])
        # the random case against float64, any-order bound: r*d*d is 2 roundings, the product with wsq 1, the Co-term sum at most Co - 1,
        # scale^2 * s * sum 2, the accumulation into gs 1: (Co + 5) * 2^-24 * (|gs0| + scale^2 |s| sum |r| d^2 wsq)
        s = host(a['s'])[:, DS_OFF:DS_OFF + a['Ci']].to(F64)
        d = host(a['d'])[:, DD_OFF:DD_OFF + a['Co']].to(F64)
        mag = a['gs0'].to(F64).abs() + DEMOD_SCALE ** 2 * s.abs() * ((host(a['r']).to(F64).abs() * d * d) @ host(a['wsq']).to(F64))
        assert ((host(a['gs'])[:, GS_OFF:GS_OFF + a['Ci']].to(F64) - a['ref']).abs() <= (a['Co'] + 5) * U * mag).all(), DB_CASES[i]


# ----------------------------------------------------------------------------- reductions
OUT_PAD, OUT_OFF = 5, 2


def depth16():
    # row_sum16 (common.hpp): `(v[0] + v[1]) + (v[2] + v[3])` is 2 additions, the four `r += __shfl_xor(r, ..)` are 4
    return 2 + 4


def depth_wave(n):
    # row_sum_wave (common.hpp): `a0 += v[0] + v[4]` is 2 additions in an element's first trip and 1 in each of the ceil(n/512) - 1 later trips,
    # `(a0 + a1) + (a2 + a3)` is 2, wave_sum's six `v += __shfl_xor(v, o, 64)` are 6
    return 2 + (-(-n // 512) - 1) + 2 + 6


def depth_rows(n):
    # row_sum (common.hpp): `n <= 64 ? row_sum16 : row_sum_wave`
    return depth16() if n <= 64 else depth_wave(n)


def depth_cols(n):
    # reduce_parts_cols_kernel (elementwise.hip): `for (j = lane; j < nparts; j += 64) s += p[j]` is ceil(n/64) additions, wave_sum 6
    return -(-n // 64) + 6


def _reduce_job(part, out, off, B, C, n, stride, acc, second=None):
    from oodgan import _lib
    j = _lib.ReduceJob(P(part), P(out, off), B, C, n, stride, acc)
    if second is not None:
        part2, scale2, s2off, s2stride = second
        j.part2, j.scale2, j.nparts2, j.scale2_stride = P(part2), P(scale2, s2off), part2.shape[2], s2stride
    return j


def _run_jobs(jobs):
    from oodgan import _lib
    ck(lib().oodgan_reduce_batch((_lib.ReduceJob * len(jobs))(*jobs), len(jobs), stream()))


def _red_out(dev, B, C, acc, seed):
    """(B, C + pad) output matrix: sentinels around the block; the block holds non-zero integers when the kernel accumulates, sentinels otherwise"""
    prev = T.ints((B, C), 6100 + seed, 1, 4)
    m = block_in(dev, prev, C + OUT_PAD, OUT_OFF) if acc else torch.full((B, C + OUT_PAD), SENT, device=dev)
    return m, prev.to(F64) if acc else torch.zeros(B, C, dtype=F64)


@pytest.mark.parametrize('acc', [0, 1])
def test_reductions_exact(dev, acc):
    """reduce_parts, reduce_parts_cols and reduce_batch on integer partials, every nparts x B*C; the batch is ONE call of 55 jobs (mixed 16-lane
    and whole-wave rows, two launches: kMaxReduce = 48)"""
    cases, jobs = [], []
    for n in RED_NPARTS:
        for B, C in RED_BC:
            part = red_data(B, C, n)
            ref, _ = T.reduce_rows(part)
            pd = part.to(dev)
            o_cols, prev = _red_out(dev, B, C, acc, 0)
            o_batch, _ = _red_out(dev, B, C, acc, 0)
            o_rows = prev.to(torch.float32).to(dev).contiguous() if acc else torch.full((B, C), SENT, device=dev)
            ck(lib().oodgan_reduce_parts(P(pd), P(o_rows), B * C, n, acc, stream()))
            ck(lib().oodgan_reduce_parts_cols(P(pd), P(o_cols, OUT_OFF), B, C, n, C + OUT_PAD, acc, stream()))
            jobs.append(_reduce_job(pd, o_batch, OUT_OFF, B, C, n, C + OUT_PAD, acc))
            cases.append((n, B, C, pd, ref + prev, o_rows, o_cols, o_batch))
    assert len(jobs) == 55
    _run_jobs(jobs)
    for n, B, C, _, ref, o_rows, o_cols, o_batch in cases:
        assert eq64(o_rows, ref), ('reduce_parts', n, B, C)
        for name, o in (('reduce_parts_cols', o_cols), ('reduce_batch', o_batch)):
            assert eq64(o[:, OUT_OFF:OUT_OFF + C], ref), (name, n, B, C)
            assert outside_untouched(o, OUT_OFF, C), (name, n, B, C)


@pytest.mark.parametrize('acc', [0, 1])
def test_reduce_batch_second_operand(dev, acc):
    """out (+)= sum part + scale2 * sum part2; nparts and nparts2 on either side of 64; scale2 a column block with its own stride"""
    S2_PAD, S2_OFF = 4, 1
    jobs, cases = [], []
    for n, n2 in RED_SECOND:
        for B, C in RED_BC:
            part, part2, sc2 = red_data(B, C, n), red_data(B, C, n2, 1), T.pow2((2, 65), 6200)[:B, :C].contiguous()
            ref, _ = T.reduce_rows(part, part2, sc2)
            out, prev = _red_out(dev, B, C, acc, 1)
            pd, p2d, s2d = part.to(dev), part2.to(dev), block_in(dev, sc2, C + S2_PAD, S2_OFF, 99.0)
            jobs.append(_reduce_job(pd, out, OUT_OFF, B, C, n, C + OUT_PAD, acc, (p2d, s2d, S2_OFF, C + S2_PAD)))
            cases.append((n, n2, B, C, ref + prev, out, pd, p2d, s2d))
    _run_jobs(jobs)
    for n, n2, B, C, ref, out, *_ in cases:
        assert eq64(out[:, OUT_OFF:OUT_OFF + C], ref), (n, n2, B, C)
        assert outside_untouched(out, OUT_OFF, C), (n, n2, B, C)


def test_reduce_batch_50_jobs_into_one_accumulator(dev):
    """one call of 50 jobs that alternates short (16-lane) and long (whole-wave) rows, two launches; the outputs are disjoint column blocks of
    one (B, R) accumulator, as the style-gradient accumulator of the W+ backward: the whole matrix is checked"""
    B = 2
    lens = [15, 513, 64, 65, 1, 1000, 63, 512, 17, 511]
    Cs = [1, 3, 4, 5, 7]
    blocks = [(lens[i % 10], Cs[i % 5]) for i in range(50)]
    R = sum(c for _, c in blocks) + 3          # three columns nobody owns
    prev = T.ints((B, R), 6300, 1, 4)
    acc_m = prev.to(dev)
    ref = prev.to(F64).clone()
    jobs, keep, off = [], [], 0
    for i, (n, C) in enumerate(blocks):
        part = red_data(B, C, n, i % 3)
        accumulate = i % 2
        s, _ = T.reduce_rows(part)
        ref[:, off:off + C] = s + (ref[:, off:off + C] if accumulate else 0.0)
        keep.append(part.to(dev))
        jobs.append(_reduce_job(keep[-1], acc_m, off, B, C, n, R, accumulate))
        off += C
    _run_jobs(jobs)
    assert eq64(acc_m, ref)


@pytest.mark.parametrize('acc', [0, 1])
def test_reductions_random(dev, acc):
    """one random-normal set per kernel and nparts, against float64 with the bound depth * 2^-24 * sum |p| (+1 addition when accumulating);
    reduce_batch == reduce_parts bit for bit at every nparts; reduce_parts_cols == both for nparts <= 16 only (another order beyond)"""
    B, C = 2, 65
    jobs, cases = [], []
    for n in RED_NPARTS:
        part = T.normal((B, C, n), 6400 + n)
        prev = T.normal((B, C), 6500 + n) if acc else torch.zeros(B, C)
        ref, mag = T.reduce_rows(part)
        ref, mag = ref + prev.to(F64), mag + prev.to(F64).abs()
        pd = part.to(dev)
        o_rows, o_cols, o_batch = prev.to(dev).contiguous(), block_in(dev, prev, C + OUT_PAD, OUT_OFF), block_in(dev, prev, C + OUT_PAD, OUT_OFF)
        ck(lib().oodgan_reduce_parts(P(pd), P(o_rows), B * C, n, acc, stream()))
        ck(lib().oodgan_reduce_parts_cols(P(pd), P(o_cols, OUT_OFF), B, C, n, C + OUT_PAD, acc, stream()))
        jobs.append(_reduce_job(pd, o_batch, OUT_OFF, B, C, n, C + OUT_PAD, acc))
        cases.append((n, pd, ref, mag, o_rows, o_cols, o_batch))
    _run_jobs(jobs)
    worst = {'reduce_parts': 0.0, 'reduce_batch': 0.0, 'reduce_parts_cols': 0.0}
    for n, _, ref, mag, o_rows, o_cols, o_batch in cases:
        rows, cols, batch = host(o_rows), host(o_cols)[:, OUT_OFF:OUT_OFF + C], host(o_batch)[:, OUT_OFF:OUT_OFF + C]
        assert torch.equal(batch, rows), ('reduce_batch != reduce_parts', n)
        if n <= 16:
            assert torch.equal(cols, rows), ('reduce_parts_cols != reduce_parts', n)
        for name, o, depth in (('reduce_parts', rows, depth_rows(n)), ('reduce_batch', batch, depth_rows(n)), ('reduce_parts_cols', cols, depth_cols(n))):
            r = ((o.to(F64) - ref).abs() / (U * mag)).max().item()
            worst[name] = max(worst[name], r / (depth + acc))
            assert r <= depth + acc, (name, n, r, depth + acc)
    print(f'reductions random acc={acc}: largest error / bound = {worst}')


# ----------------------------------------------------------------------------- abs-max
def _vmax_of(dev, x, s_mat, s_off, s_stride):
    B, C = x.shape[0], x.shape[1]
    vm = torch.zeros(B * 64, dtype=torch.int32, device=dev)
    ck(lib().oodgan_absmax_scaled(P(x), None if s_mat is None else P(s_mat, s_off), s_stride, P(vm), B, C, x.numel() // (B * C), stream()))
    return host(vm).view(torch.float32).view(B, 64).amax(1)


_X_FULL = {}


def _x_data(B, C, HW):
    """integer planes, a fresh copy of a slice of one (3, 70, 40000) set"""
    if 'x' not in _X_FULL:
        _X_FULL['x'] = T.ints((3, 70, 40000), 8000)
    return _X_FULL['x'][:B, :C, :HW].clone()


@pytest.mark.parametrize('HW', [5, 1023, 1024, 16384, 16388, 40000])          # 1023: scalar path; 16388, 40000: several chunks
def test_absmax_scaled_and_measure(dev, HW):
    from oodgan import ops
    for B in (1, 3):
        for C in (1, 3, 70):          # C = 70 with several chunks: blockIdx.x + blockIdx.y wraps the 64 slots
            x = _x_data(B, C, HW)
            s = T.normal((B, C), 8100 + C)
            # the largest |x| * |s| of sample b sits in a channel of its own; make it the LAST element of the tensor for the last sample
            x[B - 1, C - 1, HW - 1] = 9.0
            s[B - 1, C - 1] = 3.3
            ref = T.absmax_scaled(x, s)
            xd, sd = x.to(dev), block_in(dev, s, C + 4, 1, 1e6)
            assert torch.equal(_vmax_of(dev, xd, sd, 1, C + 4), ref), (B, C, HW)
            assert torch.equal(_vmax_of(dev, xd, None, 0, 0), T.absmax_scaled(x)), (B, C, HW, 'no scale')
            # FwdRange.measure: q[l] from the measurement; the other layer and the maxima buffer stay as they were
            fr = ops.FwdRange(2, B, 1, 1, None, None, dev)
            fr.measure(1, xd, ops.Cols(sd, 1, C))
            want = torch.tensor([2.0 ** T.range_exp(v) for v in ref.tolist()])
            assert torch.equal(host(fr.q[1]), want) and torch.equal(host(fr.q[0]), torch.ones(B)), (B, C, HW)
            assert int(host(fr.vm).abs().max()) == 0


@pytest.mark.parametrize('HW', [1023, 40000])
def test_absmax_position_and_nonfinite(dev, HW):
    B, C = 3, 3
    base = _x_data(B, C, HW)
    s = T.pow2((B, C), 8200)
    spots = {'first': (0, 0, 0), 'last': (B - 1, C - 1, HW - 1), 'mid': (1, 1, HW // 2)}
    if HW > 16384:
        spots.update({'chunk end': (1, 2, 16383), 'chunk start': (2, 0, 16384), 'chunk 2 end': (0, 1, 32767)})
    for name, (b, c, p) in spots.items():
        x = base.clone()
        x[b, c, p] = -100.0
        ref = T.absmax_scaled(x, s)
        assert ref[b] == 100.0 * s[b, c]
        assert torch.equal(_vmax_of(dev, x.to(dev), s.to(dev), 0, C), ref), (HW, name)
    for bad in (math.nan, math.inf, -math.inf):
        x = base.clone()
        x[B - 1, C - 1, HW - 1] = bad
        got = _vmax_of(dev, x.to(dev), s.to(dev), 0, C)
        assert torch.equal(got, T.absmax_scaled(x, s)) and math.isinf(got[B - 1]) and torch.isfinite(got[:B - 1]).all(), (HW, bad)


def test_absmax_large_plane(dev):
    """(1, 1, 4100, 4100): 16.8M values are more than 1024 chunks of 16384, so the chunk size is recomputed"""
    from oodgan import ops
    H = 4100
    x = T.ints((1, 1, H, H), 8300)
    chunk = ((H * H + 1023) // 1024 + 3) // 4 * 4
    assert (H * H + 16383) // 16384 > 1024 and chunk % 4 == 0
    xd = x.to(dev)
    flat = xd.view(-1)
    assert torch.equal(_vmax_of(dev, xd, None, 0, 0), torch.tensor([4.0]))
    for p, v in ((H * H - 1, 9.0), (chunk, 17.0), (2 * chunk - 1, 33.0)):          # the last element, the first and the last of a chunk
        flat[p] = v
        assert torch.equal(_vmax_of(dev, xd, None, 0, 0), torch.tensor([v])), p
    m2 = host(ops.absmax_mul2(xd))
    assert m2.tolist() == [2.0 ** -4, 2.0 ** 4]          # 33 * 16 = 528


def test_absmax_mul2(dev):
    from oodgan import ops
    # s = None with C > 1: the sample is flattened to one range of C * HW values
    x = T.normal((2, 9, 5000), 8400)
    x[1, 8, 4999] = 77.0          # the maximum is the last element
    e = T.range_exp(77.0)
    assert host(ops.absmax_mul2(x.to(dev))).tolist() == [2.0 ** -e, 2.0 ** e]
    # twice on the same stream and batch size; the second tensor has the SMALLER maximum: the slots were cleared in between
    y = T.normal((2, 3, 1023), 8401).clamp(-0.01, 0.01)
    y[0, 0, 0] = 0.011
    e2 = T.range_exp(torch.tensor(0.011, dtype=torch.float32).item())
    assert host(ops.absmax_mul2(y.to(dev))).tolist() == [2.0 ** -e2, 2.0 ** e2]
    # NaN / Inf in the last element: e = 0
    for bad in (math.nan, math.inf):
        z = x.clone()
        z[1, 8, 4999] = bad
        assert host(ops.absmax_mul2(z.to(dev))).tolist() == [1.0, 1.0]
        assert host(ops.absmax_mul2(y.to(dev))).tolist() == [2.0 ** -e2, 2.0 ** e2]          # and the slots are clean again
    assert host(ops.absmax_mul2(torch.zeros(2, 3, 8, device=dev))).tolist() == [1.0, 1.0]


# ----------------------------------------------------------------------------- FwdRange.update_exact / finish / plan
def _ulp(v, k):
    return (T.bits_of(v) + k).view(torch.float32).item()


def _finish(dev, L, B, m, q):
    """finish() on chosen maxima m (L*B,) and scales q (L*B,): each maximum in a slot of its own, smaller values in other slots"""
    from oodgan import ops
    n = L * B
    vm = torch.zeros(n, 64, dtype=torch.int32)
    for i in range(n):
        vm[i, (5 * i) % 64] = T.bits_of(m[i])
        vm[i, (5 * i + 9) % 64] = T.bits_of(m[i] / 3 if math.isfinite(m[i]) else 1.0)
    fr = ops.FwdRange(L, B, 1, 1, None, None, dev)
    fr.vm.copy_(vm.view(L, B, 64))
    fr.q.copy_(torch.tensor(q, dtype=torch.float32).view(L, B))
    fr.finish()
    want_q, want_flag = T.fwd_range_update(vm, torch.tensor(q, dtype=torch.float32), True)
    assert torch.equal(host(fr.q).view(-1), want_q)
    assert int(host(fr.vm).abs().max()) == 0
    assert int(fr.flag.item()) == want_flag
    assert fr.violated() == (want_flag != 0)
    return want_flag


@pytest.mark.parametrize('L,B', [(5, 3), (35, 8)], ids=['15', '280'])          # 280 entries: a second block of 256 threads
def test_fwd_range_finish(dev, L, B):
    n = L * B
    g = torch.Generator().manual_seed(n)
    base_m = (2.0 ** (torch.rand(n, generator=g) * 14.9)).to(torch.float32).tolist()          # inside [1, 2^15)
    base_q = T.pow2((n,), 8500 + n, -6, 6).tolist()
    assert _finish(dev, L, B, base_m, base_q) == 0
    probes = [(_ulp(1.0, -1), 1), (1.0, 0), (_ulp(1.0, 1), 0), (_ulp(32768.0, -1), 0), (32768.0, 1), (_ulp(32768.0, 1), 1), (math.inf, 2), (0.0, 0)]
    for where in (0, n - 1):
        for v, want in probes:
            m = list(base_m)
            m[where] = v
            assert _finish(dev, L, B, m, base_q) == want, (where, v)
    # bits 1 and 2 together; an all-zero entry gets q = 1 whatever it carried
    m = list(base_m)
    m[1], m[n - 2], m[2] = 0.5, math.inf, 0.0
    assert _finish(dev, L, B, m, base_q) == 3


def test_fwd_range_update_exact(dev):
    from oodgan import ops
    L, B = 3, 4
    fr = ops.FwdRange(L, B, 1, 1, None, None, dev)
    q0 = T.pow2((L, B), 8600, -3, 3)
    fr.q.copy_(q0)
    m = [0.0007, 3.0, 1000.0, 123456.0]
    vm = torch.full((L, B, 64), 0, dtype=torch.int32)
    vm[0, :, 1] = T.bits_of(5.0)
    for b in range(B):
        vm[1, b, 63 - b] = T.bits_of(m[b])
    fr.vm.copy_(vm)
    fr.update_exact(1)
    want, _ = T.fwd_range_update(vm[1], q0[1], False)          # exact mode: the maxima are true values, q is not consulted and no flag is set
    got = host(fr.q)
    assert torch.equal(got[1], want) and torch.equal(got[0], q0[0]) and torch.equal(got[2], q0[2])
    v = host(fr.vm)
    assert int(v[1].abs().max()) == 0 and torch.equal(v[0], vm[0])
    assert int(fr.flag.item()) == 0


def test_fwd_range_plan(dev):
    from oodgan import ops
    L, B, R, DR = 3, 2, 11, 7
    row_layer = torch.tensor([0, 0, -1, 1, 1, 1, -1, 2, 2, 0, 2], dtype=torch.int32)
    drow_layer = torch.tensor([2, -1, 1, 1, 0, 0, 2], dtype=torch.int32)
    fr = ops.FwdRange(L, B, R, DR, row_layer.to(dev), drow_layer.to(dev), dev)
    q = T.pow2((L, B), 8700, -5, 5)
    fr.q.copy_(q)
    s_all, d_all = T.ints((B, R), 8701), T.ints((B, DR), 8702)
    for row0, nrows, drow0, ndrows in [(0, None, 0, None), (3, 5, 2, 4), (0, 0, 6, 1), (10, 1, 0, 0), (2, 1, 1, 1)]:
        fr.s_sc.fill_(SENT)
        fr.d_sc.fill_(SENT)
        fr.plan(s_all.to(dev), d_all.to(dev), row0, nrows, drow0, ndrows)
        nr, ndr = R if nrows is None else nrows, DR if ndrows is None else ndrows
        ws, wd = T.fwd_range_plan(s_all, d_all, row_layer, drow_layer, q, torch.full((B, R), SENT), torch.full((B, DR), SENT), row0, nr, drow0, ndr)
        assert eq64(fr.s_sc, ws) and eq64(fr.d_sc, wd), (row0, nrows, drow0, ndrows)
    assert torch.equal(host(fr.q), q)


# ----------------------------------------------------------------------------- absmax_scale_check (single and batched)
SC_N = [1, 1023, 1024, 4095, 4096, 4097, 130000]


def _sc_parts():
    """(part, used scale) list: random values with the maximum at the last index for every n, then the probes"""
    out = []
    for i, n in enumerate(SC_N):
        p = T.normal((n,), 8800 + n).clamp(-3, 3)
        p[n - 1] = -(5.0 + i)
        out.append((p, 2.0 ** (i - 3)))
    n = 4097
    for v in (_ulp(2.0 ** -8, -1), 2.0 ** -8, _ulp(2.0 ** -8, 1), _ulp(32768.0, -1), 32768.0, _ulp(32768.0, 1)):
        for used in (1.0, 4.0):          # scaled maximum = v: part holds v / used (exact)
            p = torch.zeros(n)
            p[n - 1] = v / used
            out.append((p, used))
    p = T.normal((4097,), 8900).clamp(-3, 3)
    p[4096] = math.nan          # NaN at the last index: bit 2; the maximum is that of the rest
    out.append((p, 1.0))
    p = T.normal((1024,), 8901)
    p[1023] = math.inf
    out.append((p, 1.0))
    out.append((torch.zeros(4096), 8.0))          # all zeros: state {1, 1}, no flag
    return out


def test_absmax_scale_check_single_and_batch(dev):
    from oodgan import _lib, ops
    parts = _sc_parts()
    flags_single, states_single = [], []
    for p, used in parts:
        state = torch.tensor([1.0 / used, used], device=dev)
        flag = torch.zeros(1, dtype=torch.int32, device=dev)
        ops.absmax_scale_check(p.to(dev), state, flag)
        want_state, want_flag = T.scale_check(p, used)
        assert host(state).tolist() == list(want_state), (p.numel(), used, host(state).tolist(), want_state)
        assert int(flag.item()) == want_flag, (p.numel(), used, p[-1].item())
        flags_single.append(want_flag)
        states_single.append(host(state))
    assert set(flags_single) == {0, 1, 2}
    # 37 jobs in one call (two launches: kMaxCheck = 36) against 37 single calls
    order = [i % len(parts) for i in range(37)]
    for drop_flagged in (False, True):          # one batch with violations, one without (the flag must stay 0)
        sel = [i for i in order if not (drop_flagged and flags_single[i])]
        sel = (sel * 37)[:37]
        pd = [parts[i][0].to(dev) for i in sel]
        states = torch.tensor([[1.0 / parts[i][1], parts[i][1]] for i in sel], device=dev)
        flag = torch.zeros(1, dtype=torch.int32, device=dev)
        jobs = (_lib.ScaleCheckJob * 37)(*[_lib.ScaleCheckJob(P(pd[k]), pd[k].numel(), P(states, 2 * k)) for k in range(37)])
        ck(lib().oodgan_absmax_scale_check_batch(jobs, 37, P(flag), stream()))
        want = 0
        for k, i in enumerate(sel):
            assert torch.equal(host(states)[k], states_single[i]), (k, i)
            want |= flags_single[i]
        assert int(flag.item()) == want and (want == 0) == drop_flagged


# ----------------------------------------------------------------------------- the exponent contract, everywhere a scale is produced
def test_range_scale_contract(dev):
    """m = 2^k and one ulp either side, k in [-20, 20]: m * scale in [512, 1024), scale a power of two, unscale * scale == 1 — from
    fwd_range_update_kernel, absmax_scale_kernel, absmax_scale_check_kernel and scale_check_batch_kernel"""
    from oodgan import _lib
    m = T.contract_values()
    n = m.numel()
    assert n == 123
    md = m.to(dev)
    L = lib()
    got = {}
    # fwd_range_update, exact mode (flag = NULL) and carry mode with q = 1: each maximum in slot 7 of its entry
    for mode in ('exact', 'carry'):
        vm = torch.zeros(n, 64, dtype=torch.int32)
        vm[:, 7] = m.view(torch.int32)
        vmd, q = vm.to(dev), torch.ones(n, device=dev)
        flag = torch.zeros(1, dtype=torch.int32, device=dev)
        ck(L.oodgan_fwd_range_update(P(vmd), P(q), P(flag) if mode == 'carry' else None, n, stream()))
        got[f'fwd_range_update {mode}'] = (host(q), None)
    # absmax_scale / absmax_scale_clear: one element each
    for name, fn in (('absmax_scale', L.oodgan_absmax_scale), ('absmax_scale_clear', L.oodgan_absmax_scale_clear)):
        part, out2 = md.clone(), torch.zeros(n, 2, device=dev)
        for i in range(n):
            ck(fn(P(part, i), 1, P(out2, 2 * i), stream()))
        o = host(out2)
        got[name] = (o[:, 1], o[:, 0])
        if name.endswith('clear'):
            assert int(host(part).abs().max()) == 0
    # absmax_scale_check, one call per value, and absmax_scale_check_batch, one call of 123 jobs (four launches)
    state = torch.ones(n, 2, device=dev)
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    for i in range(n):
        ck(L.oodgan_absmax_scale_check(P(md, i), 1, P(state, 2 * i), P(flag), stream()))
    o = host(state)
    got['absmax_scale_check'] = (o[:, 1], o[:, 0])
    state = torch.ones(n, 2, device=dev)
    jobs = (_lib.ScaleCheckJob * n)(*[_lib.ScaleCheckJob(P(md, i), 1, P(state, 2 * i)) for i in range(n)])
    ck(L.oodgan_absmax_scale_check_batch(jobs, n, P(flag), stream()))
    o = host(state)
    got['absmax_scale_check_batch'] = (o[:, 1], o[:, 0])
    bad = {}
    for name, (scale, unscale) in got.items():
        ok = T.contract_ok(m, scale, unscale)
        if not ok.all():
            bad[name] = [(f'{v:.9g}', float(sc)) for v, sc, k in zip(m.tolist(), scale.tolist(), ok.tolist()) if not k]
    print('range-scale contract violations:', {k: len(v) for k, v in bad.items()} or 'none')
    assert not bad, bad
