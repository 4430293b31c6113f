"""float64 references, per-element error scales, cases and mutants of the SAMM / SAIM ops (csrc/samm.hip).  Plain torch, no GPU.

    ref(op, inp, dtype)   the operation as the reference project defines it, evaluated in ``dtype`` on the float32 inputs promoted
                          exactly: float64 is the reference, float32 is the band a correct float32 implementation lives in
    scale(op, inp)        float64 tensors A of the outputs' shapes: the same expression with every product and sum taken over absolute
                          values (``None`` for an output that is pure indexing and has to be bit-exact)
    r_value(y, ref, A)    max_e |y_e - ref_e| / (2^-24 * A_e); elements with A_e == 0 must be equal, else inf
    CASES / MUTANTS       the shapes that cross every branch of the kernels, and deliberately wrong float32 evaluations that the inputs
                          must expose (tests/test_hip_samm_f64.py)

Every op returns a tuple of tensors.  Scales that are not a plain sum of products carry their derivation in the docstring of their function;
none of them is fitted to a kernel's output."""
import functools
import math

import torch
import torch.nn.functional as F

from oracle import ref_cpu as R

U = 2.0 ** -24                   # unit roundoff of float32
TINY = 2.0 ** -126               # smallest normal float32
F32, F64 = torch.float32, torch.float64
EPS = float(torch.tensor(1e-5, dtype=F32))        # the eps the kernels receive (a float argument)
INF = float('inf')


# ------------------------------------------------------------------------------------------------------------ data
def _gen(seed):
    g = torch.Generator()
    g.manual_seed(seed)
    return g


def normal(shape, seed, std=1.0, mean=0.0):
    return (torch.randn(shape, generator=_gen(seed), dtype=F64) * std + mean).float()


def uniform(shape, seed, lo=0.0, hi=1.0):
    return (torch.rand(shape, generator=_gen(seed), dtype=F64) * (hi - lo) + lo).float()


def outlier_positions(HW):
    """Where the loops over a plane change trips: first and last element, 1024k - 1, 1024k (a trip of 4 x 256 float4 is 4096 floats, a
    float4 trip of the 256 threads 1024 floats), 4096k - 1, 4096k."""
    pos = {0, HW - 1}
    for base in range(1024, HW + 1, 1024):
        pos.update(p for p in (base - 1, base) if 0 <= p < HW)
    return sorted(pos)


def planes(BC, HW, seed, mean=100.0, std=0.1):
    """(BC, HW) planes with |mean| = 1000 std, and a distinct outlier of 4 .. 14 at every position of ``outlier_positions``."""
    x = normal((BC, HW), seed, std, mean)
    for j, p in enumerate(outlier_positions(HW)):
        for bc in range(BC):
            x[bc, p] = mean + (-1) ** (j + bc) * (4.0 + (j % 10) + 0.5 * bc)
    return x


def chunk_outliers(w, dim, chunks=(8, 32, 64)):
    """Weights 8 times larger at the last tap of each K chunk, one past it, and at the last channel."""
    K = w.shape[dim]
    ks = {K - 1}
    for c in chunks:
        ks.update(k for k in (c - 1, c) if k < K)
    idx = torch.tensor(sorted(ks))
    w.index_copy_(dim, idx, w.index_select(dim, idx) * 8.0)
    return w


# ------------------------------------------------------------------------------------------------------------ metric
def r_value(ys, refs, As):
    worst = 0.0
    assert len(ys) == len(refs) == len(As)
    for y, ref, A in zip(ys, refs, As):
        assert y.shape == ref.shape, (y.shape, ref.shape)
        y, ref = y.detach().cpu().double(), ref.double()
        if A is None:
            if not torch.equal(y, ref):
                return INF
            continue
        assert A.shape == ref.shape, (A.shape, ref.shape)
        d = (y - ref).abs()
        if not torch.isfinite(d).all():
            return INF
        zero = A == 0
        if (d[zero] != 0).any():
            return INF
        if (~zero).any():
            worst = max(worst, (d[~zero] / (U * A[~zero])).max().item())
    return worst


def measure(op, case, ys):
    """r of the outputs ``ys`` of ``op`` on ``case``.  The fused passes return the statistics OF THE TENSOR THEY STORED (a float32 tensor): their
    reference is the float64 statistics of ys[0] itself, so the rounding of y does not blur what the statistics loops are held to."""
    inp, refs, As = case_bundle(op, case)
    if op in ('affine_apply_stats', 'align_input_stats'):
        y0 = ys[0].detach().cpu().double()
        refs = (refs[0],) + _stats(y0, F64)
        As = (As[0],) + _stats_scale(y0, y0.abs(), False)
    return r_value(ys, refs, As)


def pow2ceil(v):
    return 2.0 ** math.ceil(math.log2(v)) if v > 0 else 0.0


# ------------------------------------------------------------------------------------------------------------ statistics
def _stats(y, dtype):
    var, mean = torch.var_mean(y.to(dtype), dim=(2, 3), unbiased=False)
    return mean, (var + EPS) ** -0.5


def _stats_scale(y64, Ay, rounded_input):
    """mean: mean(A_y).

    rstd = (var + eps)^-1/2: relative error, so A = rstd * (1 + t).  The mean enters through t.  With the computed mean m' = m + d,
    sum (y - m')^2 = N var + N d^2 (the cross term vanishes: sum (y - m) = 0), so a float32 mean, |d| <= u mean|y|, moves var by d^2 and
    rstd by the relative amount d^2 rstd^2 / 2 <= u * (u (mean|y| rstd)^2 / 2): t2 = u (mean|y| rstd)^2 (second order: 6e-2 at
    |mean| = 1000 std, but 60 on a constant plane of value 100, where var + eps = eps).  Where the statistics are those of a tensor the same
    pass has just rounded to float32 (``rounded_input``: the fused kernels), every element carries its own error e_i, |e_i| <= u A_i,
    and var moves by 2 mean((y - m) e) <= 2 u mean(A) / rstd at first order: t1 = mean(A_y) rstd — the u |mean| rstd of a float32 mean."""
    mean64, rstd64 = _stats(y64, F64)
    Am = Ay.mean(dim=(2, 3))
    t = U * (Am * rstd64) ** 2
    if rounded_input:
        t = t + Am * rstd64
    return Am, rstd64 * (1.0 + t)


def _stat_mutants(make_y):
    """make_y(inp) -> the float32 tensor whose statistics the op returns, and the outputs in front of them."""
    def one_pass(inp):
        pre, y = make_y(inp)
        mean = y.mean(dim=(2, 3))
        var = (y * y).mean(dim=(2, 3)) - mean * mean
        return pre + (mean, (var.clamp_min(0) + EPS) ** -0.5)

    def drop_last(inp):
        pre, y = make_y(inp)
        HW = y.shape[2] * y.shape[3]
        yf = y.flatten(2)
        if HW == 1:
            return pre + _stats(y, F32)
        mean = yf[..., :-1].sum(-1) / HW
        var = ((yf[..., :-1] - mean[..., None]) ** 2).sum(-1) / HW
        return pre + (mean, (var + EPS) ** -0.5)

    def dup_1024(inp):
        pre, y = make_y(inp)
        yf = y.flatten(2)
        HW = yf.shape[-1]
        if HW <= 1024:
            return pre + _stats(y, F32)
        mean = (yf.sum(-1) + yf[..., 1024]) / HW
        var = (((yf - mean[..., None]) ** 2).sum(-1) + (yf[..., 1024] - mean) ** 2) / HW
        return pre + (mean, (var + EPS) ** -0.5)

    return {'one-pass variance': one_pass, 'last element dropped': drop_last, 'element 4*256 counted twice': dup_1024}


STAT_HW = (1, 3, 255, 1024, 1028, 4096, 4099, 4100)      # (HW & 3) == 0 vector path / scalar path; < 256; one and two trips of 4096


def _bc(t):
    return t[:, :, None, None]


def _in_stats(case):
    HW, const = case
    x = planes(6, HW, 100 + HW).reshape(2, 3, 1, HW)
    if const:
        x[0, 0] = float(torch.tensor(100.1, dtype=F32))
    return {'x': x}


def _ref_stats(inp, dtype):
    return _stats(inp['x'], dtype)


def _scale_stats(inp):
    x = inp['x'].double()
    return _stats_scale(x, x.abs(), False)


def _in_affine(case):
    HW, const, res = case
    inp = _in_stats((HW, const))
    inp['sc'], inp['sh'] = normal((2, 3), 7, 0.2, 1.0), normal((2, 3), 8, 0.3)
    inp['res'] = normal((2, 3, 1, HW), 9) if res else None
    return inp


def _affine(inp, dtype):
    y = inp['x'].to(dtype) * _bc(inp['sc'].to(dtype)) + _bc(inp['sh'].to(dtype))
    return y if inp['res'] is None else y + inp['res'].to(dtype)


def _affine_abs(inp):
    A = inp['x'].double().abs() * _bc(inp['sc'].double().abs()) + _bc(inp['sh'].double().abs())
    return A if inp['res'] is None else A + inp['res'].double().abs()


def _ref_affine_stats(inp, dtype):
    y = _affine(inp, dtype)
    return (y,) + _stats(y, dtype)


def _scale_affine_stats(inp):
    A = _affine_abs(inp)
    return (A,) + _stats_scale(_affine(inp, F64), A, True)         # see ``measure``: the tests rebase these on the stored y


def _in_align(case):
    HW, const, diff = case
    g = planes(6, HW, 200 + HW).reshape(2, 3, 1, HW)
    e = planes(6, HW, 300 + HW, mean=-40.0, std=0.5).reshape(2, 3, 1, HW)
    if const:
        g[0, 0] = float(torch.tensor(100.1, dtype=F32))
    return {'gen': g, 'enc': e, 'diff': diff, 'st_gen': torch.stack(_stats(g, F64), -1).float(), 'st_enc': torch.stack(_stats(e, F64), -1).float()}


def _align(inp, dtype, diff=None):
    diff = inp['diff'] if diff is None else diff
    sg, se = inp['st_gen'].to(dtype), inp['st_enc'].to(dtype)
    e = (inp['enc'].to(dtype) - _bc(se[..., 0])) * _bc(se[..., 1])
    g = (inp['gen'].to(dtype) - _bc(sg[..., 0])) * _bc(sg[..., 1])
    return torch.cat([g - e if diff else g, e], dim=1)


def _align_abs(inp):
    sg, se = inp['st_gen'].double().abs(), inp['st_enc'].double().abs()
    e = (inp['enc'].double().abs() + _bc(se[..., 0])) * _bc(se[..., 1])
    g = (inp['gen'].double().abs() + _bc(sg[..., 0])) * _bc(sg[..., 1])
    return torch.cat([g + e if inp['diff'] else g, e], dim=1)


def _ref_align_stats(inp, dtype):
    y = _align(inp, dtype)
    return (y,) + _stats(y, dtype)


def _scale_align_stats(inp):
    A = _align_abs(inp)
    return (A,) + _stats_scale(_align(inp, F64), A, True)


def _zero_last(y):
    y = y.clone()
    y.flatten()[-1] = 0.0
    return y


def _in_coeffs(case):
    gamma, beta = case
    C = 257                                       # one full block of 256 threads and one thread of the second
    return {'stats': torch.stack([normal((1, C), 11, 30.0, 5.0), uniform((1, C), 12, 0.5, 10.0)], -1),
            'gamma': normal((C,), 13, 0.3, 1.0) if gamma else None, 'beta': normal((C,), 14, 2.0) if beta else None}


def _ref_coeffs(inp, dtype, use_gamma=True, use_beta=True, roll=False):
    st = inp['stats'].to(dtype)
    sc = st[..., 1].clone()
    if inp['gamma'] is not None and use_gamma:
        g = inp['gamma'].to(dtype)
        sc = sc * (torch.cat([g[:-1], g[-2:-1]]) if roll else g)
    sh = -st[..., 0] * sc
    if inp['beta'] is not None and use_beta:
        sh = inp['beta'].to(dtype) + sh
    return sc, sh


def _scale_coeffs(inp):
    st = inp['stats'].double().abs()
    sc = st[..., 1] * (1.0 if inp['gamma'] is None else inp['gamma'].double().abs())
    sh = st[..., 0] * sc + (0.0 if inp['beta'] is None else inp['beta'].double().abs())
    return sc, sh


# ------------------------------------------------------------------------------------------------------------ convs
def _in_conv1x1(case):
    B, K, M, HW = case
    return {'x': normal((B, K, 1, HW), 21, 1.0, 0.3), 'w': chunk_outliers(normal((M, K, 1, 1), 22, 0.1), 1), 'bias': normal((M,), 23)}


def _ref_conv1x1(inp, dtype, w=None, bias=True):
    w = inp['w'] if w is None else w
    return (F.conv2d(inp['x'].to(dtype), w.to(dtype), inp['bias'].to(dtype) if bias else None),)


def _scale_conv1x1(inp):
    return (F.conv2d(inp['x'].double().abs(), inp['w'].double().abs(), inp['bias'].double().abs()),)


def _drop_k(name, k, fn):
    def mutant(inp):
        w = inp[name].clone()
        if 0 <= k < w.shape[1] or (k < 0 and w.shape[1] > 1):
            w[:, k] = 0.0
        return fn(inp, w)
    return mutant


def _in_se(case):
    C, Cr = case
    B = 3
    return {'stats': torch.stack([normal((B, C), 31, 1.0, 0.3), uniform((B, C), 32, 0.5, 2.0)], -1),
            'w1': chunk_outliers(normal((Cr, C), 33, 1.0 / math.sqrt(C)), 1, (8, 256)), 'w2': chunk_outliers(normal((C, Cr), 34, 2.0 / math.sqrt(Cr)), 1, (32,))}


def _ref_se(inp, dtype, w1=None, w2=None, relu=True):
    w1 = inp['w1'] if w1 is None else w1
    w2 = inp['w2'] if w2 is None else w2
    h = inp['stats'][..., 0].to(dtype) @ w1.to(dtype).t()
    h = torch.relu(h) if relu else h
    return (torch.sigmoid(h @ w2.to(dtype).t()),)


def _scale_se(inp):
    """An activation's own scale is its value, max(|y|, 2^-126): tanhf / expf return a relative error.  The gate's argument a = W2 relu(W1 m)
    is a sum of products with the usual scale A_a = |W2| (|h| + A_h), A_h = |W1| |m| (ReLU is 1-Lipschitz), and sigmoid'(a) = y (1 - y)
    carries it to the output: A = max(|y|, 2^-126) + y (1 - y) A_a."""
    m, w1, w2 = inp['stats'][..., 0].double(), inp['w1'].double(), inp['w2'].double()
    h = torch.relu(m @ w1.t())
    y = torch.sigmoid(h @ w2.t())
    Aa = (h + m.abs() @ w1.abs().t()) @ w2.abs().t()
    return (y.clamp_min(TINY) + y * (1 - y) * Aa,)


AFFINE_COMBOS = [(sc, sh, sl) for sc in (0, 1) for sh in (0, 1) for sl in (0, 1)]


def _in_conv3(case, few=False):
    B, K, M, H, W, sc, sh, sl = case[:8]
    inp = {'x': normal((B, K, H, W), 41, 1.3, 0.1), 'w': chunk_outliers(normal((M, K, 3, 3), 42, 0.3 / math.sqrt(K)), 1),
           'in_sc': normal((B, K), 43, 0.2, 1.0) if sc else None, 'in_sh': normal((B, K), 44, 0.3, 0.5) if sh else None,
           'slope': normal((M,), 45, 0.05, 0.25) if sl else None}
    if len(case) > 8 and case[8]:
        inp['w11'] = chunk_outliers(normal((case[8], K, 1, 1), 46, 0.05), 1)
    return inp


def _conv3_input(inp, dtype, absolute=False):
    x = inp['x'].to(dtype)
    if inp['in_sc'] is not None:
        x = x * _bc(inp['in_sc'].to(dtype))
    if inp['in_sh'] is not None:
        x = x + _bc(inp['in_sh'].to(dtype))
    return x.abs() if absolute else x


def _prelu(v, slope):
    return v if slope is None else F.prelu(v, slope.to(v.dtype))


def _ref_conv3(inp, dtype, w=None, pad_shift=False, slope=True, last_col=False):
    w = (inp['w'] if w is None else w).to(dtype)
    x = _conv3_input(inp, dtype)
    if last_col:                                        # the last column treated as padding
        x = x.clone()
        x[..., -1] = 0.0
    if pad_shift and inp['in_sh'] is not None:          # the shift reaches the zero padding as well
        sh = _bc(inp['in_sh'].to(dtype))
        v = F.conv2d(F.pad(x - sh, (1, 1, 1, 1)) + sh, w)
    else:
        v = F.conv2d(x, w, padding=1)
    out = (_prelu(v, inp['slope'] if slope else None),)
    if 'w11' in inp:
        out = out + (F.conv2d(inp['x'].to(dtype), inp['w11'].to(dtype)),)
    return out


def _scale_conv3(inp):
    """conv(|x sc + sh|, |w|); PReLU multiplies by 1 or slope and its branch may differ where v ~ 0, so the scale takes max(1, |slope|)."""
    A = F.conv2d(_conv3_input(inp, F64, True), inp['w'].double().abs(), padding=1)
    if inp['slope'] is not None:
        A = A * inp['slope'].double().abs().clamp_min(1.0).view(1, -1, 1, 1)
    out = (A,)
    if 'w11' in inp:
        out = out + (F.conv2d(inp['x'].double().abs(), inp['w11'].double().abs()),)
    return out


def _drop_tap(k, ky=2, kx=2):
    def mutant(inp):
        w = inp['w'].clone()
        if k < w.shape[1]:
            w[-1, k, ky, kx] = 0.0
        return _ref_conv3(inp, F32, w)
    return mutant


# ------------------------------------------------------------------------------------------------------------ activations
HEAD_SPECIALS = (0.0, 88.8, -88.8, 100.0, -100.0, 87.5, -87.5, 20.0, -20.0, 1e-3)


def _in_head(case):
    B, HW = case
    x = torch.cat([uniform((B, 3, 1, HW - HW // 2), 51, -100.0, 100.0), normal((B, 3, 1, HW // 2), 52, 2.0)], -1)
    if HW == 1:
        x[0, :, 0, 0] = torch.tensor([-100.0, 88.8, -88.8])
    else:
        sp = torch.tensor(HEAD_SPECIALS)[:min(len(HEAD_SPECIALS), HW // 2)]
        x[:, :, 0, :len(sp)] = sp                       # first elements of every plane
        x[:, :, 0, HW - len(sp):] = -sp.flip(0)         # and its last ones (the tail of the grid-stride loop)
    return {'x': x, 'scale': 0.08}


def _ref_head(inp, dtype, nt=2):
    x = inp['x'].to(dtype)
    s = torch.tensor(inp['scale'], dtype=F32).to(dtype)
    return (torch.cat([torch.tanh(x[:, :nt]) * s, torch.sigmoid(x[:, nt:])], dim=1),)


def _scale_head(inp):
    """tanhf and expf return a relative error, so the scale is the value itself, floored at the smallest normal number: below it float32
    resolves 2^-149 = 2 * (2^-24 * 2^-126) and no relative error can be asked for.  sigmoid(-88.8) = 2.7e-39 and sigmoid(-100) = 3.7e-44
    are such values: an evaluation as 1 / (1 + exp(-v)) returns 0 there (exp overflows) and is 4e6 units away."""
    return (_ref_head(inp, F64)[0].abs().clamp_min(TINY),)


# ------------------------------------------------------------------------------------------------------------ resampling
def _tap(t, yi, xi):
    return t[..., yi, :][..., :, xi]


def _tap_range(src, ys, xs):
    """max - min of src over the window rows ys x columns xs (lists of index vectors) of every output element."""
    hi = lo = None
    for yi in ys:
        for xi in xs:
            v = _tap(src, yi, xi)
            hi = v if hi is None else torch.maximum(hi, v)
            lo = v if lo is None else torch.minimum(lo, v)
    return hi - lo


def _bilinear_geom(n_in, n_out):
    o = torch.arange(n_out, dtype=F64)
    r = ((n_in / n_out) * (o + 0.5) - 0.5).clamp_min(0.0)
    i0 = r.floor().long().clamp_max(n_in - 1)
    return r, i0, (i0 + 1).clamp_max(n_in - 1), r - i0


def bilinear_scale(src, Ho, Wo):
    """Scale of F.interpolate(mode='bilinear', align_corners=False).  The sum: hy (hx |v00| + lx |v01|) + ly (hx |v10| + lx |v11|).
    The coordinate: r = s (o + 0.5) - 0.5 with s = in / out rounded (u), the product rounded (u) and the difference rounded (u), so
    |dr| <= 3 u max(1, r + 0.5); l = r - floor(r) is exact.  The interpolant is continuous and piecewise linear in r with slope at most
    (max - min) of the taps, taken here over the cell's neighbours as well (a coordinate within u of an integer may fall into the next
    cell): the term is (3 max(1, ry + 0.5) + 3 max(1, rx + 0.5)) * (max - min), in units of u like the rest."""
    Hs, Ws = src.shape[-2:]
    ry, y0, y1, ly = _bilinear_geom(Hs, Ho)
    rx, x0, x1, lx = _bilinear_geom(Ws, Wo)
    a = src.abs()
    ly, hy, lx, hx = ly[:, None], (1 - ly)[:, None], lx[None, :], (1 - lx)[None, :]
    A = hy * (hx * _tap(a, y0, x0) + lx * _tap(a, y0, x1)) + ly * (hx * _tap(a, y1, x0) + lx * _tap(a, y1, x1))
    rng = _tap_range(src, [(y0 - 1).clamp_min(0), y0, y1, (y1 + 1).clamp_max(Hs - 1)], [(x0 - 1).clamp_min(0), x0, x1, (x1 + 1).clamp_max(Ws - 1)])
    delta = 3.0 * (ry + 0.5).clamp_min(1.0)[:, None] + 3.0 * (rx + 0.5).clamp_min(1.0)[None, :]
    return A + delta * rng


def _cubic_w(t, A=-0.75):
    c1 = lambda x: ((A + 2) * x - (A + 3)) * x * x + 1
    c2 = lambda x: ((A * x - 5 * A) * x + 8 * A) * x - 4 * A
    return [c2(t + 1), c1(t), c1(1 - t), c2(2 - t)]


def _bicubic_geom(n_in, n_out):
    o = torch.arange(n_out, dtype=F64)
    r = ((n_in - 1) / (n_out - 1) if n_out > 1 else 0.0) * o
    i = r.floor()
    return r, i.long(), _cubic_w(r - i)


def bicubic_scale(src, Ho, Wo):
    """Scale of F.interpolate(mode='bicubic', align_corners=True): sum_i |wy_i| sum_j |wx_j| |v_ij| over the 16 border-clamped taps, with the
    weights' own values (the cubic polynomials are evaluated in float32 by the reference and the kernels alike; their rounding is part of
    the band).  The coordinate r = s o with s = (in - 1) / (out - 1) rounded (u) and the product rounded (u): |dr| <= 2 u max(1, r);
    t = r - floor(r) is exact.  d/dt of the interpolant is sum_i w_i'(t) v_i = sum_i w_i'(t) (v_i - c), and sum_i |w_i'(t)| <= 3.2 for
    A = -0.75 (|w1'| = |w2'| <= 1.35, |w0'| = |w3'| <= 0.75), so with c the middle of the taps' range the slope is at most
    1.6 (max - min) <= 2 (max - min); the range again includes the neighbouring cell: (4 max(1, ry) + 4 max(1, rx)) * (max - min)."""
    Hs, Ws = src.shape[-2:]
    ry, iy, wy = _bicubic_geom(Hs, Ho)
    rx, ix, wx = _bicubic_geom(Ws, Wo)
    a = src.abs()
    A = 0.0
    for i in range(4):
        row = 0.0
        for j in range(4):
            row = row + wx[j].abs()[None, :] * _tap(a, (iy - 1 + i).clamp(0, Hs - 1), (ix - 1 + j).clamp(0, Ws - 1))
        A = A + wy[i].abs()[:, None] * row
    rng = _tap_range(src, [(iy + k).clamp(0, Hs - 1) for k in range(-2, 4)], [(ix + k).clamp(0, Ws - 1) for k in range(-2, 4)])
    delta = 4.0 * ry.clamp_min(1.0)[:, None] + 4.0 * rx.clamp_min(1.0)[None, :]
    return A + delta * rng


def _last_off(x):
    """the source as an index off by one at the last row and column reads it"""
    x = x.clone()
    if x.shape[-1] > 1:
        x[..., -1] = x[..., -2]
    if x.shape[-2] > 1:
        x[..., -1, :] = x[..., -2, :]
    return x


def _in_resize(case, seed=61):
    planes_, (Hi, Wi), (Ho, Wo) = case[:3]
    inp = {'x': normal((1, planes_, Hi, Wi), seed, 1.0, 0.5), 'size': (Ho, Wo)}
    if len(case) > 3:
        inp['extra'] = case[3]
    return inp


def _ref_nearest(inp, dtype, mode='nearest', x=None):
    # pure indexing: ATen's float32 index formula is the definition, so the float64 'reference' is the same gather
    return (F.interpolate(inp['x'] if x is None else x, size=inp['size'], mode=mode).to(dtype),)


def _ref_bilinear(inp, dtype, ac=False, x=None):
    return (F.interpolate((inp['x'] if x is None else x).to(dtype), size=inp['size'], mode='bilinear', align_corners=ac),)


def _in_bicubic(case):
    inp = _in_resize(case, 62)
    inp['add'] = normal((1, case[0]) + tuple(case[2]), 63) if case[3] else None
    return inp


def _ref_bicubic(inp, dtype, ac=True, x=None, add=True):
    y = F.interpolate((inp['x'] if x is None else x).to(dtype), size=inp['size'], mode='bicubic', align_corners=ac)
    return (y + inp['add'].to(dtype) if add and inp['add'] is not None else y,)


def _scale_bicubic(inp):
    A = bicubic_scale(inp['x'].double(), *inp['size'])
    return (A + inp['add'].double().abs() if inp['add'] is not None else A,)


def _ref_avgpool(inp, dtype, floor=False, drop=False):
    x = inp['x'].to(dtype)
    if not (floor or drop):
        return (F.adaptive_avg_pool2d(x, inp['size']),)
    (Hi, Wi), (Ho, Wo) = x.shape[-2:], inp['size']
    y = torch.empty(x.shape[:2] + (Ho, Wo), dtype=dtype)
    for oy in range(Ho):
        y0, y1 = oy * Hi // Ho, ((oy + 1) * Hi // Ho if floor else -((oy + 1) * Hi // -Ho))
        for ox in range(Wo):
            x0, x1 = ox * Wi // Wo, ((ox + 1) * Wi // Wo if floor else -((ox + 1) * Wi // -Wo))
            win = x[..., y0:y1, x0:x1]
            s = win.sum(dim=(2, 3)) - (win[..., -1, -1] if drop else 0.0)
            y[..., oy, ox] = s / ((y1 - y0) * (x1 - x0))
    return (y,)


# ------------------------------------------------------------------------------------------------------------ fields
FIELD_SCALE = float(torch.tensor(0.08, dtype=F32))


def _field(B, H, W, seed, dstd=0.05):
    # alpha outside [0, 1] as well: the clip has to matter
    return torch.cat([normal((B, 2, H, W), seed, dstd), uniform((B, 1, H, W), seed + 1, -0.25, 1.25)], 1)


def _in_compose(case):
    mode, (Hp, Wp), (H, W) = case
    B = 2
    cur = _field(B, H, W, 71)
    if mode == 0:
        acc = _field(B, H, W, 73)
        # sums that land exactly on +-scale (0.08f - 2^-5 is a float32 and the sum is exact) and beyond it
        s, half = torch.tensor(FIELD_SCALE, dtype=F32), torch.tensor(0.03125)
        plant = [(half, s - half), (-half, half - s), (s, torch.tensor(0.02)), (-s, torch.tensor(-0.2)), (s, -s)]
        a, c = acc.flatten(2), cur.flatten(2)
        for j, (va, vc) in enumerate(plant[:max(1, H * W // 2)]):
            for ch in (0, 1):
                a[:, ch, (j + ch) % (H * W)], c[:, ch, (j + ch) % (H * W)] = va, vc
        return {'mode': 0, 'acc': acc, 'cur': cur, 'scale': FIELD_SCALE}
    return {'mode': 1, 'prev': _field(B, Hp, Wp, 75), 'cur': cur, 'scale': 0.0}


def _prm(x, y):
    return y * x + x * (1 - x)


def _ref_compose(inp, dtype, clip_first=False, swap=False, ac=True, prev=None):
    cur = inp['cur'].to(dtype)
    if inp['mode'] == 0:
        acc, s = inp['acc'].to(dtype), inp['scale']
        if clip_first:
            d = torch.clip(acc[:, :2], -s, s) + torch.clip(cur[:, :2], -s, s)
            xa, ya = torch.clip(acc[:, 2:], 0, 1), torch.clip(cur[:, 2:], 0, 1)
            return (torch.cat([d, _prm(xa, ya)], 1),)
        if swap:
            return (torch.cat([torch.clip(acc[:, :2] + cur[:, :2], -s, s), torch.clip(_prm(cur[:, 2:], acc[:, 2:]), 0, 1)], 1),)
        return (R.spm_add(acc, cur, s),)
    prev = (inp['prev'] if prev is None else prev).to(dtype)
    if clip_first or swap or not ac:
        xa = prev[:, 2:]
        if xa.shape[-2:] != cur.shape[-2:]:
            xa = F.interpolate(xa, size=cur.shape[-2:], mode='bicubic', align_corners=ac)
        ya = cur[:, 2:]
        if clip_first:
            al = _prm(torch.clip(xa, 0, 1), torch.clip(ya, 0, 1))
        else:
            al = torch.clip(_prm(ya, xa) if swap else _prm(xa, ya), 0, 1)
        return (torch.cat([cur[:, :2], al], 1),)
    return (R.spm_upsample_add(prev, cur),)


def _prm_scale(xa, ya, Axa):
    """y x + x (1 - x) over absolute values, |y||x| + |x| (1 + |x|), plus the error A_x of x itself carried by
    |d/dx| = |y + 1 - 2 x| <= |y| + 1 + 2 |x|.  The clips are 1-Lipschitz."""
    return ya.abs() * xa.abs() + xa.abs() * (1 + xa.abs()) + (ya.abs() + 1 + 2 * xa.abs()) * Axa


def _scale_compose(inp):
    cur = inp['cur'].double()
    if inp['mode'] == 0:
        acc = inp['acc'].double()
        return (torch.cat([acc[:, :2].abs() + cur[:, :2].abs(), _prm_scale(acc[:, 2:], cur[:, 2:], 0.0)], 1),)
    prev = inp['prev'].double()
    if prev.shape[-2:] == cur.shape[-2:]:
        xa, Axa = prev[:, 2:], 0.0
    else:
        xa = F.interpolate(prev[:, 2:], size=cur.shape[-2:], mode='bicubic', align_corners=True)
        Axa = bicubic_scale(prev[:, 2:], *cur.shape[-2:])
    return (torch.cat([torch.zeros_like(cur[:, :2]), _prm_scale(xa, cur[:, 2:], Axa)], 1),)


def _in_warp(case):
    B, C, H, W = case
    t = normal((B, C, H, W), 81, 1.0, 0.2)
    f = torch.cat([normal((B, 2, H, W), 82, 0.3), uniform((B, 1, H, W), 83)], 1)
    ff = f.flatten(2)
    n = H * W
    # zero displacement; +-3 (nothing in range); alpha exactly 0 and 1
    for j, (dx, dy, al) in enumerate([(0.0, 0.0, 0.5), (3.0, 3.0, 0.7), (-3.0, -3.0, 0.3), (0.1, -0.1, 0.0), (-0.1, 0.1, 1.0)]):
        if j < n - 1 or j == 0:
            ff[:, 0, j], ff[:, 1, j], ff[:, 2, j] = dx, dy, al
    # the last pixel samples exactly the last column and row where W, H are powers of two (gx = 1 - 1/W: ix = W - 1), within an ulp of
    # it elsewhere; pixel (0, 0) + 2 - 1/W likewise from the other end
    if n > 1:
        ff[:, 0, n - 1], ff[:, 1, n - 1], ff[:, 2, n - 1] = -1.0 / W, -1.0 / H, 0.9
    if n > 6:
        ff[:, 0, 5], ff[:, 1, 5] = 2.0 - 1.0 / W - 2.0 * (5 % W) / max(W - 1, 1), 2.0 - 1.0 / H - 2.0 * (5 // W) / max(H - 1, 1)
    return {'target': t, 'field': f}


def _ref_warp(inp, dtype, swap=False, ac=False, target=None, drop_c=None):
    t, f = (inp['target'] if target is None else target).to(dtype), inp['field'].to(dtype)
    if not (swap or ac or drop_c is not None):
        return (R.warp_blend(t, f),)
    B, _, H, W = t.shape
    gy, gx = torch.meshgrid(torch.linspace(-1, 1, H, dtype=dtype), torch.linspace(-1, 1, W, dtype=dtype), indexing='ij')
    grid = torch.stack([gx.unsqueeze(0) + f[:, 0], gy.unsqueeze(0) + f[:, 1]], dim=-1)
    warped = F.grid_sample(t, grid, mode='bilinear', padding_mode='zeros', align_corners=ac)
    alpha = f[:, 2:]
    y = warped * (1 - alpha) + t * alpha if swap else warped * alpha + t * (1 - alpha)
    if drop_c is not None and drop_c < y.shape[1]:
        y[:, drop_c] = t[:, drop_c]
    return (y,)


def _scale_warp(inp):
    """warped |alpha| + |t| (1 + |alpha|), warped = sum of the four |w| |tap| (zero outside the image) plus the coordinate term.
    ix = ((gx + 1) W - 1) / 2 with gx = linspace + dx: the linspace value (u, |.| <= 1), the sum gx (u |gx|), gx + 1 (u |gx + 1|) — each
    times W / 2 — then the product and the difference (u each, of about 2 |ix| + 1); the halving is exact:
    |d ix| <= u ((W / 2) (1 + |gx| + |gx + 1|) + 2 |ix| + 1), likewise for iy.  The interpolant with zero padding is continuous and piecewise linear with
    slope at most (max - min) of the taps, zeros included, taken over the neighbouring cells as well."""
    t, f = inp['target'].double(), inp['field'].double()
    B, C, H, W = t.shape
    gy, gx = torch.meshgrid(torch.linspace(-1, 1, H, dtype=F64), torch.linspace(-1, 1, W, dtype=F64), indexing='ij')
    gx, gy = gx[None] + f[:, 0], gy[None] + f[:, 1]
    ix, iy = ((gx + 1) * W - 1) / 2, ((gy + 1) * H - 1) / 2
    dix = (W / 2) * (1 + gx.abs() + (gx + 1).abs()) + 2 * ix.abs() + 1
    diy = (H / 2) * (1 + gy.abs() + (gy + 1).abs()) + 2 * iy.abs() + 1
    x0, y0 = ix.floor(), iy.floor()
    wx1, wy1 = ix - x0, iy - y0
    tp = F.pad(t, (3, 3, 3, 3))                     # zeros; indices clamped into the padding ring

    def tap(src, yy, xx):
        yy, xx = (yy + 3).clamp(0, H + 5).long(), (xx + 3).clamp(0, W + 5).long()
        return torch.stack([src[b][:, yy[b], xx[b]] for b in range(B)])

    A = 0.0
    for (dy_, wy) in ((0, 1 - wy1), (1, wy1)):
        for (dx_, wx) in ((0, 1 - wx1), (1, wx1)):
            A = A + (wy * wx)[:, None] * tap(tp.abs(), y0 + dy_, x0 + dx_)
    hi = lo = None
    for dy_ in range(-1, 3):
        for dx_ in range(-1, 3):
            v = tap(tp, y0 + dy_, x0 + dx_)
            hi = v if hi is None else torch.maximum(hi, v)
            lo = v if lo is None else torch.minimum(lo, v)
    A = A + (dix + diy)[:, None] * (hi - lo)
    alpha = f[:, 2:].abs()
    return (A * alpha + t.abs() * (1 + alpha),)


def _in_mask(case):
    sizes, S, blend = case
    B = 2
    inp = {'fields': [_field(B, s, s, 90 + s) for s in sizes], 'S': S, 'x': None, 'gen': None}
    if blend:
        inp['x'], inp['gen'] = normal((B, 3, S, S), 95, 1.0, 0.2), normal((B, 3, S, S), 96, 1.0, -0.3)
    return inp


def _ref_mask(inp, dtype, swap=False, skip_full=False, ac=False, clip_first=False):
    """oracle.ref_cpu.blending_mask skips a field whose size equals S (its caller never holds one); the kernel composes it as it is
    (s == S: a plain read), and so does this reference."""
    S, a = inp['S'], None
    for f in inp['fields']:
        if skip_full and f.shape[-1] == S:
            continue
        ak = f[:, 2:].to(dtype)
        if ak.shape[-1] != S:
            ak = F.interpolate(ak, size=(S, S), mode='bilinear', align_corners=ac)
        if clip_first:
            ak = torch.clip(ak, 0, 1)
        if a is None:
            a = ak
        else:
            a = a * ak + ak * (1 - ak) if swap else ak * a + a * (1 - a)
    a = a if clip_first else torch.clip(a, 0.0, 1.0)
    if inp['gen'] is None:
        return (a,)
    return (a, a * inp['x'].to(dtype) + inp['gen'].to(dtype) * (1 - a))


def _scale_mask(inp):
    """a' = a_k a + a (1 - a): |a_k||a| + |a| (1 + |a|), plus the errors of its operands carried by the partial derivatives,
    |a| A_k + (|a_k| + 1 + 2 |a|) A_a, with A_k the bilinear scale (0 for a field read as it is).  out = a x + gen (1 - a):
    |a||x| + |gen| (1 + |a|) + (|x| + |gen|) A_a."""
    S, a, Aa = inp['S'], None, None
    for f in inp['fields']:
        ak = f[:, 2:].double()
        Ak = torch.zeros_like(ak)
        if ak.shape[-1] != S:
            Ak = bilinear_scale(ak, S, S)
            ak = F.interpolate(ak, size=(S, S), mode='bilinear')
        if a is None:
            a, Aa = ak, Ak
        else:
            Aa = ak.abs() * a.abs() + a.abs() * (1 + a.abs()) + a.abs() * Ak + (ak.abs() + 1 + 2 * a.abs()) * Aa
            a = ak * a + a * (1 - a)
    a = torch.clip(a, 0.0, 1.0)
    if inp['gen'] is None:
        return (Aa,)
    x, g = inp['x'].double().abs(), inp['gen'].double().abs()
    return (Aa, a * x + g * (1 + a) + (x + g) * Aa)


# ------------------------------------------------------------------------------------------------------------ registry
def _sq(n):
    return (n, n)


def _conv3_small_cases():
    cases, n = [], 0
    for (K, M) in ((1, 1), (1, 8), (8, 1), (8, 8), (5, 3)):            # K <= 8 && M <= 8: both limits and 1
        for (H, W) in ((1, 5), (5, 1), (13, 17), (16, 17)):            # H == 1, W == 1; HW = 272 > 256: a second block
            cases.append((2, K, M, H, W) + AFFINE_COMBOS[n % 8])
            n += 3
    for combo in AFFINE_COMBOS:                                         # in_sc / in_sh / slope each passed and omitted
        cases.append((2, 5, 3, 13, 17) + combo)
        cases.append((2, 8, 8, 16, 17) + combo)
    return list(dict.fromkeys(cases))


FEWOUT_SHAPES = ((2, 200, 20, 45, 3), (1, 1024, 32, 32, 3), (3, 16, 9, 7, 4), (1, 256, 64, 64, 1), (1, 8, 1, 5, 4), (2, 64, 20, 44, 3))
# (B, K, H, W, M, M2); the quad form (fewout3) runs when fewout_quad && M == 3 && (M2 == 0 || M2 == 3) && W % 4 == 0
FEWOUT2_SHAPES = ((2, 200, 20, 45, 3, 3), (1, 1024, 32, 32, 3, 3), (3, 16, 9, 7, 4, 2), (1, 256, 64, 64, 1, 0), (8, 256, 40, 33, 3, 3),
                  (2, 64, 20, 44, 3, 3), (2, 72, 13, 36, 3, 0), (1, 512, 128, 128, 3, 3), (1, 8, 1, 5, 4, 0))

def _few(shape, sc, sh, sl):
    B, K, H, W, M = shape[:5]
    return (B, K, M, H, W, sc, sh, sl) + tuple(shape[5:])


CASES = {
    # (HW & 3) == 0: float4 path, else scalar; HW < 256; i += 1024 float4: a second trip from HW > 4096; constant plane
    'instnorm_stats': [(hw, False) for hw in STAT_HW] + [(1028, True)],
    'affine_apply_stats': [(hw, False, res) for hw in STAT_HW for res in (False, True)] + [(1028, True, True)],
    'align_input_stats': [(hw, False, diff) for hw in STAT_HW for diff in (0, 1)] + [(1028, True, 1)],
    # gx = min(64, ceil(HW / 256)): the grid-stride loop makes a second trip from HW > 16384
    'affine_apply': [(5, False, True), (16384, False, False), (16389, False, True), (16389, False, False)],
    'align_input': [(5, False, 1), (16384, False, 0), (16389, False, 1), (16389, False, 0)],
    'instnorm_coeffs': [(g, b) for g in (0, 1) for b in (0, 1)],
    # wide form: M > 16 && ceil(HW/256)*ceil(M/64)*B >= 1024; K chunks of 64 (narrow) / 32 (wide); eight planes per trip (K < 8)
    'conv1x1': [(1, 1, 1, 1), (2, 7, 16, 300), (1, 65, 17, 257), (1, 64, 35, 81), (8, 33, 65, 16129), (4, 32, 130, 32768 + 3)],
    # C <= 1024 && Cr <= 64; j0 += 32: Cr = 33 needs a second, partial trip; c += 8: C = 13 is no multiple
    'se_gate': [(1, 1), (13, 33), (512, 32), (1024, 64)],
    'conv3x3_small': _conv3_small_cases(),
    # cases are (B, K, M, H, W, in_sc, in_sh, slope[, M2])
    'conv3x3_fewout': [_few(s, 1, 1, 1) for s in FEWOUT_SHAPES] + [_few(s, 0, 0, 0) for s in FEWOUT_SHAPES[2:5]],
    'conv3x3_fewout2': [_few(s, 1, 1, 1) for s in FEWOUT2_SHAPES] + [_few((3, 16, 9, 7, 4, 2), 0, 0, 0), _few((2, 64, 20, 44, 3, 3), 1, 0, 0)],
    # stream_grid caps at 2048 blocks: 3 * HW > 524288 starts the grid-stride loop
    'align_head': [(1, 1), (3, 257), (2, 300000)],
    'field_compose': [(0, (1, 3), (1, 3)), (0, (7, 9), (7, 9)), (0, (16, 17), (16, 17))] +
                     [(1, p, s) for p, s in ((_sq(1), _sq(4)), (_sq(3), _sq(7)), ((4, 6), (9, 11)), (_sq(5), _sq(5)), (_sq(8), _sq(1)), (_sq(16), _sq(32)))],
    # H == 1 / W == 1: linspace_pm1(n == 1); C = 1, 8, 9, 13 around the channel chunk of 8
    'warp_blend': [(1, 1, 1, 5), (1, 8, 5, 1), (2, 9, 16, 17), (1, 13, 24, 40)],
    # s == S is a plain read; chunks = min(1024, ceil(S*S / 256)): the grid-stride loop from S*S > 262144 (S = 520)
    'mask_blend': [((6,), 48, True), ((6, 12), 48, True), ((6, 12, 24), 48, True), ((6, 12, 24, 48), 48, True), ((5, 7), 33, True),
                   ((6, 12, 24, 48), 48, False), ((5, 7), 33, False), ((65, 130), 520, True)],
    'resize_nearest': [(3, _sq(37), _sq(100)), (3, _sq(100), _sq(37)), (3, _sq(64), _sq(16)), (3, _sq(5), _sq(48)), (3, (4, 6), (9, 11)),
                       (3, _sq(5), _sq(12), ('pitch', 40, 0)), (3, _sq(5), _sq(12), ('pitch', 40, 17))],
    # the last case has 3 * 420 * 420 = 529200 > 524288 outputs: the grid-stride loop
    'resize_bilinear': [(3, _sq(1), _sq(4)), (3, _sq(3), _sq(7)), (3, (4, 6), (9, 11)), (3, _sq(37), _sq(100)), (3, _sq(100), _sq(37)),
                        (3, _sq(64), _sq(16)), (3, (7, 5), (3, 9)), (3, _sq(64), _sq(420))],
    'resize_bicubic_ac': [(3, p, s, add) for p, s in ((_sq(1), _sq(4)), (_sq(3), _sq(7)), ((4, 6), (9, 11)), (_sq(5), _sq(12)), (_sq(16), _sq(32)),
                                                       (_sq(8), _sq(1)), ((9, 9), (4, 7))) for add in (False, True)],
    # wave kernel when (ceil(Hin/Hout)+1)*(ceil(Win/Wout)+1) >= 128: 30 -> 3 gives 121, 31 -> 3 gives 144; its grid is capped at 2048 blocks
    # of four outputs: 1000 planes * 9 = 9000 > 8192; one plane: 9 outputs, no multiple of four
    'avgpool': [(6, _sq(30), _sq(3)), (6, _sq(31), _sq(3)), (6, _sq(128), _sq(3)), (6, _sq(1024), _sq(256)), (6, (40, 33), (3, 5)),
                (1, _sq(31), _sq(3)), (1, _sq(30), _sq(3)), (1000, _sq(31), _sq(3))],
}

_MAKE = {
    'instnorm_stats': _in_stats, 'affine_apply_stats': _in_affine, 'align_input_stats': _in_align, 'affine_apply': _in_affine,
    'align_input': _in_align, 'instnorm_coeffs': _in_coeffs, 'conv1x1': _in_conv1x1, 'se_gate': _in_se, 'conv3x3_small': _in_conv3,
    'conv3x3_fewout': _in_conv3, 'conv3x3_fewout2': _in_conv3, 'align_head': _in_head, 'field_compose': _in_compose, 'warp_blend': _in_warp,
    'mask_blend': _in_mask, 'resize_nearest': _in_resize, 'resize_bilinear': _in_resize, 'resize_bicubic_ac': _in_bicubic,
    'avgpool': lambda case: _in_resize(case, 64),
}

_REF = {
    'instnorm_stats': _ref_stats, 'affine_apply_stats': _ref_affine_stats, 'align_input_stats': _ref_align_stats,
    'affine_apply': lambda inp, dt: (_affine(inp, dt),), 'align_input': lambda inp, dt: (_align(inp, dt),), 'instnorm_coeffs': _ref_coeffs,
    'conv1x1': _ref_conv1x1, 'se_gate': _ref_se, 'conv3x3_small': _ref_conv3, 'conv3x3_fewout': _ref_conv3, 'conv3x3_fewout2': _ref_conv3,
    'align_head': _ref_head, 'field_compose': _ref_compose, 'warp_blend': _ref_warp, 'mask_blend': _ref_mask, 'resize_nearest': _ref_nearest,
    'resize_bilinear': _ref_bilinear, 'resize_bicubic_ac': _ref_bicubic, 'avgpool': _ref_avgpool,
}

_SCALE = {
    'instnorm_stats': _scale_stats, 'affine_apply_stats': _scale_affine_stats, 'align_input_stats': _scale_align_stats,
    'affine_apply': lambda inp: (_affine_abs(inp),), 'align_input': lambda inp: (_align_abs(inp),), 'instnorm_coeffs': _scale_coeffs,
    'conv1x1': _scale_conv1x1, 'se_gate': _scale_se, 'conv3x3_small': _scale_conv3, 'conv3x3_fewout': _scale_conv3,
    'conv3x3_fewout2': _scale_conv3, 'align_head': _scale_head, 'field_compose': _scale_compose, 'warp_blend': _scale_warp,
    'mask_blend': _scale_mask, 'resize_nearest': lambda inp: (None,),
    'resize_bilinear': lambda inp: (bilinear_scale(inp['x'].double(), *inp['size']),), 'resize_bicubic_ac': _scale_bicubic,
    'avgpool': lambda inp: (F.adaptive_avg_pool2d(inp['x'].double().abs(), inp['size']),),
}

def _w_drop(w, k):
    w = w.clone()
    if k < w.shape[1]:
        w[-1, k, 2, 2] = 0.0
    return w


def _w11_drop(inp):
    if 'w11' not in inp:
        return _ref_conv3(inp, F32)
    w11 = inp['w11'].clone()
    w11[:, -1] = 0.0
    return _ref_conv3(dict(inp, w11=w11), F32)


_few_mutants = {
    'shift applied to the padding': lambda inp: _ref_conv3(inp, F32, pad_shift=True),
    'tap (2,2) of the last channel dropped': lambda inp: _ref_conv3(inp, F32, _w_drop(inp['w'], -1)),
    'tap (2,2) of channel 8 (second LDS stage) dropped': lambda inp: _ref_conv3(inp, F32, _w_drop(inp['w'], 8)),
    'tap (2,2) of channel 7 (end of the first stage) dropped': lambda inp: _ref_conv3(inp, F32, _w_drop(inp['w'], 7)),
    'last column read as padding': lambda inp: _ref_conv3(inp, F32, last_col=True),
}

MUTANTS = {
    'instnorm_stats': _stat_mutants(lambda inp: ((), inp['x'])),
    'affine_apply_stats': dict(_stat_mutants(lambda inp: ((_affine(inp, F32),), _affine(inp, F32))),
                               **{'res ignored': lambda inp: _ref_affine_stats(dict(inp, res=None), F32)}),
    # no one-pass variance here: the planes this op stores are normalised (mean 0, std 1), where one pass is as good as two
    'align_input_stats': dict({k: v for k, v in _stat_mutants(lambda inp: ((_align(inp, F32),), _align(inp, F32))).items() if k != 'one-pass variance'},
                              **{'diff ignored': lambda inp: _ref_align_stats(dict(inp, diff=1), F32)}),
    'affine_apply': {'res ignored': lambda inp: (_affine(dict(inp, res=None), F32),),
                     'last element dropped': lambda inp: (_zero_last(_affine(inp, F32)),)},
    'align_input': {'diff ignored': lambda inp: (_align(inp, F32, diff=1),), 'last element dropped': lambda inp: (_zero_last(_align(inp, F32)),)},
    'instnorm_coeffs': {'gamma ignored': lambda inp: _ref_coeffs(inp, F32, use_gamma=False), 'beta ignored': lambda inp: _ref_coeffs(inp, F32, use_beta=False),
                        'gamma of the last channel read one early': lambda inp: _ref_coeffs(inp, F32, roll=True)},
    'conv1x1': {'last channel dropped': _drop_k('w', -1, lambda inp, w: _ref_conv1x1(inp, F32, w)),
                'channel 32 (one past a wide chunk) dropped': _drop_k('w', 32, lambda inp, w: _ref_conv1x1(inp, F32, w)),
                'channel 64 (one past a narrow chunk) dropped': _drop_k('w', 64, lambda inp, w: _ref_conv1x1(inp, F32, w)),
                'channel 31 (end of a wide chunk) dropped': _drop_k('w', 31, lambda inp, w: _ref_conv1x1(inp, F32, w)),
                'bias dropped': lambda inp: _ref_conv1x1(inp, F32, bias=False)},
    'se_gate': {'last channel dropped': _drop_k('w1', -1, lambda inp, w: _ref_se(inp, F32, w1=w)),
                'last hidden unit dropped': _drop_k('w2', -1, lambda inp, w: _ref_se(inp, F32, w2=w)),
                'hidden unit 32 (second trip) dropped': _drop_k('w2', 32, lambda inp, w: _ref_se(inp, F32, w2=w)),
                'ReLU omitted': lambda inp: _ref_se(inp, F32, relu=False)},
    'conv3x3_small': {k: v for k, v in _few_mutants.items() if 'channel 8' not in k and 'channel 7' not in k},
    'conv3x3_fewout': _few_mutants,
    'conv3x3_fewout2': dict(_few_mutants, **{'1x1: last channel dropped': _w11_drop}),
    'align_head': {'sigmoid on channel 1': lambda inp: _ref_head(inp, F32, nt=1), 'last element dropped': lambda inp: (_zero_last(_ref_head(inp, F32)[0]),)},
    'field_compose': {'clip before the composition': lambda inp: _ref_compose(inp, F32, clip_first=True),
                      'alpha composed in the other order': lambda inp: _ref_compose(inp, F32, swap=True),
                      'align_corners flipped': lambda inp: _ref_compose(inp, F32, ac=False),
                      'source index off by one at the last row / column': lambda inp: _ref_compose(inp, F32, prev=_last_off(inp['prev'])) if inp['mode'] else _ref_compose(inp, F32)},
    'warp_blend': {'alpha composed in the other order': lambda inp: _ref_warp(inp, F32, swap=True), 'align_corners flipped': lambda inp: _ref_warp(inp, F32, ac=True),
                   'source index off by one at the last row / column': lambda inp: (_warp_off(inp),),
                   'channel 8 (second chunk) dropped': lambda inp: _ref_warp(inp, F32, drop_c=8)},
    'mask_blend': {'alpha composed in the other order': lambda inp: _ref_mask(inp, F32, swap=True), 'field with s == S skipped': lambda inp: _ref_mask(inp, F32, skip_full=True),
                   'align_corners flipped': lambda inp: _ref_mask(inp, F32, ac=True), 'clip before the composition': lambda inp: _ref_mask(inp, F32, clip_first=True)},
    'resize_nearest': {'nearest-exact': lambda inp: _ref_nearest(inp, F32, mode='nearest-exact'),
                       'source index off by one at the last row / column': lambda inp: _ref_nearest(inp, F32, x=_last_off(inp['x']))},
    'resize_bilinear': {'align_corners flipped': lambda inp: _ref_bilinear(inp, F32, ac=True),
                        'source index off by one at the last row / column': lambda inp: _ref_bilinear(inp, F32, x=_last_off(inp['x']))},
    'resize_bicubic_ac': {'align_corners flipped': lambda inp: _ref_bicubic(inp, F32, ac=False), 'add dropped': lambda inp: _ref_bicubic(inp, F32, add=False),
                          'source index off by one at the last row / column': lambda inp: _ref_bicubic(inp, F32, x=_last_off(inp['x']))},
    'avgpool': {'window end floor instead of ceil': lambda inp: _ref_avgpool(inp, F32, floor=True), 'last element of the window dropped': lambda inp: _ref_avgpool(inp, F32, drop=True)},
}


def _warp_off(inp):
    """the warp with the last row / column of the SAMPLED image off by one (the blend still reads the true target)"""
    t = inp['target']
    warped_off = _ref_warp(dict(inp, field=torch.cat([inp['field'][:, :2], torch.ones_like(inp['field'][:, 2:])], 1)), F32, target=_last_off(t))[0]
    alpha = inp['field'][:, 2:]
    return warped_off * alpha + t * (1 - alpha)


OPS = tuple(CASES)
# cases too large for the mutant sweep (the mutants need one case each; the small ones carry them)
HEAVY = {('conv1x1', (8, 33, 65, 16129)), ('conv1x1', (4, 32, 130, 32768 + 3)), ('conv3x3_fewout2', (1, 512, 3, 128, 128, 1, 1, 1, 3)),
         ('mask_blend', ((65, 130), 520, True)), ('avgpool', (6, _sq(1024), _sq(256))), ('avgpool', (1000, _sq(31), _sq(3))),
         ('resize_bilinear', (3, _sq(64), _sq(420))), ('align_head', (2, 300000))}


def case_id(case):
    def s(v):
        if isinstance(v, (tuple, list)):
            return 'x'.join(s(t) for t in v)
        return str(v)
    return '-'.join(s(v) for v in case)


def inputs(op, case):
    return _MAKE[op](case)


def ref(op, inp, dtype):
    with torch.no_grad():
        return tuple(_REF[op](inp, dtype))


def scale(op, inp):
    with torch.no_grad():
        return tuple(_SCALE[op](inp))


def terms(op, inp):
    """n, the number of terms of an output element: the any-order worst case of a float32 sum of n products is (n + 2) units."""
    if op in ('instnorm_stats', 'affine_apply_stats', 'align_input_stats'):
        return (inp['x'] if 'x' in inp else inp['gen']).shape[-1] + 4
    if op == 'conv1x1':
        return inp['x'].shape[1] + 1
    if op == 'se_gate':
        return inp['w1'].shape[0] + inp['w1'].shape[1]
    if op.startswith('conv3x3'):
        return 9 * inp['x'].shape[1] + 2
    if op == 'avgpool':
        (Hi, Wi), (Ho, Wo) = inp['x'].shape[-2:], inp['size']
        return (-(-Hi // Ho) + 1) * (-(-Wi // Wo) + 1)
    return ELEMENTWISE_TERMS[op]


# roundings on the longest path of one output element, for the ops that are no long sums
ELEMENTWISE_TERMS = {
    'affine_apply': 3, 'align_input': 5, 'instnorm_coeffs': 3,
    'align_head': 14,               # tanhf / expf of a float32 libm are within 4 ulp = 8 u, then the add and the divide, or the product with scale
    'field_compose': 4 + 30, 'resize_bicubic_ac': 30,     # 16 taps, two weight polynomials of six operations each, the add
    'resize_bilinear': 10, 'mask_blend': 4 * 10 + 3 * 4 + 4, 'warp_blend': 16,
    'resize_nearest': 0,
}


@functools.lru_cache(maxsize=None)
def case_bundle(op, case):
    """(inputs, float64 reference, scales) of a case, computed once and shared between the tests."""
    inp = inputs(op, case)
    return inp, ref(op, inp, F64), scale(op, inp)
