"""Float64 references of the style, backward-tail and range-scale kernels (csrc/style.hip, csrc/bwd_tail.hip, csrc/fwd_range.hip and the
reduction / abs-max kernels of csrc/elementwise.hip and csrc/bwd_producers.hip), written from the formulas in the kernels' header comments
in plain torch, plus the integer-valued data sets on which float32 arithmetic is exact in any order.

tests/test_tail_ref_cpu.py checks the references against autograd and the data sets against the exact regime; tests/test_hip_style_tail.py
compares the kernels with them."""
import math

import numpy as np
import torch

F64 = torch.float64
U = 2.0 ** -24          # unit roundoff of float32


# ----------------------------------------------------------------------------- data
def ints(shape, seed, lo=-4, hi=4):
    """float32 tensor of integers in [lo, hi]"""
    g = torch.Generator().manual_seed(seed)
    return torch.randint(lo, hi + 1, tuple(shape), generator=g).to(torch.float32)


def pow2(shape, seed, lo=-2, hi=2):
    """float32 tensor of powers of two 2^lo .. 2^hi"""
    g = torch.Generator().manual_seed(seed)
    return torch.ldexp(torch.ones(tuple(shape)), torch.randint(lo, hi + 1, tuple(shape), generator=g)).to(torch.float32)


def normal(shape, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(tuple(shape), generator=g)


def exact_regime(terms):
    """terms (..., n) float32: the float32 sum forwards, the float32 sum reversed and the float64 sum of every row are identical (the sums
    are taken sequentially, so every partial sum on the way is a float32 number too)."""
    t = terms.reshape(-1, terms.shape[-1]).to(torch.float32).contiguous()
    assert t.dtype == torch.float32
    # numpy's accumulate adds one float32 at a time (torch's CPU cumsum accumulates in double)
    fwd = torch.from_numpy(np.cumsum(t.numpy(), axis=1, dtype=np.float32))
    rev = torch.from_numpy(np.cumsum(t.flip(1).contiguous().numpy(), axis=1, dtype=np.float32))
    s64 = t.to(F64).sum(1)
    # cumsum in float32 must reproduce the float64 prefix sums element for element: every partial sum is exact
    return bool(torch.equal(fwd.to(F64), torch.cumsum(t.to(F64), 1)) and torch.equal(rev.to(F64), torch.cumsum(t.flip(1).to(F64), 1))
                and torch.equal(fwd[:, -1].to(F64), s64) and torch.equal(rev[:, -1].to(F64), s64))


# ----------------------------------------------------------------------------- style affine
def style_affine_acc(lat, w, row_lat=None):
    """acc[b,r] = sum_k W[r,k] * lat[b, row_lat[r], k]   (float64)"""
    lat = lat.to(F64)
    if lat.ndim == 2:
        lat = lat.unsqueeze(1)
    R = w.shape[0]
    rl = torch.zeros(R, dtype=torch.long) if row_lat is None else torch.as_tensor(row_lat).long()
    return torch.einsum('brk,rk->br', lat[:, rl, :], w.to(F64))


def style_affine(lat, w, bias=None, row_lat=None, lr_mul=1.0):
    """s[b,r] = (1/sqrt(S)) * lr_mul * acc[b,r] + bias[r] * lr_mul.  Returns (s, bound_scale) with bound_scale = |acc*scale| + |bias*lr_mul|."""
    S = w.shape[1]
    scale = (1.0 / math.sqrt(S)) * lr_mul
    a = style_affine_acc(lat, w, row_lat) * scale
    b = torch.zeros(w.shape[0], dtype=F64) if bias is None else bias.to(F64) * lr_mul
    return a + b, a.abs() + b.abs()


def style_affine_backward(gs, w, lat_start, L, lr_mul=1.0, grad_div=1.0):
    """glat[b,l,k] = scale * sum_{r in [lat_start[l], lat_start[l+1])} gs[b,r] * W[r,k], scale = (1/sqrt(S)) * lr_mul / grad_div"""
    B, S = gs.shape[0], w.shape[1]
    scale = (1.0 / math.sqrt(S)) * lr_mul / grad_div
    out = torch.zeros(B, L, S, dtype=F64)
    for l in range(L):
        a, b = int(lat_start[l]), int(lat_start[l + 1])
        if b > a:
            out[:, l] = gs[:, a:b].to(F64) @ w[a:b].to(F64)
    return out * scale


def row_lat_of(lat_start, R):
    rl = torch.zeros(R, dtype=torch.long)
    for l in range(len(lat_start) - 1):
        rl[int(lat_start[l]):int(lat_start[l + 1])] = l
    return rl


# ----------------------------------------------------------------------------- demodulation
def weight_sqsum(w):
    """(Co,Ci,k,k) -> (Co,Ci): sum of squares over the taps"""
    return (w.to(F64) ** 2).sum((2, 3))


def demod_arg(s, wsq, scale):
    """scale^2 * sum_ci s[b,ci]^2 * wsq[co,ci]  (B,Co)"""
    return (scale * scale) * ((s.to(F64) ** 2) @ wsq.to(F64).t())


def demod_fwd(s, wsq, scale):
    """d[b,co] = rsqrt(scale^2 * sum_ci s^2 * wsq + 1e-8)"""
    return torch.rsqrt(demod_arg(s, wsq, scale) + 1e-8)


def demod_bwd(s, wsq, d, r, scale):
    """the increment of gs: -scale^2 * s[b,ci] * sum_co r[b,co] * d[b,co]^2 * wsq[co,ci]"""
    return -(scale * scale) * s.to(F64) * ((r.to(F64) * d.to(F64) ** 2) @ wsq.to(F64))


# ----------------------------------------------------------------------------- reductions
def reduce_rows(part, part2=None, scale2=None):
    """part (B,C,n) -> (B,C): sum_j part[b,c,j] (+ scale2[b,c] * sum_j part2[b,c,j]).  Also the sum of absolute values."""
    s, a = part.to(F64).sum(-1), part.to(F64).abs().sum(-1)
    if part2 is not None:
        s = s + scale2.to(F64) * part2.to(F64).sum(-1)
        a = a + scale2.to(F64).abs() * part2.to(F64).abs().sum(-1)
    return s, a


# ----------------------------------------------------------------------------- range scales
def range_exp(m):
    """e with m * 2^e in [512, 1024); 0 for zero / non-finite m; clamped to +-100 (fwd_range.hip)."""
    m = float(m)
    if not (m > 0.0 and math.isfinite(m)):
        return 0
    mant, ex = math.frexp(m)            # m = mant * 2^ex, mant in [0.5, 1): floor(log2 m) = ex - 1
    return max(-100, min(100, 9 - (ex - 1)))


def absmax_scaled(x, s=None):
    """vmax[b] = max_c float32(max_p |x[b,c,p]| * |s[b,c]|); +inf when the sample holds a non-finite value"""
    B, C = x.shape[0], x.shape[1]
    xf = x.reshape(B, C, -1)
    m = xf.abs().amax(2)
    m = torch.where(torch.isfinite(xf).all(2), m, torch.full_like(m, math.inf))
    if s is not None:
        m = (m * s.abs().to(torch.float32)).to(torch.float32)       # one float32 product, as stored
        m = torch.where(torch.isnan(m), torch.full_like(m, math.inf), m)
    return m.amax(1)


def bits_of(v):
    return torch.as_tensor(v, dtype=torch.float32).view(torch.int32)


def fwd_range_update(vm_bits, q, carry):
    """vm_bits (n, slots) int32 float patterns, q (n,) -> (new q, flag).  Carry mode: the maxima were measured on values scaled by q; bit 1 when a
    positive finite maximum is outside [1, 2^15), bit 2 when one is non-finite."""
    m = vm_bits.view(torch.float32).amax(1)
    flag, out = 0, []
    for mi, qi in zip(m.tolist(), q.tolist()):
        t = mi
        if carry:
            if not math.isfinite(mi):
                flag |= 2
            elif mi > 0.0 and not (1.0 <= mi < 32768.0):
                flag |= 1
            t = mi / qi
        out.append(2.0 ** range_exp(t))
    return torch.tensor(out, dtype=torch.float32), flag


def fwd_range_plan(s_all, d_all, row_layer, drow_layer, q, s_prev, d_prev, row0, nrows, drow0, ndrows):
    """s_sc = s_all * q[layer(row), b] for rows [row0, row0+nrows), d_sc = d_all / q[layer(drow), b] for [drow0, drow0+ndrows); layer -1 passes
    through; everything else keeps s_prev / d_prev."""
    s_sc, d_sc = s_prev.clone().to(F64), d_prev.clone().to(F64)
    B = s_all.shape[0]
    for b in range(B):
        for r in range(row0, row0 + nrows):
            l = int(row_layer[r])
            s_sc[b, r] = s_all[b, r].to(F64) * (q[l, b].to(F64) if l >= 0 else 1.0)
        for r in range(drow0, drow0 + ndrows):
            l = int(drow_layer[r])
            d_sc[b, r] = d_all[b, r].to(F64) / (q[l, b].to(F64) if l >= 0 else 1.0)
    return s_sc, d_sc


def scale_check(part, used):
    """(new {unscale, scale}, flag) of absmax_scale_check: m = max |part| (NaN ignored by the max); bit 2 on any non-finite entry; bit 1 when
    m is positive and finite and m * used is outside [2^-8, 2^15); the next scale from m."""
    p = part.to(torch.float32)
    flag = 0 if bool(torch.isfinite(p).all()) else 2
    pa = p.abs()
    pa = pa[~torch.isnan(pa)]
    m = float(pa.max()) if pa.numel() else 0.0
    if m > 0.0 and math.isfinite(m):
        scaled = float(torch.tensor(m, dtype=torch.float32) * torch.tensor(used, dtype=torch.float32))
        if not (2.0 ** -8 <= scaled < 32768.0):
            flag |= 1
    e = range_exp(m)
    return (2.0 ** -e, 2.0 ** e), flag


def contract_values(kmin=-20, kmax=20):
    """2^k, one ulp above and one ulp below, k in [kmin, kmax]  (float32)"""
    out = []
    for k in range(kmin, kmax + 1):
        p = torch.tensor(2.0 ** k, dtype=torch.float32)
        b = p.view(torch.int32)
        out += [(b - 1).view(torch.float32).item(), p.item(), (b + 1).view(torch.float32).item()]
    return torch.tensor(out, dtype=torch.float32)


def contract_ok(m, scale, unscale=None):
    """per element: m * scale in [512, 1024), scale a power of two, unscale * scale == 1"""
    m, scale = m.to(F64), scale.to(F64)
    mant, _ = torch.frexp(scale)
    ok = (m * scale >= 512.0) & (m * scale < 1024.0) & (mant == 0.5)
    if unscale is not None:
        ok &= unscale.to(F64) * scale == 1.0
    return ok
