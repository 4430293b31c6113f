"""Float64 references of the streaming kernels around the convolutions: ToRGB and rgb_finish (csrc/torgb.hip), bias + noise + leaky ReLU forward
and backward, the merged activation / ToRGB backward and feature_modulation (csrc/elementwise.hip), and the part of LPIPS after the convolutions
(csrc/lpips.hip: prep, img_grad, head, add_mask, finish).  Written from the formulas in the kernels' header comments in plain torch.

Where a kernel uses a float32 constant (0.2f, kSqrt2, 1.f / scale3[c], float(1 / sqrt(Ci)), 1e-10f) the reference uses that float32 value converted
to float64, so the constant's own rounding is not counted as kernel error.

tests/test_stream_ref_cpu.py checks the references against autograd and the oracle, and the integer data sets against the exact regime;
tests/test_hip_torgb.py, tests/test_hip_act_kernels.py and tests/test_hip_lpips_tail.py compare the kernels with them."""
import math

import numpy as np
import torch

F64 = torch.float64
U = 2.0 ** -24          # unit roundoff of float32


def f32(v):
    """the float32 nearest to v, as a Python float (what a kernel holds after `float c = v`)"""
    return float(np.float32(v))


def f32_mul(a, b):
    return float(np.float32(a) * np.float32(b))


def f32_div(a, b):
    return float(np.float32(a) / np.float32(b))


def fits_float32(t64):
    """every entry of the float64 tensor is itself a float32 number"""
    return bool(torch.equal(t64.to(torch.float32).to(F64), t64))


def exact_any_order(terms64):
    """terms (..., n) float64.  Sufficient for a float32 sum of each row to be exact in ANY order and grouping: every term is a multiple of
    g = 2^k (the smallest power of two at or below the smallest non-zero |term| that divides them all) and sum |terms| <= 2^24 g, so every partial
    sum of every sub-set is a multiple of g below 2^24 g."""
    t = terms64.reshape(-1, terms64.shape[-1])
    nz = t[t != 0].abs()
    if nz.numel() == 0:
        return True
    g = 2.0 ** math.floor(math.log2(nz.min().item()))
    for _ in range(60):
        if bool(torch.equal(torch.round(t / g) * g, t)):
            break
        g /= 2.0
    else:
        return False
    return bool((t.abs().sum(1) <= 2.0 ** 24 * g).all())


# ----------------------------------------------------------------------------- ToRGB
def torgb_scale(Ci):
    """float(1 / sqrt(Ci)), the value the wrapper passes"""
    return f32(1.0 / math.sqrt(Ci))


def upsample_skip(skip, k4):
    """upfirdn2d(skip, k4, up=2, pad=(2, 1)) as a gather (torgb.hip, SkipTaps): out[Y, X] = sum_{ky,kx} kflip[ky,kx] * z[Y+ky-2, X+kx-2], z the
    zero-stuffed skip (z[2i, 2j] = skip[i, j]), kflip[ky][kx] = k4[3-ky][3-kx].  Returns (value, sum of |terms|)."""
    B, C, h, w = skip.shape
    k = k4.to(F64)
    z = torch.zeros(B, C, 2 * h + 3, 2 * w + 3, dtype=F64)          # pad 2 before, 1 after
    z[:, :, 2:2 * h + 2:2, 2:2 * w + 2:2] = skip.to(F64)
    out = torch.zeros(B, C, 2 * h, 2 * w, dtype=F64)
    mag = torch.zeros_like(out)
    for ky in range(4):
        for kx in range(4):
            win = z[:, :, ky:ky + 2 * h, kx:kx + 2 * w]
            out += k[3 - ky, 3 - kx] * win
            mag += k[3 - ky, 3 - kx].abs() * win.abs()
    return out, mag


def torgb(x, w, s, bias=None, skip=None, k4=None, scale=None):
    """y[b,k] = scale * sum_c w[k,c] s[b,c] x[b,c] + bias[k] + upfirdn2d(skip, k4, up=2, pad=(2,1)); w (3,Ci), s (B,Ci).
    Returns (y, mag): mag = the same expression with every term replaced by its absolute value."""
    B, Ci, H, W = x.shape
    scale = torgb_scale(Ci) if scale is None else scale
    ws = scale * w.to(F64)[None] * s.to(F64)[:, None, :]          # (B,3,Ci)
    y = torch.einsum('bkc,bchw->bkhw', ws, x.to(F64))
    mag = torch.einsum('bkc,bchw->bkhw', ws.abs(), x.to(F64).abs())
    if bias is not None:
        y = y + bias.to(F64).view(1, 3, 1, 1)
        mag = mag + bias.to(F64).abs().view(1, 3, 1, 1)
    if skip is not None:
        u, um = upsample_skip(skip, k4)
        y, mag = y + u, mag + um
    return y, mag


def rgb_finish(parts, bias=None, skip=None, k4=None):
    """parts (nparts,B,3,H,W) summed in the order of their index + bias + the up-sampled skip.  Returns (y, mag)."""
    p = parts.to(F64)
    y, mag = p[0].clone(), p[0].abs()
    for q in range(1, p.shape[0]):
        y, mag = y + p[q], mag + p[q].abs()
    if bias is not None:
        y = y + bias.to(F64).view(1, 3, 1, 1)
        mag = mag + bias.to(F64).abs().view(1, 3, 1, 1)
    if skip is not None:
        u, um = upsample_skip(skip, k4)
        y, mag = y + u, mag + um
    return y, mag


# ----------------------------------------------------------------------------- bias + noise + leaky ReLU
class ActConsts:
    """the four factors of lrelu(slope) * scale and its inverse.  kernel(): as act_bwd_fused_kernel holds them (kSqrt2, 0.2f * kSqrt2 and
    1.f / each, all float32); ideal(): the same from exact arithmetic, for the comparison with autograd."""

    def __init__(self, pos, neg, inv_pos, inv_neg):
        self.pos, self.neg, self.inv_pos, self.inv_neg = pos, neg, inv_pos, inv_neg

    @staticmethod
    def kernel():
        pos = f32(math.sqrt(2.0))
        neg = f32_mul(f32(0.2), pos)
        return ActConsts(pos, neg, f32_div(1.0, pos), f32_div(1.0, neg))

    @staticmethod
    def ideal(slope, scale):
        return ActConsts(scale, slope * scale, 1.0 / scale, 1.0 / (slope * scale))


def _plane(t, B, C, shape):
    """(B or 1, 1, ...) noise broadcast to x's shape"""
    return t.to(F64).reshape((t.shape[0], 1) + tuple(shape[2:])).expand(shape)


def bias_noise_act_pre(x, bias=None, noise=None, noise_weight=None):
    """x + nw * noise + bias[c]: (value, sum of |terms|); nw = 1 when noise is given without a weight"""
    x64 = x.to(F64)
    pre, mag = x64.clone(), x64.abs()
    if noise is not None:
        nw = 1.0 if noise_weight is None else float(noise_weight.reshape(-1)[0])
        n = _plane(noise, x.shape[0], x.shape[1], x.shape)
        pre, mag = pre + nw * n, mag + abs(nw) * n.abs()
    if bias is not None:
        bshape = (1, -1) + (1,) * (x.ndim - 2)
        pre, mag = pre + bias.to(F64).view(bshape), mag + bias.to(F64).abs().view(bshape)
    return pre, mag


def bias_noise_act(x, bias=None, noise=None, noise_weight=None, slope=0.2, scale=math.sqrt(2.0)):
    """y = lrelu(x + nw * noise + bias[c], slope) * scale with slope and scale rounded to float32"""
    pre, _ = bias_noise_act_pre(x, bias, noise, noise_weight)
    sl, sc = f32(slope), f32(scale)
    return torch.where(pre > 0, pre, pre * sl) * sc


def bias_act_bwd(gy, y, slope=0.2, scale=math.sqrt(2.0)):
    """gx = gy * (y > 0 ? scale : slope * scale); gbias[c] = sum_{b,p} gx"""
    sl, sc = f32(slope), f32(scale)
    g = gy.to(F64)
    gx = torch.where(y.to(F64) > 0, g * sc, g * (sl * sc))
    return gx


def channel_sum(gx):
    """(B,C,...) -> (C,): (sum, sum of absolute values)"""
    g = gx.to(F64).reshape(gx.shape[0], gx.shape[1], -1)
    return g.sum((0, 2)), g.abs().sum((0, 2))


ACT_CHUNK = 4096          # kActChunk


def act_bwd_fused(out, g_feat=None, noise=None, noise_weight=None, bias=None, g_rgb=None, w_rgb=None, s_rgb=None, rgb_scale=None, dscale=None,
                  consts=None):
    """The quantities act_bwd_fused_kernel returns, per element and per (b,c) (elementwise.hip):
        t_px = sum_k (w_rgb[k,c] * rgb_scale) * g_rgb[b,k,p]          g = g_feat + s_rgb[b,c] * t_px
        g_pre = g * (out > 0 ? pos : neg)                              y_cv = (out > 0 ? out * inv_pos : out * inv_neg) - nw * noise - bias[c]
        r[b,c] = sum_p g_pre * y_cv          t[b,c] = sum_p out * t_px          part_max[b,c,chunk] = max_p |g_pre| * |dscale[b,c]|
    out (B,C,H,W) or (B,C,HW).  Returns a dict with g_pre, r, t (None without the RGB branch), part_max, and the magnitudes g_pre_mag (|g_feat| +
    |s_rgb| sum |w g_rgb|, times the factor), r_mag (sum |g_pre| (|out inv| + |nw noise| + |bias|)) and t_mag (sum |out| sum_k |w g_rgb|)."""
    k = ActConsts.kernel() if consts is None else consts
    B, C = out.shape[0], out.shape[1]
    o = out.to(F64).reshape(B, C, -1)
    HW = o.shape[2]
    gf = torch.zeros_like(o) if g_feat is None else g_feat.to(F64).reshape(B, C, HW)
    tpx = torch.zeros_like(o)
    tpx_mag = torch.zeros_like(o)
    sr = torch.zeros(B, C, dtype=F64)
    if g_rgb is not None:
        rgb_scale = torgb_scale(C) if rgb_scale is None else rgb_scale
        wk = w_rgb.to(F64).reshape(3, C) * rgb_scale
        gr = g_rgb.to(F64).reshape(B, 3, HW)
        tpx = torch.einsum('kc,bkp->bcp', wk, gr)
        tpx_mag = torch.einsum('kc,bkp->bcp', wk.abs(), gr.abs())
        sr = s_rgb.to(F64)
    g = gf + sr[:, :, None] * tpx
    g_mag = gf.abs() + sr.abs()[:, :, None] * tpx_mag
    pos = o > 0
    fac = torch.where(pos, torch.full_like(o, k.pos), torch.full_like(o, k.neg))
    gp = g * fac
    lin = torch.where(pos, o * k.inv_pos, o * k.inv_neg)
    ycv, ycv_mag = lin.clone(), lin.abs()
    if noise is not None:
        nw = 1.0 if noise_weight is None else float(noise_weight.reshape(-1)[0])
        n = noise.to(F64).reshape(noise.shape[0], 1, HW).expand(B, C, HW)
        ycv, ycv_mag = ycv - nw * n, ycv_mag + abs(nw) * n.abs()
    if bias is not None:
        ycv, ycv_mag = ycv - bias.to(F64).view(1, C, 1), ycv_mag + bias.to(F64).abs().view(1, C, 1)
    nchunk = (HW + ACT_CHUNK - 1) // ACT_CHUNK
    ds = torch.ones(B, C, dtype=F64) if dscale is None else dscale.to(F64).abs()
    pm = torch.stack([gp[:, :, c * ACT_CHUNK:(c + 1) * ACT_CHUNK].abs().amax(2) for c in range(nchunk)], 2) * ds[:, :, None]
    return dict(g_pre=gp.reshape(out.shape), g_pre_mag=(g_mag * fac).reshape(out.shape), r=(gp * ycv).sum(2), r_mag=(gp.abs() * ycv_mag).sum(2),
                r_mag_full=(g_mag * fac * ycv_mag).sum(2),
                t=None if g_rgb is None else (o * tpx).sum(2), t_mag=(o.abs() * tpx_mag).sum(2), part_max=pm, y_cv=ycv.reshape(out.shape))


def part_max_of(g_pre32, dscale32=None):
    """part_max from the kernel's OWN float32 g_pre: float32(max_chunk |g_pre| * |dscale|), one float32 product"""
    B, C = g_pre32.shape[0], g_pre32.shape[1]
    g = g_pre32.reshape(B, C, -1).abs()
    nchunk = (g.shape[2] + ACT_CHUNK - 1) // ACT_CHUNK
    m = torch.stack([g[:, :, c * ACT_CHUNK:(c + 1) * ACT_CHUNK].amax(2) for c in range(nchunk)], 2)
    if dscale32 is not None:
        m = (m * dscale32.abs().to(torch.float32)[:, :, None]).to(torch.float32)
    return m


# ----------------------------------------------------------------------------- feature_modulation
def feature_modulation(x, c0, c1, mode):
    """SFT y = x (1 + c0) + c1; ADD y = x + c1; FUSE y = x + c1 sigmoid(c0).  Conditions broadcast to x.  Returns (y, sum of |terms|)."""
    x64 = x.to(F64)
    c1 = c1.to(F64).expand_as(x64)
    if mode == 'ADD':
        return x64 + c1, x64.abs() + c1.abs()
    c0 = c0.to(F64).expand_as(x64)
    if mode == 'SFT':
        return x64 * (1.0 + c0) + c1, x64.abs() * (1.0 + c0.abs()) + c1.abs()
    sg = 1.0 / (1.0 + torch.exp(-c0))
    return x64 + c1 * sg, x64.abs() + c1.abs() * sg


# ----------------------------------------------------------------------------- LPIPS tail
def lpips_prep(img, a, b0, shift3, scale3):
    """v = (a x + b0 - shift_c) * (1.f / scale_c), zero pad 2, 4x4 space-to-depth: out (B, 48, H/4+1, W/4+1), channel = c*16 + dy*4 + dx,
    out[b, ch, Y, X] = v[b, c, 4Y + dy - 2, 4X + dx - 2].  Returns (out, mag, inside): mag = (|a x| + |b0| + |shift|) |1/scale|, inside = the
    cells that hold a pixel (the others are pad and exactly zero)."""
    B, _, H, W = img.shape
    x = img.to(F64)
    sh = torch.tensor([f32(v) for v in shift3], dtype=F64).view(1, 3, 1, 1)
    inv = torch.tensor([f32_div(1.0, f32(v)) for v in scale3], dtype=F64).view(1, 3, 1, 1)
    a, b0 = f32(a), f32(b0)
    v = (a * x + b0 - sh) * inv
    vm = ((a * x).abs() + abs(b0) + sh.abs()) * inv.abs()
    return _space_to_depth(v, H, W), _space_to_depth(vm, H, W), _space_to_depth(torch.ones_like(v), H, W) > 0


def _space_to_depth(v, H, W):
    B = v.shape[0]
    Hs, Ws = H // 4 + 1, W // 4 + 1
    p = torch.zeros(B, 3, 4 * Hs, 4 * Ws, dtype=F64)
    p[:, :, 2:2 + H, 2:2 + W] = v
    # p[b, c, 4Y + dy, 4X + dx] -> out[b, c*16 + dy*4 + dx, Y, X]
    return p.view(B, 3, Hs, 4, Ws, 4).permute(0, 1, 3, 5, 2, 4).reshape(B, 48, Hs, Ws)


def lpips_img_grad_factors(a, coef, scale3):
    """k_c = coef * a / scale_c in float32, the way the entry point forms it on the host"""
    return [f32_div(f32_mul(f32(coef), f32(a)), f32(v)) for v in scale3]


def lpips_img_grad(g48, gimg0, a, coef, scale3):
    """gimg0 + k_c * depth_to_space(g48): the adjoint of lpips_prep (without its constants b0 and shift), added to what gimg held"""
    B, _, H, W = gimg0.shape
    Hs, Ws = H // 4 + 1, W // 4 + 1
    k = torch.tensor(lpips_img_grad_factors(a, coef, scale3), dtype=F64).view(1, 3, 1, 1)
    p = g48.to(F64).view(B, 3, 4, 4, Hs, Ws).permute(0, 1, 4, 2, 5, 3).reshape(B, 3, 4 * Hs, 4 * Ws)
    return gimg0.to(F64) + k * p[:, :, 2:2 + H, 2:2 + W]


HEAD_PIX = 32          # kHeadPix
HEAD_CG = 8            # kHeadCg


def lpips_head(f0, n1=None, w=None, coef=1.0, mode=0):
    """One tap of LPIPS (lpips.hip).  f0, n1 (B,C,HW); w (C,).
      mode 0: out = f / (sqrt(sum_c f^2) + 1e-10f)
      mode 1: d = sum_c w_c (n0_c - n1_c)^2, part[b, blk] = sum of d over the 32 pixels of block blk;
              out = coef (r e_c - (sum_k e_k f_k) r^2 / s f_c), e_c = 2 w_c (n0_c - n1_c), s = |f|, r = 1 / (s + eps); the second term is DROPPED where s == 0
      mode 2: mode 1 with out multiplied by (f > 0)
    Returns dict(out, out_mag, part, part_mag, d): the magnitudes are the expressions with every term, also those of n0 - n1, made positive."""
    f = f0.to(F64)
    B, C, HW = f.shape
    eps = f32(1e-10)
    s = torch.sqrt((f * f).sum(1, keepdim=True))
    r = 1.0 / (s + eps)
    if mode == 0:
        return dict(out=f * r, out_mag=(f * r).abs())
    coef = f32(coef)
    n = n1.to(F64)
    wv = w.to(F64).view(1, C, 1)
    df = f * r - n
    dfm = (f * r).abs() + n.abs()
    d = (wv * df * df).sum(1)
    dm = (wv.abs() * dfm * dfm).sum(1)
    dotk = (2.0 * wv * df * f).sum(1, keepdim=True)
    dotm = (2.0 * wv.abs() * dfm * f.abs()).sum(1, keepdim=True)
    safe = torch.where(s > 0, s, torch.ones_like(s))
    q = torch.where(s > 0, dotk * r * r / safe, torch.zeros_like(s))
    qm = torch.where(s > 0, dotm * r * r / safe, torch.zeros_like(s))
    out = coef * (2.0 * wv * df * r - q * f)
    out_mag = abs(coef) * (2.0 * wv.abs() * dfm * r + qm * f.abs())
    if mode == 2:
        out = torch.where(f > 0, out, torch.zeros_like(out))
    nblk = (HW + HEAD_PIX - 1) // HEAD_PIX
    pad = nblk * HEAD_PIX - HW
    part = torch.nn.functional.pad(d, (0, pad)).view(B, nblk, HEAD_PIX).sum(2)
    part_mag = torch.nn.functional.pad(dm, (0, pad)).view(B, nblk, HEAD_PIX).sum(2)
    return dict(out=out, out_mag=out_mag, part=part, part_mag=part_mag, d=d)


def head_roundings(C, what):
    """Number of float32 roundings on the longest path of lpips_head_kernel, first order, in units of 2^-24 times the magnitude lpips_head returns.
    cC = ceil(C / 8) + 8: `s2 += v * v` over a group's channels (a product and an addition each: counted ceil(C/8) + 1 since the terms are
    positive and a relative error does not grow with them) and `s2 += red[0][k][pl]` over the 8 groups.
      s2 relative: cC;  s = sqrtf(s2): cC/2 + 1;  r = 1.f / (s + 1e-10f): E_r = cC/2 + 3  (sqrtf, the addition, the division: one rounding each,
      the library is built with correctly rounded sqrt and division)
      mode 0, `fb * r`: E_r + 1
      df = f * r - n1: (E_r + 2) (|f r| + |n1|)
      d = sum w df df: 2 (E_r + 2) + 2 products + cC for the two-level sum; part adds the 5 `v += __shfl_xor` of the block sum
      out = coef * (2.f * w * df * r - q * f), q = dotk * r * r / s:
         first term (E_r + 2) + (E_r + 4);  second term (E_r + 2) + 3 [2 w df f] + cC [sum] + 2 E_r + (cC/2 + 1) + 3 [r r / s] + 2 [q f, coef];  1 for the subtraction"""
    cC = -(-C // HEAD_CG) + 8
    Er = cC / 2 + 3
    if what == 'norm':
        return Er + 1
    if what == 'part':
        return 2 * (Er + 2) + 2 + cC + 5
    first = 2 * Er + 6
    second = (Er + 2) + 3 + cC + 2 * Er + (cC / 2 + 1) + 3 + 2
    return max(first, second) + 1


def add_mask(y, add, mask):
    """(y + add) where mask > 0, +0 elsewhere, in the dtype of y (float32: the kernel's own arithmetic, one addition)"""
    return torch.where(mask > 0, y + add, torch.zeros_like(y))


def lpips_finish(parts, hw):
    """lpips[b] = sum_t (sum_j part_t[b, j]) * (1.f / hw_t); parts: list of (B, nparts_t).  Returns (value, sum of |terms|)."""
    tot = torch.zeros(parts[0].shape[0], dtype=F64)
    mag = torch.zeros_like(tot)
    for p, h in zip(parts, hw):
        inv = f32_div(1.0, float(h))
        tot = tot + p.to(F64).sum(1) * inv
        mag = mag + p.to(F64).abs().sum(1) * inv
    return tot, mag
