"""Float64 model of the split-f16 3x3 convolutions (include/oodgan.h, oodgan_conv3x3_f16s) — CPU only, shared by
tests/test_splitf16_ref_cpu.py and tests/test_hip_conv_accuracy.py.

The kernels compute every product of a scaled activation v_x and a scaled weight v_w as hi*hi + hi*lo + lo*hi of the f16 splits
v = hi + lo, accumulate in fp32, and undo the power-of-two scales in the epilogue.  This module holds

  * ``split`` / ``pow2_scale``: the operand rules (round-to-nearest f16, lo from the stored hi; max * 2^e in [512, 1024));
  * ``reference``: the operation itself from the true fp32 operands in float64, with the whole epilogue (in_scale, out_scale,
    noise, bias, leaky-ReLU / PReLU) and the dot epilogue sum_p raw * dotx, taken before out_scale;
  * ``yardstick``: e_model + e32 — the error of the three-term formula evaluated exactly (float64) plus the error of the same
    formula in float32 on the CPU: what a correct kernel may cost, derived from the reference alone;
  * ``sabotages``: the error of three subtly wrong kernels (A: lo(x)*hi(w) lost for one tap, B: both lo terms lost in the last
    16-channel chunk, C: lo(w) lost for the last 8 output channels) — what a test bar must stay well below;
  * decoders (and, for their own test, encoders) of the documented operand layouts: S-form (csrc/sform.hpp), phase-split S-form
    (include/oodgan.h, oodgan_sform_phases_bytes) and the packed split-f16 weights [K/16][9][hi|lo][2][Mp][8];
  * the case table: one row per kernel route of oodgan_conv3x3_f16s, at the smallest shapes that still have a ragged K chunk, a
    ragged M block and a partial tile in each direction.
"""
import functools
import math
from collections import namedtuple

import torch
import torch.nn.functional as F

from oodgan import synth

S1, T2, S2 = 0, 1, 2            # OODGAN_CONV_S1 / _T2 / _S2
UPVB = 3                        # oodgan_upconv_vblur_fform: T2 + Blur(pad=(1,1)), the vertical blur pass folded into two weight sets
SQRT2 = math.sqrt(2.0)
METRICS = ('max', 'rms')


# ------------------------------------------------------------------------------------------------ operand rules
def split(v32):
    """fp32 tensor -> (hi, lo) as float64: hi = RN_f16(v), lo = RN_f16(v - hi) with the STORED hi (v - hi is exact in fp32)."""
    assert v32.dtype == torch.float32
    hi = v32.to(torch.float16)
    lo = (v32.double() - hi.double()).float().to(torch.float16)
    return hi.double(), lo.double()


def split16(v32):
    """The same as f16 tensors (for the layout encoders)."""
    hi = v32.to(torch.float16)
    return hi, (v32.double() - hi.double()).float().to(torch.float16)


def pow2_scale(m):
    """(2^-e, 2^e) with m * 2^e in [512, 1024) — absmax_finish_kernel / the range control; e = 0 for zero or non-finite m."""
    m = float(m)
    e = 0
    if m > 0.0 and math.isfinite(m):
        e = 9 - (math.frexp(m)[1] - 1)          # m = f * 2^ex with f in [0.5, 1): floor(log2 m) = ex - 1
    e = max(-60, min(60, e))
    return 2.0 ** -e, 2.0 ** e


# ------------------------------------------------------------------------------------------------ the operation
def conv_raw(mode, x, w):
    """x (B,K,h,w), w (M,K,3,3) the weight as packed (m = output, k = contraction) -> raw accumulators, any dtype.
    S1: zero pad 1; S2: stride 2, no pad, (2H+1,2W+1) -> (H,W); T2: transposed stride 2, (H,W) -> (2H+1,2W+1)."""
    if mode == S1:
        return F.conv2d(x, w, padding=1)
    if mode == S2:
        return F.conv2d(x, w, stride=2)
    if mode == UPVB:
        return _conv_vfold(x, w)
    # the transposed conv as a plain correlation of the zero-stuffed input with the flipped weight: out[Y,X] = sum x[(Y-ky)/2, (X-kx)/2] *
    # w[ky,kx].  (F.conv_transpose2d scatters column by column: in float32 its sums over K = 512 channels err by 2e-6, five times the
    # error of F.conv2d on the same numbers — an artefact of that routine, which would only widen the yardstick.)
    B, K, H, W = x.shape
    xz = x.new_zeros(B, K, 2 * H + 3, 2 * W + 3)
    xz[:, :, 2:2 * H + 1:2, 2:2 * W + 1:2] = x
    return F.conv2d(xz, torch.flip(w, [2, 3]))


def _conv_vfold(x, wv):
    """The matrix part of the one-pass up-conv (include/oodgan.h, oodgan_upconv_vblur_fform): wv (2,M,K,3,3), one set per output row
    parity; v[2I+py][X] = sum_{d,kx} x[I+d][(X-kx)/2] * wv[py][d+1][kx] — stride 1 along the rows, transposed stride 2 along the
    columns -> (B,M,2H,2W+1)."""
    B, K, H, W = x.shape
    xz = x.new_zeros(B, K, H + 2, 2 * W + 3)
    xz[:, :, 1:H + 1, 2:2 * W + 1:2] = x
    v = x.new_zeros(B, wv.shape[1], 2 * H, 2 * W + 1)
    for py in range(2):
        v[:, :, py::2] = F.conv2d(xz, torch.flip(wv[py], [3]))
    return v


def blur_factors(k2d):
    """(kv, kh) float64 with flip(k2d)[a][b] = kv[a] * kh[b], kh the row of the largest entry (ops.rank_one_factors)."""
    kf = torch.flip(k2d.double(), [0, 1])
    i, j = divmod(int(kf.abs().argmax()), 4)
    return kf[:, j] / kf[i, j], kf[i, :].clone()


def fold_vblur(w, kv):
    """Wv[py][d+1][kx] = sum over (a, ky) with py + a - 1 - ky == 2d of kv[a] * W[ky][kx] (include/oodgan.h), float64."""
    wv = torch.zeros(2, *w.shape, dtype=torch.float64)
    for py in range(2):
        for a in range(4):
            for ky in range(3):
                t = py + a - 1 - ky
                if t % 2 == 0 and -1 <= t // 2 <= 1:
                    wv[py, :, :, t // 2 + 1, :] += kv[a] * w[:, :, ky, :].double()
    return wv


def _epilogue(raw, o, dt):
    """raw accumulators (already unscaled) -> (y, dot) in dtype dt, the order of the kernels' epilogues."""
    if o['mode'] == UPVB:           # the horizontal blur pass runs on the accumulators: y[Y][X] = sum_b kh[b] * v[Y][X+b-1]
        kh = blur_factors(o['k'])[1].to(dt)
        rp = F.pad(raw, (1, 1))
        n = raw.shape[3] - 1
        raw = sum(kh[b] * rp[..., b:b + n] for b in range(4))
    dot = None
    if o['dotx'] is not None:
        dot = (raw * o['dotx'].to(dt)).sum(dim=(2, 3))
    y = raw
    if o['d'] is not None:
        y = y * o['d'].to(dt)[:, :, None, None]
    if o['noise'] is not None:
        y = y + o['nw'].to(dt) * o['noise'].to(dt)
    if o['bias'] is not None:
        y = y + o['bias'].to(dt)[None, :, None, None]
    if o['act'] == 'lrelu':
        y = torch.where(y > 0, y, 0.2 * y) * SQRT2
    elif o['act'] == 'prelu':
        y = torch.where(y > 0, y, o['slope'].to(dt)[None, :, None, None] * y)
    return y, dot


def true_input(o):
    """x * in_scale in float64 (the range scale cancels)."""
    x = o['x'].double()
    return x if o['s'] is None else x * o['s'].double()[:, :, None, None]


def reference(o):
    """(y, dot, raw) in float64 from the true fp32 operands."""
    if o['mode'] == UPVB:
        # the operation as the reference model states it: transposed conv, then the vertical pass of the blur on the (2H+1) x (2W+1)
        # image (the horizontal pass is part of the epilogue) — no folded weights here
        z = conv_raw(T2, true_input(o), o['w'].double() * o['wscale'])
        kv = blur_factors(o['k'])[0]
        zp = F.pad(z, (0, 0, 1, 1))
        n = z.shape[2] - 1
        raw = sum(kv[a] * zp[:, :, a:a + n] for a in range(4))
    else:
        raw = conv_raw(o['mode'], true_input(o), o['w'].double())
    y, dot = _epilogue(raw, o, torch.float64)
    return y, dot, raw


def true_weight(o):
    """float64 weight of conv_raw(o['mode'], ...): w itself, or the two folded sets of the one-pass up-conv."""
    if o['mode'] == UPVB:
        return fold_vblur(o['w'], blur_factors(o['k'])[0]) * o['wscale']
    return o['w'].double()


def staged(o):
    """The fp32 values the kernels split — x * in_scale * in_mul2[1] and w * scale * 2^e — and the product of the unscale factors as
    a tensor that broadcasts over the weight (one power of two per packed set)."""
    x = o['x']
    if o['s'] is not None:
        x = x * o['s'][:, :, None, None]
    un_x = 1.0
    if o['mul2'] is not None:
        x = x * float(o['mul2'][1])
        un_x = float(o['mul2'][0])
    if o['mode'] == UPVB:
        # ops.pack_upconv_vblur: the folded sets rounded to fp32, each packed with scale = wscale (pack_f16s_kernel: w * fp32(2^e * scale))
        w32 = fold_vblur(o['w'], blur_factors(o['k'])[0]).float()
        sc32 = torch.tensor(o['wscale'], dtype=torch.float32)
        p2 = [pow2_scale((w32[py] * sc32).abs().max()) for py in range(2)]
        wv = torch.stack([w32[py] * (sc32 * p2[py][1]) for py in range(2)])
        un = torch.tensor([p2[0][0], p2[1][0]], dtype=torch.float64).view(2, 1, 1, 1, 1) * un_x
        return x, wv, un
    un_w, sc_w = pow2_scale(o['w'].abs().max())
    return x, o['w'] * sc_w, torch.tensor(un_x * un_w, dtype=torch.float64)


def _terms(o):
    """(x hi, x lo, w hi, w lo) in float64 with the power-of-two unscale factors folded into the weight halves (exact, and exact in
    float32 too: scaling by a power of two commutes with every rounding)."""
    xv, wv, un = staged(o)
    xh, xl = split(xv)
    wh, wl = split(wv)
    return xh, xl, wh * un, wl * un


def model_raw(o):
    """hi*hi + hi*lo + lo*hi on the split scaled operands, evaluated in float64 and unscaled."""
    xh, xl, wh, wl = _terms(o)
    m = o['mode']
    return conv_raw(m, xh, wh) + conv_raw(m, xh, wl) + conv_raw(m, xl, wh)


def errors(y, dot, ref_y, ref_dot):
    """{(what, metric): error}: e_max = max|d| / max|ref|, e_rms = rms(d) / rms(ref), for y and (where present) dot."""
    out = {}
    for what, a, b in (('y', y, ref_y), ('dot', dot, ref_dot)):
        if b is None:
            continue
        dlt = a.double() - b
        out[(what, 'max')] = float(dlt.abs().max() / b.abs().max())
        out[(what, 'rms')] = float(dlt.pow(2).mean().sqrt() / b.pow(2).mean().sqrt())
    return out


def yardstick(o, ref=None):
    """{(what, metric): e_model + e32}: the exact three-term formula against the truth, plus the same formula in float32 on the CPU."""
    ref_y, ref_dot, _ = ref if ref is not None else reference(o)
    e_model = errors(*_epilogue(model_raw(o), o, torch.float64), ref_y, ref_dot)
    xh, xl, wh, wl = _terms(o)
    m = o['mode']
    f = torch.float32
    raw32 = conv_raw(m, xh.to(f), wh.to(f)) + conv_raw(m, xh.to(f), wl.to(f)) + conv_raw(m, xl.to(f), wh.to(f))
    e32 = errors(*_epilogue(raw32, o, f), ref_y, ref_dot)
    return {k: e_model[k] + e32[k] for k in e_model}


def sabotages(o, ref=None):
    """{'A' | 'B' | 'C': {(what, metric): error}} of three wrong kernels, each evaluated exactly (float64):
    A: lo(x)*hi(w) dropped for tap (0,0); B: both lo terms dropped in the last 16-channel chunk; C: lo(w) dropped for the last 8
    output channels."""
    ref_y, ref_dot, _ = ref if ref is not None else reference(o)
    xh, xl, wh, wl = _terms(o)
    m = o['mode']
    good = conv_raw(m, xh, wh) + conv_raw(m, xh, wl) + conv_raw(m, xl, wh)
    K, M = wh.shape[-3], wh.shape[-4]           # (M,K,3,3), or (2,M,K,3,3) for the two sets of the one-pass up-conv
    wa = torch.zeros_like(wh)
    wa[..., 0, 0] = wh[..., 0, 0]
    k0 = (K - 1) // 16 * 16
    wc = torch.zeros_like(wl)
    wc[..., M - 8:, :, :, :] = wl[..., M - 8:, :, :, :]
    lost = {'A': conv_raw(m, xl, wa),
            'B': conv_raw(m, xh[:, k0:], wl[..., k0:, :, :]) + conv_raw(m, xl[:, k0:], wh[..., k0:, :, :]),
            'C': conv_raw(m, xh, wc)}
    return {k: errors(*_epilogue(good - v, o, torch.float64), ref_y, ref_dot) for k, v in lost.items()}


# ------------------------------------------------------------------------------------------------ layouts
def sform_dims(C, H, W):
    """csrc/sform.hpp: KC 16-channel blocks, padded plane Hp x Wp (one-pixel border, tile padding)."""
    return (C + 15) // 16, (H + 1 + 7) // 8 * 8 + 2, (W + 1 + 31) // 32 * 32 + 2


def decode_sform(data, B, C, H, W):
    """f16 buffer S[b][kc][Hp][Wp][slot 0..3][8] (slot = hi 0-7, hi 8-15, lo 0-7, lo 8-15; pixel (y,x) at [y+1][x+1]) ->
    (hi, lo, rest): hi / lo (B, 16*KC, H, W) float64 of the image pixels, rest = every other f16 of the buffer (border, tile
    padding), which must be zero.  Channels C .. 16*KC are the padded channels."""
    KC, Hp, Wp = sform_dims(C, H, W)
    v = data.detach().cpu().reshape(B, KC, Hp, Wp, 2, 2, 8)
    planes = v.permute(4, 0, 1, 5, 6, 2, 3).reshape(2, B, KC * 16, Hp, Wp)
    inner = planes[:, :, :, 1:H + 1, 1:W + 1]
    mask = torch.ones(Hp, Wp, dtype=torch.bool)
    mask[1:H + 1, 1:W + 1] = False
    return inner[0].double(), inner[1].double(), planes[:, :, :, mask]


def encode_sform(hi, lo, B, C, H, W):
    """The inverse, written from the address rule of sform.hpp (16-byte unit of slot s of pixel (y,x): (((b*KC + kc)*Hp + y+1)*Wp + x+1)*4 + s)."""
    KC, Hp, Wp = sform_dims(C, H, W)
    out = torch.zeros(B * KC * Hp * Wp * 32, dtype=torch.float16)
    b, c, y, x = torch.meshgrid(torch.arange(B), torch.arange(C), torch.arange(H), torch.arange(W), indexing='ij')
    kc, j = c // 16, c % 16
    unit = (((b * KC + kc) * Hp + y + 1) * Wp + x + 1) * 4
    out[(unit + j // 8) * 8 + j % 8] = hi
    out[(unit + 2 + j // 8) * 8 + j % 8] = lo
    return out


def sp_dims(C, H, W):
    """Phase-split S-form of a (2H+1) x (2W+1) image: KC blocks, four parity planes of Hq x Wq records, no border."""
    return (C + 15) // 16, (H + 7) // 8 * 8 + 2, (W + 31) // 32 * 32 + 2


def decode_sform_phases(data, B, C, H, W):
    """f16 buffer SP[b][kc][py*2+px][Hq][Wq][slot][8], G[py][px][i][j] = x[2i+py][2j+px] -> (hi, lo, rest): hi / lo
    (B, 16*KC, 2H+1, 2W+1) float64, rest = everything that is not a pixel of the image (rows / columns past it and the tile
    padding): zero."""
    KC, Hq, Wq = sp_dims(C, H, W)
    v = data.detach().cpu().reshape(B, KC, 2, 2, Hq, Wq, 2, 2, 8)
    # -> [hl][b][kc][h][j8][i][py][jj][px]: row 2i+py, column 2jj+px
    img = v.permute(6, 0, 1, 7, 8, 4, 2, 5, 3).reshape(2, B, KC * 16, 2 * Hq, 2 * Wq)
    mask = torch.ones(2 * Hq, 2 * Wq, dtype=torch.bool)
    mask[:2 * H + 1, :2 * W + 1] = False
    return img[0, :, :, :2 * H + 1, :2 * W + 1].double(), img[1, :, :, :2 * H + 1, :2 * W + 1].double(), img[:, :, :, mask]


def encode_sform_phases(hi, lo, B, C, H, W):
    """The inverse, from the address rule: record (i,j) of plane ((b*KC + kc)*4 + py*2+px) at 16-byte unit (plane*Hq*Wq + i*Wq + j)*4."""
    KC, Hq, Wq = sp_dims(C, H, W)
    out = torch.zeros(B * KC * 4 * Hq * Wq * 32, dtype=torch.float16)
    b, c, y, x = torch.meshgrid(torch.arange(B), torch.arange(C), torch.arange(2 * H + 1), torch.arange(2 * W + 1), indexing='ij')
    kc, j = c // 16, c % 16
    unit = ((((b * KC + kc) * 4 + (y % 2) * 2 + x % 2) * Hq + y // 2) * Wq + x // 2) * 4
    out[(unit + j // 8) * 8 + j % 8] = hi
    out[(unit + 2 + j // 8) * 8 + j % 8] = lo
    return out


def wpk_dims(K, M):
    return (K + 15) // 16, (M + 63) // 64 * 64


def decode_wpk(data, K, M):
    """f16 buffer [K/16][9 taps][hi|lo][h][Mp][8] (k = 16*chunk + 8*h + j) -> (hi, lo) (Mp, 16*chunks, 3, 3) float64: rows M .. Mp and
    contraction channels K .. 16*chunks are padding."""
    nch, Mp = wpk_dims(K, M)
    v = data.detach().cpu().reshape(nch, 9, 2, 2, Mp, 8)
    w = v.permute(2, 4, 0, 3, 5, 1).reshape(2, Mp, nch * 16, 3, 3)
    return w[0].double(), w[1].double()


def encode_wpk(hi, lo, K, M):
    """The inverse for (M,K,3,3) f16 tensors, from the index rule ((((chunk*9 + tap)*2 + hl)*2 + h)*Mp + m)*8 + j."""
    nch, Mp = wpk_dims(K, M)
    out = torch.zeros(nch * 9 * 2 * 2 * Mp * 8, dtype=torch.float16)
    m, k, tap = torch.meshgrid(torch.arange(M), torch.arange(K), torch.arange(9), indexing='ij')
    base = (k // 16 * 9 + tap) * 2
    h, j = k % 16 // 8, k % 8
    out[(((base + 0) * 2 + h) * Mp + m) * 8 + j] = hi.reshape(M, K, 9)
    out[(((base + 1) * 2 + h) * Mp + m) * 8 + j] = lo.reshape(M, K, 9)
    return out


# ------------------------------------------------------------------------------------------------ the cases
# route: the dispatch counter of oodgan_conv3x3_f16s that must tick; mode; B, K -> M; H x W: the S1 / T2 input size, the S2 OUTPUT size
# (its input is (2H+1) x (2W+1)); src: how the input reaches the kernel ('nchw' fp32, 'sform', 'phases', 'padtl' = phase-split from
# the unpadded tensor of a padding-1 conv, 'fform'); calls: which of the instances below the route has; tun: dispatch tunables.
Case = namedtuple('Case', 'id route mode B K M H W src calls tun')
ALL4 = ('fwd', 'plain', 'dx', 'dx12')
S2ALL = ('fwd_prelu', 'plain', 'dx', 'dx12')
CASES = [
    Case('s1pp-24-40', 's1pp', S1, 2, 24, 40, 9, 37, 'nchw', ALL4, {}),
    Case('s1pp-512-64', 's1pp', S1, 1, 512, 64, 8, 8, 'nchw', ALL4, {}),
    Case('t2gen-24-40', 't2gen', T2, 2, 24, 40, 9, 37, 'nchw', ('plain',), {}),
    Case('t2gen-512-64', 't2gen', T2, 1, 512, 64, 8, 8, 'nchw', ('plain',), {}),
    Case('s2gen-24-40', 's2gen', S2, 2, 24, 40, 9, 37, 'nchw', S2ALL, {}),
    Case('s2gen-512-64', 's2gen', S2, 1, 512, 64, 8, 8, 'nchw', S2ALL, {}),
    Case('s1v2-24-40', 's1v2', S1, 2, 24, 40, 9, 37, 'sform', ALL4, {}),
    Case('s1v2-40-24', 's1v2', S1, 2, 40, 24, 10, 36, 'sform', ALL4, {}),
    Case('t2v2-24-40', 't2v2', T2, 2, 24, 40, 9, 37, 'sform', ('plain',), {}),
    Case('s2v2-40-24', 's2v2', S2, 2, 40, 24, 9, 37, 'phases', S2ALL, {}),
    Case('strip-24-20', 'strip', S1, 2, 24, 20, 13, 45, 'sform', ALL4, {}),
    Case('strip-32-32', 'strip', S1, 1, 32, 32, 7, 100, 'sform', ALL4, {}),
    Case('s1big-80-96', 's1big', S1, 1, 80, 96, 17, 33, 'sform', ALL4, {'s1_big_min_items': 1}),
    Case('t2big-48-80', 't2big', T2, 1, 48, 80, 9, 33, 'sform', ('plain',), {'t2_big_min_items': 1}),
    Case('s2big-48-80', 's2big', S2, 1, 48, 80, 9, 33, 'phases', ('plain', 'dx', 'dx12'), {'s2_big_min_items': 0}),
    Case('s2big-48-80-fwd', 's2big', S2, 1, 48, 80, 9, 33, 'padtl', ('fwd_prelu',), {'s2_big_min_items': 0}),
    Case('tiny-s1-512-64', 'tiny', S1, 2, 512, 64, 4, 4, 'sform', ALL4, {}),
    Case('tiny-s1-64-64', 'tiny', S1, 2, 64, 64, 8, 8, 'sform', ALL4, {}),
    Case('tiny-s2-512-64', 'tiny', S2, 2, 512, 64, 4, 4, 'phases', S2ALL, {}),
    Case('tiny-s2-64-64', 'tiny', S2, 2, 64, 64, 8, 8, 'phases', S2ALL, {}),
    Case('stripx-32-32', 'stripx', S1, 1, 32, 32, 8, 32, 'fform', ('fwd', 'plain'), {}),
    # the smallest shape oodgan_upconv_vblur_supported accepts (K % 16 == 0, M % 32 == 0, H >= 4, W >= 30); output (2H) x (2W)
    Case('upvb-48-32', 'upvb', UPVB, 2, 48, 32, 4, 30, 'sform', ('fwd', 'plain'), {}),
]
CASE_IDS = [c.id for c in CASES]

# Calls of a CORRECT route that measure above 4 x yardstick on the MI355X: (case, precision, call, what, metric) -> measured error; their
# bar is 2 x that value, and never more than 1/10 of the call's smallest sabotage error (tests/test_splitf16_ref_cpu.py holds the cap).
# All of them are e_max at K = 512 through the kernels that walk the whole contraction in ONE accumulator per output: 9 * 512 / 2 = 2304
# dependent fp32 additions in the exact-fp32 kernel (v_mfma_f32_32x32x2_f32), 3 * 9 * 512 / 16 = 864 in the split-f16 one, against the
# blocked sums of the CPU's float32 conv.  The exact-fp32 kernel — no split at all — errs MORE than the split-f16 kernel on the same data,
# the transposed conv (a quarter of the taps per output) less, the K-split skinny-GEMM kernel at the same 512 -> 64 shape sits at half the
# yardstick, and e_rms stays inside 4 x yardstick everywhere: the length of the fp32 chain, not a lost term (a sabotage costs >= 4e-5).
MEASURED_ABOVE = {
    ('s1pp-512-64', 'f16s', 'fwd', 'y', 'max'): 1.24e-6,
    ('s1pp-512-64', 'f32', 'fwd', 'y', 'max'): 1.58e-6,
    ('s1pp-512-64', 'f32', 'plain', 'y', 'max'): 1.72e-6,
    ('s1pp-512-64', 'f32', 'dx', 'y', 'max'): 1.72e-6,
    ('s1pp-512-64', 'f32', 'dx12', 'y', 'max'): 1.72e-6,
    ('t2gen-512-64', 'f32', 'plain', 'y', 'max'): 1.50e-6,
    ('s2gen-512-64', 'f32', 'fwd_prelu', 'y', 'max'): 1.63e-6,
    ('s2gen-512-64', 'f32', 'plain', 'y', 'max'): 1.72e-6,
    ('s2gen-512-64', 'f32', 'dx', 'y', 'max'): 1.72e-6,
    ('s2gen-512-64', 'f32', 'dx12', 'y', 'max'): 1.72e-6,
    ('s2gen-512-64', 'f32', 'dx', 'dot', 'max'): 1.39e-6,
    ('s2gen-512-64', 'f32', 'dx12', 'dot', 'max'): 1.39e-6,
}
BAR_FACTOR = 4.0


def bar(cid, prec, call, key, Y):
    """The bar of one figure: 4 x yardstick, or 2 x the measured value of a correct route recorded above."""
    m = MEASURED_ABOVE.get((cid, prec, call) + tuple(key))
    return BAR_FACTOR * Y[key] if m is None else 2.0 * m


def in_hw(c):
    return (2 * c.H + 1, 2 * c.W + 1) if c.mode == S2 else (c.H, c.W)


def out_hw(c):
    if c.mode == UPVB:
        return 2 * c.H, 2 * c.W
    return (2 * c.H + 1, 2 * c.W + 1) if c.mode == T2 else (c.H, c.W)


@functools.lru_cache(maxsize=None)
def analysis(cid, call):
    """(operands, reference, yardstick, sabotages) of one call of one case, computed once per session and shared by the tests (read only)."""
    o = operands(CASES[CASE_IDS.index(cid)], call)
    ref = reference(o)
    return o, ref, yardstick(o, ref), sabotages(o, ref)


def operands(c, call):
    """The seeded operands of one call of one case (fp32 CPU tensors; absent terms are None):
      'fwd'        out_scale, per-sample noise, bias, leaky-ReLU            'fwd_prelu'  out_scale, bias, PReLU (the stride-2 forward use)
      'plain'      out_scale only
      'dx'         the input-gradient instance: dotx, no noise / bias / activation
      'dx12'       the same with data of overall scale 2^-12 and the in_mul2 pair pow2_scale gives for it
    Styles are N(1, 0.3), weights N(0, 1/sqrt(9K)).  'padtl': x is the (2H+1) x (2W+1) image whose top row and left column are the
    zero padding; o['x_unpadded'] is the tensor the producer gets."""
    def g(name, shape, seed, std=1.0, mean=0.0):
        return synth.normal(f'convacc.{c.id}.{name}', shape, seed, std, mean)
    B, K, M = c.B, c.K, c.M
    hi_, wi_ = in_hw(c)
    ho, wo = out_hw(c)
    o = dict(mode=c.mode, s=g('s', (B, K), 2, 0.3, 1.0), w=g('w', (M, K, 3, 3), 3, 1.0 / math.sqrt(9 * K)), d=g('d', (B, M), 4, 0.3, 1.0),
             noise=None, nw=None, bias=None, slope=None, act='none', dotx=None, mul2=None, x_unpadded=None, k=None, wscale=None)
    if c.mode == UPVB:      # as the engine hands the layer over: the raw N(0,1) weight, its 1/sqrt(9K) as the packing scale, Blur's kernel
        k1 = torch.tensor([1., 3., 3., 1.])
        o.update(w=g('w', (M, K, 3, 3), 3), wscale=1.0 / math.sqrt(9 * K), k=(k1[:, None] * k1[None, :] / 64 * 4).contiguous(), d=o['d'].abs())
    if c.src == 'padtl':
        xu = g('x', (B, K, hi_ - 1, wi_ - 1), 1)
        o['x_unpadded'], o['x'] = xu, F.pad(xu, (1, 0, 1, 0))
    else:
        o['x'] = g('x', (B, K, hi_, wi_), 1)
    if call == 'fwd':
        o.update(noise=g('nz', (B, 1, ho, wo), 5), nw=torch.tensor([0.37]), bias=g('b', (M,), 6, 0.5), act='lrelu')
    elif call == 'fwd_prelu':
        o.update(bias=g('b', (M,), 6, 0.5), act='prelu', slope=0.05 + 0.2 * synth.uniform(f'convacc.{c.id}.slope', (M,), 7))
    elif call in ('dx', 'dx12'):
        o['dotx'] = g('dotx', (B, M, ho, wo), 8)
        if call == 'dx12':
            o['x'] = o['x'] * 2.0 ** -12
            o['mul2'] = pow2_scale((o['x'] * o['s'][:, :, None, None]).abs().max())
    else:
        assert call == 'plain', call
    return o
