"""Float64 model of the backward producers (csrc/bwd_producers.hip: oodgan_act_bwd_sform, oodgan_act_bwd_sform_f,
oodgan_act_bwd_blurT_sform_phases[_hi]) and of the two-pass root oodgan_blurT_to_sform_phases — CPU only, shared by
tests/test_bwd_producer_ref_cpu.py and tests/test_hip_bwd_producers_f64.py.  Written from the semantics in the header comment of
bwd_producers.hip and include/oodgan.h, not from the kernels:

    t      = sum_k (w_rgb[k,c] * rgb_scale) * g_rgb[b,k]                      (ToRGB branch; 0 without one)
    g      = g_feat + s_rgb[b,c] * t
    g_pre  = g * (out > 0 ? sqrt2 : 0.2 * sqrt2)                               (out == 0 and -0 take the negative branch)
    r[b,c] = sum g_pre * ((out > 0 ? out / sqrt2 : out / (0.2 * sqrt2)) - nw * noise - bias)
    t_sum  = sum out * t
    m      = max |g_pre| * |d[b,c]|
    PRE (out = None): g_pre = g_feat, r = -sum g_pre * (nw * noise + bias) + scale[b,c] * sum dot_part[b,c,:]
    plain layers:        record value g_pre * d * mul2[1]
    up-sampling layers:  g2[Y,X] = sum_{a,b} kflip[a][b] * g_pre[Y+a-2][X+b-2], Y in 0..2H, X in 0..2W, zero outside; record g2 * d * mul2[1]

This module holds

  * ``chain``: that operation in any dtype — float64 is the reference, float32 (with the fp32 constants of csrc/common.hpp) the model;
  * ``record_values``: the f16 split of the fp32 record value, hi = f16(v), lo = f16(v - hi), value hi + lo (hi alone for hi-only records);
  * ``errors`` / ``yardstick``: e_max = max|d| / max|ref| and e_rms = rms(d) / rms(ref) on the record values, on r and on t_sum, the relative
    error of m; the yardstick is the float32 model against the float64 reference, BAR_FACTOR = 4 (one factor 2 for FMA contraction, one for
    another summation order).  m is ONE number: its yardstick is at least 2^-24, the half-ulp of a single fp32 rounding, so that a lucky
    exact model value does not make the bar zero.  hi-only records have no fp32-class bar by design; their figure is
    ('hi', 'excess') = max (|hi - ref| - 2^-11 |ref|) / max|ref| (what exceeds the half-ulp of f16), held to 4 x the e_max yardstick of the
    full records;
  * ``sabotages``: seven subtly wrong kernels evaluated exactly (float64), each where its branch exists:
      A  vertical taps of the rank-one path reversed                          B  the right halo column of the first strip read as zero
      C  lo half missing in the column X = 2W (position j = W)                D  the first g row of segment 1 counted in no segment's r
      E  lo half missing in the phase plane (py, px) = (1, 1)                 F  |d| left out of the recorded maximum
      G  (plain layers) lo half of channels 8-15 missing: S-form slot 3
  * decoders and encoders of the 32-byte hi-only phase records and of the F-form, beside those of splitf16_ref;
  * the launcher's geometry re-stated (``strip_geometry``, ``tile_geometry``, ``plain_chunks``) and the case table.
"""
import functools
import math
from collections import namedtuple

import torch
import torch.nn.functional as F

from oodgan import synth
from splitf16_ref import decode_sform, decode_sform_phases, pow2_scale, sp_dims, split  # noqa: F401  (re-exported for the tests)

SQRT2 = math.sqrt(2.0)
BAR_FACTOR = 4.0
M_FLOOR = 2.0 ** -24            # half an ulp of fp32, relative: the least one rounding may cost (yardstick floor of the single number m)
HALF_ULP_F16 = 2.0 ** -11
# the fp32 constants of csrc/common.hpp (kSqrt2, 0.2f * kSqrt2, kInvPos, kInvNeg)
_f32 = lambda v: torch.tensor(v, dtype=torch.float32)
K_SQRT2 = _f32(1.4142135623730951)
K_NEG = _f32(0.2) * K_SQRT2
K_INVPOS = _f32(1.0) / K_SQRT2
K_INVNEG = _f32(1.0) / K_NEG


# ------------------------------------------------------------------------------------------------ blur kernels
def blur_kernel(kind):
    """'r1': outer([1,2,4,1], [1,3,3,2]) normalised to sum 4 — rank one, neither palindromic nor symmetric (the vertical taps are powers of
    two, so the kernels' own rank-one tests hold exactly in fp32); 'gen': the same with two entries moved, no longer rank one; 'sym':
    the generator's [1,3,3,1] x [1,3,3,1]."""
    if kind == 'sym':
        k1 = torch.tensor([1., 3., 3., 1.])
        return (k1[:, None] * k1[None, :] / 64 * 4).contiguous()
    k = torch.tensor([1., 2., 4., 1.])[:, None] * torch.tensor([1., 3., 3., 2.])[None, :]
    k = k / k.sum() * 4.0
    if kind == 'gen':
        k[1, 2] += 0.37
        k[3, 0] -= 0.11
    else:
        assert kind == 'r1', kind
    return k.contiguous()


def is_rank_one_strip(k):
    """The strip walk's test re-stated (fp32 taps, kp = the flipped kernel, kv = column 0 / kp[0][0], kh = row 0, 1e-7 * max|k|); the products are
    taken exactly, as a fused multiply-add does, and rounded to fp32, as a separate multiply does — both must agree for the answer to count."""
    kp = torch.flip(k, [0, 1])
    if float(kp[0, 0]) == 0.0:
        return False
    kv, kh = kp[:, 0] / kp[0, 0], kp[0, :]
    tol = 1e-7 * float(kp.abs().max())
    fused = bool(((kp.double() - kv.double()[:, None] * kh.double()[None, :]).abs() <= tol).all())
    plain = bool(((kp - kv[:, None] * kh[None, :]).abs() <= tol).all())
    assert fused == plain, 'rank-one test depends on the contraction'
    return fused


def is_rank_one_tile(k):
    """The tile kernel's test re-stated (u = column 0 / k[0][0], v = row 0, 1e-7 * |k[0][0]|)."""
    if float(k[0, 0]) == 0.0:
        return False
    u, v = k[:, 0] / k[0, 0], k[0, :]
    tol = 1e-7 * abs(float(k[0, 0]))
    fused = bool(((k.double() - u.double()[:, None] * v.double()[None, :]).abs() <= tol).all())
    plain = bool(((k - u[:, None] * v[None, :]).abs() <= tol).all())
    assert fused == plain, 'rank-one test depends on the contraction'
    return fused


# ------------------------------------------------------------------------------------------------ the operation
def _blurT(g, kflip):
    """g (B,C,2H,2W) -> g2 (B,C,2H+1,2W+1), g2[Y,X] = sum kflip[a][b] * g[Y+a-2][X+b-2], zero outside, in g's dtype."""
    B, C, Hg, Wg = g.shape
    gp = F.pad(g.reshape(B * C, 1, Hg, Wg), (2, 2, 2, 2))
    return F.conv2d(gp, kflip.to(g.dtype).reshape(1, 1, 4, 4)).reshape(B, C, Hg + 1, Wg + 1)


def chain(o, dt, kflip=None):
    """The operation in dtype dt (float64: the reference; float32: the model, with the fp32 constants) -> dict g_pre, rterm (the per-pixel
    terms of r), r, t_sum (None without ToRGB), m, v (the record value before mul2[1]: g_pre * d or g2 * d), g2 (None on plain layers).
    ``kflip`` overrides the flipped blur kernel (sabotage A)."""
    f = lambda x: None if x is None else x.to(dt)
    pre = o['out'] is None
    g_feat, out, d = f(o['g_feat']), f(o['out']), f(o['d'])
    B, C = d.shape
    if dt == torch.float64:
        c_pos, c_neg, i_pos, i_neg = SQRT2, 0.2 * SQRT2, 1.0 / SQRT2, 1.0 / (0.2 * SQRT2)
    else:
        c_pos, c_neg, i_pos, i_neg = K_SQRT2, K_NEG, K_INVPOS, K_INVNEG
    t = None
    if o['g_rgb'] is not None:
        w = f(o['w_rgb']) * f(o['rgb_scale'])                  # (3,C): the kernels keep w * rgb_scale per channel
        gr = f(o['g_rgb'])
        t = w[0][None, :, None, None] * gr[:, 0:1] + w[1][None, :, None, None] * gr[:, 1:2] + w[2][None, :, None, None] * gr[:, 2:3]
    nb = torch.zeros((), dtype=dt)                                # nw * noise + bias
    if o['noise'] is not None:
        nb = nb + f(o['nw']) * f(o['noise'])
    if o['bias'] is not None:
        nb = nb + f(o['bias'])[None, :, None, None]
    if pre:
        assert t is None
        g_pre = g_feat
        rterm = -(g_pre * nb)
        r = rterm.sum(dim=(2, 3)) + f(o['dot_scale']) * f(o['dot_part']).sum(dim=2)
    else:
        g = f(o['s_rgb'])[:, :, None, None] * t if t is not None else None
        if g_feat is not None:
            g = g_feat if g is None else g_feat + g
        pos = out > 0
        g_pre = g * torch.where(pos, torch.as_tensor(c_pos, dtype=dt), torch.as_tensor(c_neg, dtype=dt))
        ycv = torch.where(pos, out * i_pos, out * i_neg) - nb
        rterm = g_pre * ycv
        r = rterm.sum(dim=(2, 3))
    res = dict(g_pre=g_pre, rterm=rterm, r=r, t_sum=None if t is None else (out * t).sum(dim=(2, 3)),
               m=(g_pre.abs() * d.abs()[:, :, None, None]).max(), g2=None)
    if o['k'] is not None:
        res['g2'] = _blurT(g_pre, torch.flip(o['k'], [0, 1]) if kflip is None else kflip)
        res['v'] = res['g2'] * d[:, :, None, None]
    else:
        res['v'] = g_pre * d[:, :, None, None]
    return res


def record_values(v, scale, hi_only=False):
    """v * scale (a power of two: exact) rounded to fp32 and split as the producers do -> (value, hi) float64: value = hi + lo, or hi alone."""
    hi, lo = split((v.double() * scale).float())
    return (hi if hi_only else hi + lo), hi


def _rel(a, b):
    d = a.double() - b
    return float(d.abs().max() / b.abs().max()), float(d.pow(2).mean().sqrt() / b.pow(2).mean().sqrt())


def errors(got, ref, hi_only=False):
    """got / ref: dicts rec (record values), r, t_sum (None without ToRGB), m -> {(what, metric): error}."""
    out = {}
    if hi_only:
        d = (got['rec'].double() - ref['rec']).abs() - HALF_ULP_F16 * ref['rec'].abs()
        out[('hi', 'excess')] = max(0.0, float(d.max() / ref['rec'].abs().max()))
    else:
        out[('rec', 'max')], out[('rec', 'rms')] = _rel(got['rec'], ref['rec'])
    out[('r', 'max')], out[('r', 'rms')] = _rel(got['r'], ref['r'])
    if ref['t_sum'] is not None:
        out[('t', 'max')], out[('t', 'rms')] = _rel(got['t_sum'], ref['t_sum'])
    out[('m', 'rel')] = abs(float(got['m']) - float(ref['m'])) / float(ref['m'])
    return out


def reference(o, scale):
    """The float64 figures of one call at range scale ``scale`` = mul2[1]: rec, r, t_sum, m (and the chain itself under 'chain')."""
    c = chain(o, torch.float64)
    return dict(rec=c['v'] * scale, r=c['r'], t_sum=c['t_sum'], m=c['m'], chain=c)


def model32(o, scale, hi_only=False):
    c = chain(o, torch.float32)
    return dict(rec=record_values(c['v'], scale, hi_only)[0], r=c['r'], t_sum=c['t_sum'], m=c['m'])


def yardstick(o, scale, ref=None):
    """The float32 model against the reference.  Always on the FULL records (a hi-only call borrows ('rec', 'max') for its excess figure)."""
    ref = ref if ref is not None else reference(o, scale)
    Y = errors(model32(o, scale), ref)
    Y[('m', 'rel')] = max(Y[('m', 'rel')], M_FLOOR)
    return Y


def bar(key, Y):
    return BAR_FACTOR * Y[('rec', 'max') if key == ('hi', 'excess') else key]


TOUCHES = {'A': 'rec', 'B': 'rec', 'C': 'rec', 'D': 'r', 'E': 'rec', 'F': 'm', 'G': 'rec'}


def sabotages(o, scale, ref, fam, hi_only=False, W=None, seg_rows=None, nseg=1):
    """{name: {(what, metric): error}} of the wrong kernels that exist for this call.  fam: 'strip' | 'tile' | 'plain' | 'fform' | 'twopass';
    W: the up-conv input width; seg_rows / nseg: the strip walk's segments (D)."""
    c = ref['chain']
    up = o['k'] is not None
    base = dict(r=c['r'], t_sum=c['t_sum'], m=c['m'])
    good, hi = record_values(c['v'], scale, hi_only)
    out = {}

    def put(name, **kw):
        out[name] = errors({**base, 'rec': good, **kw}, ref, hi_only)

    if up and is_rank_one_strip(o['k']):
        kf = torch.flip(torch.flip(o['k'], [0, 1]), [0])            # vertical taps reversed
        put('A', rec=record_values(chain(o, torch.float64, kflip=kf)['v'], scale, hi_only)[0])
    if fam == 'strip' and 2 * W > 64:
        gz = torch.zeros_like(c['g_pre'])
        gz[..., 64] = c['g_pre'][..., 64]
        g2 = c['g2'].clone()
        g2[..., :64] -= _blurT(gz, torch.flip(o['k'], [0, 1]))[..., :64]
        put('B', rec=record_values(g2 * o['d'].double()[:, :, None, None], scale, hi_only)[0])
    if up and not hi_only:
        v = good.clone()
        v[..., 2 * W] = hi[..., 2 * W]
        put('C', rec=v)
        v = good.clone()
        v[:, :, 1::2, 1::2] = hi[:, :, 1::2, 1::2]
        put('E', rec=v)
    if fam == 'strip' and nseg >= 2:
        put('D', r=c['r'] - c['rterm'][:, :, 2 * seg_rows + 1].sum(dim=2))
    if fam in ('plain', 'fform'):
        v = good.clone()
        for c0 in range(8, v.shape[1], 16):
            v[:, c0:c0 + 8] = hi[:, c0:c0 + 8]
        put('G', rec=v)
    if fam != 'twopass':
        put('F', m=c['g_pre'].abs().max())
    return out


# ------------------------------------------------------------------------------------------------ layouts
def decode_sform_phases_hi(data, B, C, H, W):
    """f16 buffer of 32-byte hi-only phase records: record (i,j) of phase plane p = (b*KC + kc)*4 + py*2+px at 16-byte unit
    p*plane + (i*Wq + j)*2, plane = Hq*Wq*4 units (the FULL-record plane size), slots = hi 0-7, hi 8-15 -> (hi, rest): hi
    (B, 16*KC, 2H+1, 2W+1) float64, rest = every other f16 of the buffer (the second half of every plane included): zero."""
    KC, Hq, Wq = sp_dims(C, H, W)
    v = data.detach().cpu().reshape(B, KC, 2, 2, 2, Hq, Wq, 2, 8)          # [b][kc][py][px][plane half][i][j][slot][8]
    first = v[:, :, :, :, 0]
    # -> [b][kc][slot][j8][i][py][jj][px]: row 2i+py, column 2jj+px
    img = first.permute(0, 1, 6, 7, 4, 2, 5, 3).reshape(B, KC * 16, 2 * Hq, 2 * Wq)
    mask = torch.ones(2 * Hq, 2 * Wq, dtype=torch.bool)
    mask[:2 * H + 1, :2 * W + 1] = False
    rest = torch.cat([img[:, :, mask].reshape(-1), v[:, :, :, :, 1].reshape(-1)])
    return img[:, :, :2 * H + 1, :2 * W + 1].double(), rest


def encode_sform_phases_hi(hi, B, C, H, W):
    """The inverse, from the address rule."""
    KC, Hq, Wq = sp_dims(C, H, W)
    plane = Hq * Wq * 4
    out = torch.zeros(B * KC * 4 * plane * 8, dtype=torch.float16)
    b, c, y, x = torch.meshgrid(torch.arange(B), torch.arange(C), torch.arange(2 * H + 1), torch.arange(2 * W + 1), indexing='ij')
    kc, j = c // 16, c % 16
    unit = ((b * KC + kc) * 4 + (y % 2) * 2 + x % 2) * plane + ((y // 2) * Wq + x // 2) * 2
    out[(unit + j // 8) * 8 + j % 8] = hi
    return out


def encode_fform(x):
    """(B,C,H,W) fp32, C % 16 == 0 -> F-form [B][C/16][H*W][16] in the storage of a (B,C,H,W) tensor, from the address rule: element
    (b, c, p) at ((b*KC + c/16) * HW + p) * 16 + c % 16."""
    B, C, H, W = x.shape
    assert C % 16 == 0
    KC, HW = C // 16, H * W
    out = torch.zeros(B * C * HW, dtype=x.dtype)
    b, c, p = torch.meshgrid(torch.arange(B), torch.arange(C), torch.arange(HW), indexing='ij')
    out[((b * KC + c // 16) * HW + p) * 16 + c % 16] = x.reshape(B, C, HW)
    return out.reshape(B, C, H, W)


def decode_fform(f):
    """The inverse: F-form storage -> (B,C,H,W)."""
    B, C, H, W = f.shape
    return f.reshape(B, C // 16, H * W, 16).permute(0, 1, 3, 2).reshape(B, C, H, W).contiguous()


# ------------------------------------------------------------------------------------------------ the launcher's arithmetic
def strip_geometry(B, C, H, W, seg_tun=0):
    """act_bwd_blurT_impl's strip-walk geometry for an up-conv input of H x W (tunable blurt_seg_rows = seg_tun): nstrips, extra, nseg,
    seg_rows, the segments' position rows, the steps of walk() per segment (two warm-up iterations included) and whether its
    single-step tail runs."""
    KC = (C + 15) // 16
    tiles_x, tiles_y = (W + 1 + 31) // 32, (H + 1 + 3) // 4
    extra = 1 if (W % 32 == 0 and W <= 32) else 0
    nstrips = W // 32 if extra else (W + 1 + 31) // 32
    base = B * KC * nstrips
    nseg = max(1, 4096 // base)
    seg_rows = max(16, (H + 1 + nseg - 1) // nseg)
    if seg_tun > 0:
        seg_rows = min(max(seg_tun, 16), H + 1)
    nseg = (H + 1 + seg_rows - 1) // seg_rows
    segs = [(s * seg_rows, min((s + 1) * seg_rows, H + 1)) for s in range(nseg)]
    return dict(KC=KC, tiles_x=tiles_x, tiles_y=tiles_y, extra=extra, nstrips=nstrips, nseg=nseg, seg_rows=seg_rows,
                rows=[i1 - i0 for i0, i1 in segs], steps=[i1 - i0 + 2 for i0, i1 in segs], tail=[(i1 - i0) % 2 == 1 for i0, i1 in segs],
                strip_ok=H >= 32 and W >= 32 and nseg <= tiles_y and nstrips <= tiles_x,
                last_quads=min(16, (2 * W - 64 * (nstrips - 1)) // 4), last_right_halo=64 * nstrips < 2 * W)


def tile_geometry(C, H, W):
    return dict(KC=(C + 15) // 16, tiles_x=(W + 1 + 31) // 32, tiles_y=(H + 1 + 3) // 4)


def plain_chunks(H, W):
    """(full 512-pixel chunks, pixels of the tail chunk) of oodgan_act_bwd_sform[_f]."""
    return divmod(H * W, 512)


# ------------------------------------------------------------------------------------------------ the cases
# Call: kern 'r1' | 'gen' | None (plain layer); pre: out = None with a hand-made DotActGrad; hi: 32-byte hi-only records; noise 'per' (one map per
# sample) | 'shared' (noise_batch = 1) | None; bias / rgb present; twopass: ops.blurT_to_sform_phases also runs on this call's g_pre (PRE calls).
Call = namedtuple('Call', 'id kern pre hi noise bias rgb twopass', defaults=(False,))
# fam: 'strip' | 'tile' | 'plain' | 'fform'; H, W: the up-conv INPUT size for strip / tile (tensors are 2H x 2W), the tensor size otherwise;
# segs: the blurt_seg_rows settings every call runs with (0 = the launcher's own rule); window: also runs its first call at the window's two ends.
Case = namedtuple('Case', 'id fam B C H W calls segs window', defaults=((0,), False))

CASES = [
    # ---- strip walk.  XTRA instance (W == 32, one strip that also emits j = W); default segments 16,16,1: a one-row last segment
    Case('w32', 'strip', 1, 32, 32, 32, (Call('r1', 'r1', False, False, 'per', True, False),
                                         Call('gen', 'gen', False, False, None, True, False),
                                         Call('pre-r1-hi', 'r1', True, True, 'per', True, False),
                                         Call('pre-gen', 'gen', True, False, 'per', True, False)), (0, 17, 19, 33)),
    # three strips, the third holds only position j = W (X0 = 2W: no own columns, left halo only); default segments 16,16,2
    Case('w64', 'strip', 2, 16, 33, 64, (Call('r1-shared', 'r1', False, False, 'shared', True, False),
                                         Call('pre-gen-nobias', 'gen', True, False, 'per', False, False)), (0, 17, 34)),
    # partial channel block; second strip with one valid quad and no right halo; H + 1 = 48: three full segments, none clipped
    Case('w34', 'strip', 1, 24, 47, 34, (Call('gen-nonoise', 'gen', False, False, None, True, False),
                                         Call('pre-r1', 'r1', True, False, 'per', True, False, True),
                                         Call('pre-gen', 'gen', True, False, 'per', True, False, True)), (0, 17, 48), True),
    # KC = 3; 2W = 132: the last strip has one quad
    Case('w66', 'strip', 1, 48, 40, 66, (Call('r1', 'r1', False, False, 'per', True, False),
                                         Call('pre-r1-hi', 'r1', True, True, None, True, False),
                                         Call('pre-gen', 'gen', True, False, 'per', True, False, True),
                                         Call('pre-r1', 'r1', True, False, 'shared', True, False, True)), (0, 17, 41)),
    # ---- tile kernel (ToRGB present, or H < 32)
    Case('t2', 'tile', 2, 16, 2, 2, (Call('rgb-r1', 'r1', False, False, 'per', True, True),)),                     # smallest
    Case('t18x32', 'tile', 1, 40, 18, 32, (Call('rgb-r1', 'r1', False, False, 'shared', True, True),)),             # j = W alone in tile column 2; KC = 3 partial
    Case('t7x34', 'tile', 1, 24, 7, 34, (Call('gen', 'gen', False, False, None, True, False),)),                   # two tile columns, ragged
    Case('t31x30', 'tile', 2, 32, 31, 30, (Call('r1', 'r1', False, False, 'shared', True, False),)),                # H + 1 = 32: exact tile rows
    Case('t33x36', 'tile', 1, 16, 33, 36, (Call('rgb-r1', 'r1', False, False, 'per', False, True),)),               # ToRGB at a strip-sized shape
    # ---- act_bwd_sform (512 pixels per chunk), each with and without ToRGB
    Case('p4x4', 'plain', 2, 16, 4, 4, (Call('rgb', None, False, False, 'per', True, True), Call('feat', None, False, False, 'shared', True, False))),
    Case('p8x20', 'plain', 1, 48, 8, 20, (Call('rgb', None, False, False, 'per', True, True), Call('feat', None, False, False, None, False, False))),
    Case('p16x32', 'plain', 1, 32, 16, 32, (Call('rgb', None, False, False, 'per', True, True), Call('feat', None, False, False, 'per', True, False))),
    Case('p40x36', 'plain', 1, 24, 40, 36, (Call('feat', None, False, False, 'per', True, False), Call('rgb', None, False, False, 'per', True, True)),
         (0,), True),
    # ---- act_bwd_sform_f (F-form input, ToRGB only)
    Case('f48x64', 'fform', 2, 32, 48, 64, (Call('rgb', None, False, False, 'per', True, True),)),                  # HW a multiple of 512
    Case('f9x20', 'fform', 1, 16, 9, 20, (Call('rgb', None, False, False, 'shared', True, True),)),                 # 180 pixels: clamped tail lanes
    Case('f23x28', 'fform', 1, 32, 23, 28, (Call('rgb', None, False, False, 'per', False, True),)),                 # 644 pixels: a full chunk and a tail
]
CASE_IDS = [c.id for c in CASES]
WINDOWS = {None: None, 'lo': -7, 'hi': 14}      # floor(log2(m * mul2[1])) of a window call

# Figures of a CORRECT kernel measured above 4 x yardstick on the MI355X: (case, call, blurt_seg_rows, win, what, metric) -> measured error; the bar
# is 2 x that value and stays under 1/10 of the call's smallest sabotage on that figure (tests/test_bwd_producer_ref_cpu.py holds the cap).
# The one entry is e_max of r when the strip walk runs the whole height as ONE segment: every thread keeps one fp32 accumulator for its four
# columns over all 2 * 41 g rows, 328 dependent additions, against the blocked sum of the CPU's float32 model (yardstick 0.95e-7, the smallest r
# yardstick of the strip cases: this call's r has no noise term).  The same call measures 1.94 / 2.40 / 5.59 x yardstick at segments of 16 / 17 /
# 41 rows — the error grows with the length of the chain, as it does for the K = 512 convs of splitf16_ref.MEASURED_ABOVE — and its e_rms stays
# inside the bar (3.16).  A row lost from r (sabotage D) costs 0.1.
MEASURED_ABOVE = {
    ('w66', 'pre-r1-hi', 41, None, 'r', 'max'): 5.32e-7,
}


def case(cid):
    return CASES[CASE_IDS.index(cid)]


def call_of(c, call_id):
    return next(k for k in c.calls if k.id == call_id)


def tensor_hw(c):
    return (2 * c.H, 2 * c.W) if c.fam in ('strip', 'tile') else (c.H, c.W)


def inputs(c, k):
    """The seeded fp32 operands of one call (absent ones are None), at the scales tests/test_hip_bwd_producers.py uses; d = |N(1, 0.2)|.
    `out` holds a +0 and a -0 per plane: both take the negative branch."""
    seed = 1000 + 7 * CASE_IDS.index(c.id)
    g = lambda name, shape, std=1.0, mean=0.0: synth.normal(f'bwdprod.{c.id}.{name}', shape, seed, std, mean)
    B, C = c.B, c.C
    Ht, Wt = tensor_hw(c)
    o = dict(out=None, g_feat=None, noise=None, nw=torch.tensor([0.1]), bias=None, d=g('d', (B, C), 0.2, 1.0).abs(), g_rgb=None, w_rgb=None,
             s_rgb=None, rgb_scale=torch.tensor(1.0 / math.sqrt(C), dtype=torch.float32), k=None if k.kern is None else blur_kernel(k.kern),
             dot_part=None, dot_scale=None)
    if c.fam != 'fform':
        o['g_feat'] = g('g', (B, C, Ht, Wt), 3e-4)
    if k.pre:
        o['dot_part'], o['dot_scale'] = g('dotp', (B, C, 3), 1e-3), g('dots', (B, C), 0.3, 1.0)
    else:
        out = g('out', (B, C, Ht, Wt))
        out[:, :, 1, 1] = 0.0
        out[:, :, 1, 2] = -0.0
        o['out'] = out
    if k.noise is not None:
        o['noise'] = g('nz', (B if k.noise == 'per' else 1, 1, Ht, Wt))
    if k.bias:
        o['bias'] = g('bias', (C,), 0.1)
    if k.rgb:
        o.update(g_rgb=g('grgb', (B, 3, Ht, Wt), 1e-3), w_rgb=g('wrgb', (3, C)), s_rgb=g('srgb', (B, C), 0.3, 1.0))
    return o


def range_scale(m, win=None):
    """(unscale, scale) of a call: pow2_scale(m), or for a window call the power of two with floor(log2(m * scale)) = WINDOWS[win]."""
    if win is None:
        return pow2_scale(m)
    e = WINDOWS[win] - (math.frexp(float(m))[1] - 1)
    return 2.0 ** -e, 2.0 ** e


@functools.lru_cache(maxsize=None)
def analysis(cid, call_id, win=None):
    """(operands, mul2 pair, reference, yardstick) of one call of one case, computed once per session and shared by the tests (read only)."""
    c = case(cid)
    o = inputs(c, call_of(c, call_id))
    m = chain(o, torch.float64)['m']
    mul2 = range_scale(m, win)
    ref = reference(o, mul2[1])
    return o, mul2, ref, yardstick(o, mul2[1], ref)


def bar_of(cid, call_id, seg, win, key, Y):
    """The bar of one figure: 4 x yardstick, or 2 x the measured value of a correct kernel recorded above."""
    meas = MEASURED_ABOVE.get((cid, call_id, seg, win) + tuple(key))
    return bar(key, Y) if meas is None else 2.0 * meas
