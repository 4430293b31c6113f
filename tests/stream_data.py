"""Data sets of tests/test_hip_torgb.py, tests/test_hip_act_kernels.py and tests/test_hip_lpips_tail.py (CPU tensors): small integers, powers of two
and dyadic constants, so that every float32 product and sum of the kernels is exact in any order.  tests/test_stream_ref_cpu.py checks that claim
on the terms exact_term_sets() lists."""
import torch

import tail_ref as T

F64 = torch.float64


# ----------------------------------------------------------------------------- FIR kernels of the skip up-sampling
def fir(name):
    if name == 'dyadic':          # make_kernel([1, 3, 3, 1]) * 4: the generator's own, entries {1, 3, 9} / 16
        k = torch.tensor([1.0, 3.0, 3.0, 1.0])
        k = k[None, :] * k[:, None]
        return (k / k.sum() * 4.0).contiguous()
    # integers, no symmetry: k != k^T, != either flip
    return torch.tensor([[1.0, 2.0, 0.0, -1.0], [3.0, -2.0, 1.0, 0.0], [0.0, 1.0, 4.0, -3.0], [2.0, 0.0, -1.0, 1.0]])


# ----------------------------------------------------------------------------- ToRGB
def torgb_data(B, Ci, H, W, seed=0):
    """x, w integers in [-4, 4], s powers of two 2^-2 .. 2^2, integer bias and skip, ys_scale powers of two"""
    k = 100 * seed + Ci + 7 * H + 13 * W
    return dict(x=T.ints((B, Ci, H, W), 9000 + k), w=T.ints((3, Ci), 9100 + k), s=T.pow2((B, Ci), 9200 + k), bias=T.ints((3,), 9300 + k, 1, 4),
                skip=T.ints((B, 3, max(H // 2, 1), max(W // 2, 1)), 9400 + k), ys_scale=T.pow2((B, Ci), 9500 + k))


def torgb_normal(B, Ci, H, W, seed=0):
    k = 100 * seed + Ci + 7 * H + 13 * W
    return dict(x=T.normal((B, Ci, H, W), 9000 + k), w=T.normal((3, Ci), 9100 + k), s=T.normal((B, Ci), 9200 + k), bias=T.normal((3,), 9300 + k),
                skip=T.normal((B, 3, max(H // 2, 1), max(W // 2, 1)), 9400 + k))


def rgb_parts(nparts, B, H, W, seed=0):
    return T.ints((nparts, B, 3, H, W), 9600 + nparts + 7 * H + seed)


def _skip_terms(skip, k4):
    B, C, h, w = skip.shape
    z = torch.zeros(B, C, 2 * h + 3, 2 * w + 3, dtype=F64)
    z[:, :, 2:2 * h + 2:2, 2:2 * w + 2:2] = skip.to(F64)
    return torch.stack([k4[3 - ky, 3 - kx].to(F64) * z[:, :, ky:ky + 2 * h, kx:kx + 2 * w] for ky in range(4) for kx in range(4)], -1)


def torgb_terms(d, k4, scale):
    """(B,3,H,W, Ci + 1 + 16): the products the kernel sums for one output element"""
    ws = scale * d['w'].to(F64)[None] * d['s'].to(F64)[:, None, :]
    conv = (ws[:, :, :, None, None] * d['x'].to(F64)[:, None]).permute(0, 1, 3, 4, 2)
    B, _, H, W, _ = conv.shape
    bias = d['bias'].to(F64).view(1, 3, 1, 1, 1).expand(B, 3, H, W, 1)
    return torch.cat([conv, bias, _skip_terms(d['skip'], k4)], -1)


# ----------------------------------------------------------------------------- activation kernels
def act_data(B, C, H, W, noise_batch=0):
    """integers everywhere; s_rgb powers of two, dscale signed powers of two, nw = 2; `out` has zeros planted at the first and last pixel of every
    plane and wherever the integers fall on 0"""
    k = 31 * B + 7 * C + H + 3 * W
    out = T.ints((B, C, H, W), 9700 + k)
    out.view(B, C, -1)[:, :, 0] = 0.0
    out.view(B, C, -1)[:, :, -1] = 0.0
    sign = T.ints((B, C), 9790 + k, 0, 1) * 2 - 1
    return dict(out=out, g_feat=T.ints((B, C, H, W), 9710 + k), noise=None if not noise_batch else T.ints((noise_batch, 1, H, W), 9720 + k),
                nw=torch.tensor([2.0]), bias=T.ints((C,), 9730 + k), g_rgb=T.ints((B, 3, H, W), 9740 + k), w_rgb=T.ints((3, C), 9750 + k),
                s_rgb=T.pow2((B, C), 9760 + k), dscale=T.pow2((B, C), 9770 + k, -3, 3) * sign, rgb_scale=0.5)


def act_normal(B, C, H, W, noise_batch=0):
    k = 31 * B + 7 * C + H + 3 * W
    out = T.normal((B, C, H, W), 9800 + k)
    out.view(B, C, -1)[:, :, 0] = 0.0
    return dict(out=out, g_feat=T.normal((B, C, H, W), 9810 + k), noise=None if not noise_batch else T.normal((noise_batch, 1, H, W), 9820 + k),
                nw=torch.tensor([0.37]), bias=T.normal((C,), 9830 + k), g_rgb=T.normal((B, 3, H, W), 9840 + k), w_rgb=T.normal((3, C), 9850 + k),
                s_rgb=T.normal((B, C), 9860 + k), dscale=T.pow2((B, C), 9870 + k, -3, 3), rgb_scale=None)


def bias_act_data(shape, noise_batch=0, seed=0):
    k = sum(shape) + seed
    C = shape[1]
    return dict(x=T.ints(shape, 9900 + k), bias=T.ints((C,), 9910 + k), noise=None if not noise_batch else T.ints((noise_batch, 1) + tuple(shape[2:]), 9920 + k),
                nw=torch.tensor([2.0]))


def bias_bwd_data(shape, lo=-4, hi=4):
    """gy integers in [lo, hi]; y integers with zeros planted at the first and the last element"""
    k = sum(shape)
    y = T.ints(shape, 9940 + k)
    y.view(-1)[0] = 0.0
    y.view(-1)[-1] = 0.0
    return dict(gy=T.ints(shape, 9930 + k, lo, hi), y=y)


# ----------------------------------------------------------------------------- LPIPS tail
DYADIC_PREP = dict(a=2.0, b0=-1.0, shift=(0.5, -0.25, 0.125), scale=(0.5, 2.0, 4.0))


def prep_image(B, H, W):
    """multiples of 1/8 in [0, 1]"""
    return T.ints((B, 3, H, W), 10000 + B + H + 3 * W, 0, 8) / 8.0


def head_data(B, C, HW, mode):
    """f0 integers (mode 2: in [-2, 4], zeros and negatives among them; else [0, 4]); one pixel with every f0 channel zero while n1 is not;
    n1 multiples of 1/8 in [-1, 1]; w multiples of 1/4 in [0, 1]"""
    k = 17 * B + C + 3 * HW + mode
    f0 = T.ints((B, C, HW), 10100 + k, -2 if mode == 2 else 0, 4)
    n1 = T.ints((B, C, HW), 10110 + k, -8, 8) / 8.0
    f0[B - 1, :, HW - 1] = 0.0
    n1[B - 1, :, HW - 1] = 0.5
    if HW > 1:          # a pixel with one live channel: s > 0 among zeros
        f0[0, :, 0] = 0.0
        f0[0, C - 1, 0] = 3.0
    return f0, n1, T.ints((C,), 10120 + k, 0, 4) / 4.0


def finish_parts(nparts_list, B=3):
    return [T.ints((B, n), 10200 + 7 * i + n) for i, n in enumerate(nparts_list)]


# ----------------------------------------------------------------------------- the terms of every exact comparison
def exact_term_sets():
    """name -> (..., n) float64 terms that one float32 sum of a kernel adds, for the largest case of every torch.equal comparison of the GPU files"""
    out = {}
    for (B, Ci, H, W), kn in (((1, 1024, 2, 2), 'asym'), ((1, 64, 64, 64), 'dyadic'), ((2, 16, 2, 2), 'asym'), ((1, 16, 66, 64), 'asym'), ((1, 16, 10, 20), 'dyadic')):
        out[f'torgb {B}x{Ci}x{H}x{W} {kn}'] = torgb_terms(torgb_data(B, Ci, H, W), fir(kn), 1.0 / Ci ** 0.5)
    for nparts in (1, 2, 5):
        p = rgb_parts(nparts, 2, 6, 10).to(F64).permute(1, 2, 3, 4, 0)
        d = torgb_data(2, 16, 6, 10)
        out[f'rgb_finish nparts={nparts}'] = torch.cat([p, d['bias'].to(F64).view(1, 3, 1, 1, 1).expand(2, 3, 6, 10, 1), _skip_terms(d['skip'], fir('asym'))], -1)
    d = torgb_data(1, 48, 16, 40)
    out['torgb_sform ys'] = (d['x'].to(F64) * d['ys_scale'].to(F64)[:, :, None, None]).reshape(-1, 1)
    a = act_data(2, 2, 64, 128, 2)
    wk = a['w_rgb'].to(F64) * a['rgb_scale']
    tk = wk.t()[None, :, :, None] * a['g_rgb'].to(F64).reshape(2, 1, 3, -1)          # (B,C,3,HW)
    out['act_bwd g'] = torch.cat([a['g_feat'].to(F64).reshape(2, 2, 1, -1), a['s_rgb'].to(F64)[:, :, None, None] * tk], 2).permute(0, 1, 3, 2)
    out['act_bwd t'] = (a['out'].to(F64).reshape(2, 2, 1, -1) * tk).reshape(2, 2, -1)
    out['act_bwd y_cv tail'] = torch.stack([(a['nw'].to(F64) * a['noise'].to(F64)).expand(2, 2, 64, 128), a['bias'].to(F64).view(1, 2, 1, 1).expand(2, 2, 64, 128)], -1)
    b = bias_act_data((1, 2, 257, 256), 1)
    out['bias_act_fwd'] = torch.stack([b['x'].to(F64), (b['nw'].to(F64) * b['noise'].to(F64)).expand(1, 2, 257, 256),
                                       b['bias'].to(F64).view(1, 2, 1, 1).expand(1, 2, 257, 256)], -1)
    g = bias_bwd_data((1, 2, 1025, 1025), -1, 1)
    out['channel_sum 1025x1025'] = torch.where(g['y'] > 0, g['gy'] * 2.0, g['gy'] * 0.5).to(F64).permute(1, 0, 2, 3).reshape(2, -1)
    g = bias_bwd_data((2, 4, 8, 8))
    out['channel_sum 2x4x8x8'] = torch.where(g['y'] > 0, g['gy'] * 2.0, g['gy'] * 0.5).to(F64).permute(1, 0, 2, 3).reshape(4, -1)
    x, c0, c1 = T.ints((2, 5, 10, 10), 10300).to(F64), T.ints((2, 5, 10, 10), 10301).to(F64), T.ints((2, 5, 10, 10), 10302).to(F64)
    out['feature_modulation SFT'] = torch.stack([x, x * c0, c1], -1)
    img = prep_image(2, 16, 20).to(F64)
    P = DYADIC_PREP
    sh = torch.tensor(P['shift'], dtype=F64).view(1, 3, 1, 1)
    out['lpips_prep sum'] = torch.stack([P['a'] * img, torch.full_like(img, P['b0']), (-sh).expand_as(img)], -1)
    out['lpips_prep product'] = ((P['a'] * img + P['b0'] - sh) / torch.tensor(P['scale'], dtype=F64).view(1, 3, 1, 1)).reshape(-1, 1)
    out['lpips_img_grad'] = torch.stack([T.ints((2, 3, 16, 20), 10400).to(F64), 2.0 * T.ints((2, 3, 16, 20), 10401).to(F64)], -1)
    parts = finish_parts([130, 70, 64, 1, 130])
    out['lpips_finish'] = torch.cat([p.to(F64) / h for p, h in zip(parts, (64, 16, 4, 1024, 256))], 1)
    return out
