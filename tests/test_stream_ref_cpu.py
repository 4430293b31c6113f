"""The float64 references of tests/stream_ref.py are not circular: ToRGB equals einsum + the oracle's upfirdn2d, the activation backward and the
LPIPS head equal autograd of their forward formulas, prep and img_grad are adjoint, and the integer / power-of-two / dyadic data sets of the three
GPU files lie in the regime where float32 sums are exact in any order.  No GPU."""
import math
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import lpips_cpu as LO  # noqa: E402
from oracle import ref_cpu as R  # noqa: E402

import stream_ref as S  # noqa: E402
import stream_data as D  # noqa: E402
import tail_ref as T  # noqa: E402

F64 = torch.float64


# ----------------------------------------------------------------------------- ToRGB
@pytest.mark.parametrize('kname', ['dyadic', 'asym'])
def test_torgb_reference_is_einsum_plus_oracle_upfirdn2d(kname):
    k4 = D.fir(kname)
    for B, Ci, H, W in [(2, 5, 6, 10), (1, 16, 2, 2), (1, 3, 4, 8)]:
        x, w, s = T.normal((B, Ci, H, W), 1).to(F64), T.normal((3, Ci), 2).to(F64), T.normal((B, Ci), 3).to(F64)
        bias, skip = T.normal((3,), 4).to(F64), T.normal((B, 3, H // 2, W // 2), 5).to(F64)
        y, mag = S.torgb(x, w, s, bias, skip, k4)
        want = S.torgb_scale(Ci) * torch.einsum('kc,bc,bchw->bkhw', w, s, x) + bias.view(1, 3, 1, 1) + R.upfirdn2d(skip, k4.to(F64), up=2, pad=(2, 1))
        assert torch.allclose(y, want, rtol=1e-13, atol=1e-13)
        assert (mag >= y.abs() - 1e-12).all()
        y2, _ = S.torgb(x, w, s)
        assert torch.allclose(y2, S.torgb_scale(Ci) * torch.einsum('kc,bc,bchw->bkhw', w, s, x), rtol=1e-13, atol=1e-13)
        # rgb_finish: the colour sums split into parts + the same tail
        parts = T.normal((3, B, 3, H, W), 6).to(F64)
        yf, _ = S.rgb_finish(parts, bias, skip, k4)
        assert torch.allclose(yf, parts.sum(0) + bias.view(1, 3, 1, 1) + R.upfirdn2d(skip, k4.to(F64), up=2, pad=(2, 1)), rtol=1e-13, atol=1e-13)


def test_asymmetric_kernel_tells_a_transpose_and_a_missing_flip_apart():
    k4 = D.fir('asym')
    skip = T.normal((1, 3, 3, 4), 7).to(F64)
    u, _ = S.upsample_skip(skip, k4)
    for wrong in (k4.t(), torch.flip(k4, [0, 1]), torch.flip(k4, [0]), torch.flip(k4, [1])):
        uw, _ = S.upsample_skip(skip, wrong.contiguous())
        assert (u - uw).abs().max() > 1.0
    sym = D.fir('dyadic')
    us, _ = S.upsample_skip(skip, sym)
    assert torch.equal(us, S.upsample_skip(skip, torch.flip(sym.t(), [0, 1]).contiguous())[0])          # the symmetric kernel cannot


def test_torgb_scale_is_a_power_of_two_for_the_exact_channel_counts():
    for Ci in (16, 64, 256, 1024):
        assert S.torgb_scale(Ci) == 1.0 / math.sqrt(Ci) and math.frexp(S.torgb_scale(Ci))[0] == 0.5
    for Ci in (3, 5, 24, 48, 80, 320):
        assert math.frexp(S.torgb_scale(Ci))[0] != 0.5


# ----------------------------------------------------------------------------- activation
def test_act_constants():
    k, i = S.ActConsts.kernel(), S.ActConsts.ideal(0.2, math.sqrt(2.0))
    for a, b in ((k.pos, i.pos), (k.neg, i.neg), (k.inv_pos, i.inv_pos), (k.inv_neg, i.inv_neg)):
        assert a == S.f32(a) and abs(a - b) <= 2.0 * S.U * abs(b)          # float32 numbers, within two roundings of the exact factor


@pytest.mark.parametrize('noise_kind', ['none', 'shared', 'per_sample'])
@pytest.mark.parametrize('rgb', [False, True])
def test_act_bwd_reference_is_autograd(noise_kind, rgb):
    """out = lrelu(conv + nw noise + bias, 0.2) sqrt2; rgb = scale sum_c w[k,c] s[b,c] out[b,c]; L = <g_feat, out> + <g_rgb, rgb>"""
    B, C, H, W = 2, 3, 4, 5
    slope, scale = 0.2, math.sqrt(2.0)
    conv = T.normal((B, C, H, W), 11).to(F64).requires_grad_(True)
    noise = None if noise_kind == 'none' else T.normal((1 if noise_kind == 'shared' else B, 1, H, W), 12).to(F64)
    nw, bias = torch.tensor([0.7], dtype=F64), T.normal((C,), 13).to(F64)
    g_feat, g_rgb = T.normal((B, C, H, W), 14).to(F64), T.normal((B, 3, H, W), 15).to(F64)
    w_rgb, s_rgb = T.normal((3, C), 16).to(F64), T.normal((B, C), 17).to(F64).requires_grad_(True)
    pre = conv + bias.view(1, C, 1, 1) + (0 if noise is None else nw * noise)
    pre.retain_grad()
    out = F.leaky_relu(pre, slope) * scale
    L = (g_feat * out).sum()
    rs = 1.0 / math.sqrt(C)
    if rgb:
        L = L + (g_rgb * (rs * torch.einsum('kc,bc,bchw->bkhw', w_rgb, s_rgb, out))).sum()
    L.backward()
    ref = S.act_bwd_fused(out.detach(), g_feat, noise, nw, bias, g_rgb if rgb else None, w_rgb, s_rgb.detach(), rs, consts=S.ActConsts.ideal(slope, scale))
    assert torch.allclose(ref['g_pre'], pre.grad, rtol=1e-12, atol=1e-13)
    assert torch.allclose(ref['y_cv'], conv.detach(), rtol=1e-12, atol=1e-12)          # the conv output recovered from the activation
    assert torch.allclose(ref['r'], (pre.grad * conv.detach()).sum((2, 3)), rtol=1e-11, atol=1e-12)
    if rgb:
        assert torch.allclose(ref['t'], s_rgb.grad, rtol=1e-12, atol=1e-12)
    else:
        assert ref['t'] is None
    # g_feat = None with the RGB branch: the same with a zero g_feat
    if rgb:
        a = S.act_bwd_fused(out.detach(), None, noise, nw, bias, g_rgb, w_rgb, s_rgb.detach(), rs)
        b = S.act_bwd_fused(out.detach(), torch.zeros_like(g_feat), noise, nw, bias, g_rgb, w_rgb, s_rgb.detach(), rs)
        assert torch.equal(a['g_pre'], b['g_pre']) and torch.equal(a['r'], b['r'])
    # part_max: per chunk of 4096
    assert ref['part_max'].shape == (B, C, 1) and torch.equal(ref['part_max'][:, :, 0], ref['g_pre'].abs().amax((2, 3)))


def test_act_bwd_reference_at_zero_and_chunks():
    """out == 0 takes the negative branch (as autograd of leaky_relu at 0); part_max splits at 4096"""
    out = torch.tensor([[[0.0, 2.0, -1.0]]], dtype=F64)
    g = torch.tensor([[[1.0, 1.0, 1.0]]], dtype=F64)
    k = S.ActConsts.kernel()
    ref = S.act_bwd_fused(out, g)
    assert ref['g_pre'].flatten().tolist() == [k.neg, k.pos, k.neg]
    x = torch.zeros(1, 1, 2, requires_grad=True, dtype=F64)
    F.leaky_relu(x, 0.2).sum().backward()
    assert x.grad.flatten().tolist() == [0.2, 0.2]
    big = torch.ones(1, 1, 4097, dtype=F64)
    gg = torch.ones(1, 1, 4097, dtype=F64)
    gg[0, 0, 4096] = 5.0
    pm = S.act_bwd_fused(big, gg, dscale=torch.tensor([[-2.0]]))['part_max']
    assert pm.shape == (1, 1, 2) and torch.allclose(pm.flatten(), torch.tensor([2.0 * k.pos, 10.0 * k.pos], dtype=F64))
    assert torch.equal(S.part_max_of(torch.tensor([[[1.0, -3.0]]]), torch.tensor([[-0.5]])), torch.tensor([[[1.5]]]))


def test_bias_noise_act_and_backward_reference():
    B, C, H, W = 2, 3, 3, 5
    x = T.normal((B, C, H, W), 21).to(F64).requires_grad_(True)
    noise, nw, bias = T.normal((B, 1, H, W), 22).to(F64), torch.tensor([0.3], dtype=F64), T.normal((C,), 23).to(F64)
    y = S.bias_noise_act(x, bias, noise, nw, 0.25, 2.0)
    want = R.fused_leaky_relu(x + nw * noise, bias, 0.25, 2.0)
    assert torch.allclose(y, want, rtol=1e-14, atol=1e-14)
    gy = T.normal((B, C, H, W), 24).to(F64)
    (gx,) = torch.autograd.grad(want, x, gy)
    ref = S.bias_act_bwd(gy, y.detach(), 0.25, 2.0)
    assert torch.allclose(ref, gx, rtol=1e-14, atol=1e-14)
    assert torch.allclose(S.channel_sum(ref)[0], gx.sum((0, 2, 3)), rtol=1e-13, atol=1e-13)
    # no noise weight: 1; 2-D input: bias over dim 1
    assert torch.equal(S.bias_noise_act(x.detach(), None, noise, None, 0.25, 2.0), R.fused_leaky_relu(x.detach() + noise, None, 0.25, 2.0))
    x2, b2 = T.normal((5, 24), 25).to(F64), T.normal((24,), 26).to(F64)
    assert torch.allclose(S.bias_noise_act(x2, b2, slope=0.25, scale=2.0), R.fused_leaky_relu(x2, b2, 0.25, 2.0), rtol=1e-14, atol=1e-14)


def test_feature_modulation_reference():
    x, c0, c1 = T.normal((2, 3, 4, 5), 31).to(F64), T.normal((2, 3, 1, 1), 32).to(F64), T.normal((2, 3, 1, 1), 33).to(F64)
    assert torch.allclose(S.feature_modulation(x, c0, c1, 'SFT')[0], x * (1 + c0) + c1)
    assert torch.allclose(S.feature_modulation(x, None, c1, 'ADD')[0], x + c1)
    assert torch.allclose(S.feature_modulation(x, c0, c1, 'FUSE')[0], x + c1 * torch.sigmoid(c0), rtol=1e-14, atol=1e-14)


# ----------------------------------------------------------------------------- LPIPS tail
def test_prep_and_img_grad_are_adjoint():
    """<prep(x), g> == <x, img_grad(g)> once b0 and the shift are removed (prep is then linear: a x / scale_c, padded and rearranged)"""
    for B, H, W in [(1, 16, 16), (2, 16, 20), (1, 20, 16)]:
        x = T.normal((B, 3, H, W), 41)
        g = T.normal((B, 48, H // 4 + 1, W // 4 + 1), 42)
        a, scale3 = 2.0, (0.5, 0.25, 4.0)
        p, _, inside = S.lpips_prep(x, a, 0.0, (0.0, 0.0, 0.0), scale3)
        gi = S.lpips_img_grad(g, torch.zeros(B, 3, H, W), a, 1.0, scale3)
        lhs, rhs = (p * g.to(F64)).sum(), (x.to(F64) * gi).sum()
        assert abs(lhs - rhs) <= 1e-12 * (p * g.to(F64)).abs().sum()
        assert inside.sum() == B * 3 * H * W and (p[~inside] == 0).all()
        # against the oracle's own ScalingLayer + pad + unfold, with the real constants
        pr, _, _ = S.lpips_prep(x, 2.0, -1.0, LO.SHIFT, LO.SCALE)
        v = ((2 * x.to(F64) - 1) - torch.tensor([S.f32(s) for s in LO.SHIFT], dtype=F64).view(1, 3, 1, 1)) * \
            torch.tensor([S.f32_div(1.0, S.f32(s)) for s in LO.SCALE], dtype=F64).view(1, 3, 1, 1)
        vp = F.pad(v, (2, 2, 2, 2))
        for ch in (0, 5, 22, 47):
            c, dy, dx = ch // 16, (ch // 4) % 4, ch % 4
            assert torch.equal(pr[:, ch], vp[:, c, dy::4, dx::4][:, :H // 4 + 1, :W // 4 + 1])
        # += : what gimg held stays
        g0 = T.normal((B, 3, H, W), 43)
        assert torch.allclose(S.lpips_img_grad(g, g0, a, 1.0, scale3), g0.to(F64) + gi)


@pytest.mark.parametrize('mode', [1, 2])
def test_head_reference_is_autograd_of_the_oracle(mode):
    B, C, HW = 2, 13, 33
    f = T.normal((B, C, HW), 51).to(F64)
    if mode == 2:
        f = f.clamp_min(0.0) + 0.0
        f[0, :, 4] = 0.0
        f[0, 3, 4] = 1.5          # s > 0 with zero channels beside it
    f = f.requires_grad_(True)
    n1 = LO.normalize_tensor(T.normal((B, C, HW), 52).to(F64))
    w = T.normal((C,), 53).to(F64).abs()
    coef = 0.125
    d = (w.view(1, C, 1) * (LO.normalize_tensor(f) - n1) ** 2).sum(1)          # (B, HW): lin layer of the squared difference
    (g,) = torch.autograd.grad(d.sum() * coef, f)
    ref = S.lpips_head(f.detach(), n1, w, coef, mode)
    want = g if mode == 1 else g * (f.detach() > 0)
    assert torch.allclose(ref['out'], want, rtol=1e-10, atol=1e-12)
    assert torch.allclose(ref['d'], d.detach(), rtol=1e-12, atol=1e-14)
    assert ref['part'].shape == (B, 2) and torch.allclose(ref['part'][:, 0], d.detach()[:, :32].sum(1)) and torch.allclose(ref['part'][:, 1], d.detach()[:, 32])
    assert (ref['out_mag'] >= ref['out'].abs() * (1 - 1e-12)).all()
    assert torch.allclose(S.lpips_head(f.detach())['out'], LO.normalize_tensor(f.detach()), rtol=1e-12, atol=1e-14)


def test_head_reference_convention_at_zero_norm():
    """a pixel whose f0 channels are all zero: n0 = 0, e_c = -2 w n1, out = coef * r * e_c with r = 1 / 1e-10f, the second term dropped; autograd
    gives NaN there (sqrt backward at 0)"""
    C = 3
    f = torch.zeros(1, C, 2, dtype=F64)
    f[0, :, 1] = torch.tensor([1.0, 2.0, 2.0], dtype=F64)
    n1 = torch.tensor([[[0.5, 0.1], [-0.25, 0.2], [0.0, 0.3]]], dtype=F64)
    w = torch.tensor([1.0, 2.0, 0.5], dtype=F64)
    ref = S.lpips_head(f, n1, w, 0.5, 1)
    r = 1.0 / S.f32(1e-10)
    assert torch.allclose(ref['out'][0, :, 0], 0.5 * r * (-2.0 * w * n1[0, :, 0]), rtol=1e-14)
    assert torch.isfinite(ref['out']).all()
    assert torch.allclose(ref['d'][0, 0], (w * n1[0, :, 0] ** 2).sum())
    assert (S.lpips_head(f, n1, w, 0.5, 2)['out'][0, :, 0] == 0).all()          # mode 2: !(f > 0)
    fz = f.clone().requires_grad_(True)
    (g,) = torch.autograd.grad((w.view(1, C, 1) * (LO.normalize_tensor(fz) - n1) ** 2).sum(), fz)
    assert torch.isnan(g[0, :, 0]).all() and torch.isfinite(g[0, :, 1]).all()


def test_add_mask_and_finish_reference():
    y, a = torch.tensor([1.0, 2.0, 3.0, 4.0]), torch.tensor([10.0, 10.0, 10.0, 10.0])
    m = torch.tensor([0.0, -0.0, -1.0, 0.5])
    assert S.add_mask(y, a, m).tolist() == [0.0, 0.0, 0.0, 14.0]
    parts = [T.ints((3, 70), 61), T.ints((3, 1), 62)]
    v, mag = S.lpips_finish(parts, [64, 3])
    assert torch.allclose(v, parts[0].to(F64).sum(1) / 64 + parts[1].to(F64).sum(1) * S.f32_div(1.0, 3.0))
    assert (mag >= v.abs()).all()


# ----------------------------------------------------------------------------- the data sets of the GPU files
def test_exact_any_order_helper():
    assert S.exact_any_order(torch.tensor([[1.0, -2.5, 0.25]], dtype=F64))
    assert not S.exact_any_order(torch.tensor([[2.0 ** 24, 0.5]], dtype=F64))
    assert not S.exact_any_order(torch.tensor([[1.0, 1.0 / 3.0]], dtype=F64))


def test_data_sets_are_in_the_exact_regime():
    sets = D.exact_term_sets()
    assert len(sets) >= 10
    for name, t64 in sets.items():
        assert S.fits_float32(t64), name
        assert S.exact_any_order(t64), name
        rows = t64.reshape(-1, t64.shape[-1])
        assert T.exact_regime(rows[:256].to(torch.float32)), name
