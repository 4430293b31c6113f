"""The similarity alignment of the W+ loop without a GPU: the yardstick of tests/align_ref.py is torch's own
``grid_sample`` / ``affine_grid`` call, in value and in dL/dtheta; ``ops.similarity_inverse`` inverts; the option checks and refusals of
``oodgan.engine``; the C ABI keeps its number and carries the new entries."""
import os
import re

import pytest
import torch

import align_ref as AR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(32, 32), (32, 64), (37, 53)]
THETAS = {'identity': [0.0, 0.0, 0.0, 0.0], 'whole-pixel': None, 'rotation + scale': [0.4, 1.1, 0.2, -0.1], 'general': [0.1, 0.3, 0.2, -0.1],
          'leaves the image': [0.0, 0.0, 3.0, 0.0], 'off-image': [-0.2, -0.5, 3.0, 0.4]}


@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: f'{s[0]}x{s[1]}')
def test_yardstick_is_torchs_grid_sample(shape):
    """Value and dL/dtheta of the float64 yardstick against F.grid_sample(x, F.affine_grid([[a, -s, tx], [s, a, ty]], align_corners=False),
    mode='bicubic', padding_mode='border', align_corners=False) in float64: <= 1e-12 of the largest value / gradient entry."""
    H, W = shape
    gen = torch.Generator().manual_seed(H * 100 + W)
    x = torch.randn(2, 3, H, W, generator=gen, dtype=torch.float64)
    go = torch.randn(2, 3, H, W, generator=gen, dtype=torch.float64)
    for name, row in THETAS.items():
        row = [0.0, 0.0, 2.0 / W, 0.0] if row is None else row
        th = torch.tensor([row, [0.5 * v for v in row]], dtype=torch.float32)
        y = AR.warp(x, th)
        td = th.double().requires_grad_(True)
        yt = AR.torch_warp(x, td)
        gt = torch.autograd.grad((go * yt).sum(), td)[0]
        g = AR.theta_grad(x, th, go)
        e_y = (y - yt).abs().max().item() / x.abs().max().item()
        e_g = (g - gt).abs().max().item() / max(gt.abs().max().item(), 1.0)
        print(f'{H}x{W} {name}: value {e_y:.2e}, dL/dtheta {e_g:.2e} (bar 1e-12)')
        assert e_y <= 1e-12 and e_g <= 1e-12
        if name == 'identity':
            assert torch.equal(AR.warp(x.float(), th, torch.float32), x.float())      # the float32 formula returns the source's bits


def test_non_finite_theta_stays_in_the_image():
    x = torch.randn(1, 1, 8, 8, generator=torch.Generator().manual_seed(0), dtype=torch.float64)
    for row in ([float('nan'), 0, 0, 0], [0, float('inf'), 0, 0], [0, 0, float('inf'), float('-inf')], [float('inf'), 0, 0, 0]):
        y = AR.warp(x, torch.tensor([row], dtype=torch.float32))
        assert y.shape == x.shape       # every gather index was inside the plane


def test_similarity_inverse_round_trips():
    """theta^-1 composed with theta is the identity on the sampling coordinates (<= 1e-12 px), inverts twice to theta, and — through the
    yardstick's warp — returns the interior of a smooth image up to two bicubic resamplings."""
    from oodgan import ops
    th = torch.tensor([[0.1, 0.3, 0.2, -0.1], [-0.1, -0.2, 0.1, 0.15], [0.0, 0.0, 0.06, 0.06]], dtype=torch.float64)
    ti = ops.similarity_inverse(th)
    assert ti.dtype == th.dtype and (ti - AR.inverse(th)).abs().max() <= 1e-15
    assert (ops.similarity_inverse(ti) - th).abs().max() <= 1e-15
    assert ops.similarity_inverse(th.float()).dtype == torch.float32
    for H, W in ((32, 32), (32, 64)):
        # p -> q = T_theta(p) -> T_theta^-1(q): apply the second map at the (non-integer) points of the first, in normalised coordinates
        def mat(t):
            e, c, s = torch.exp(t[:, 0]), torch.cos(t[:, 1]), torch.sin(t[:, 1])
            return torch.stack([torch.stack([e * c, -e * s, t[:, 2]], 1), torch.stack([e * s, e * c, t[:, 3]], 1),
                                torch.tensor([[0.0, 0.0, 1.0]], dtype=torch.float64).expand(t.shape[0], 3)], 1)
        prod = mat(th) @ mat(ti)
        assert (prod - torch.eye(3, dtype=torch.float64)).abs().max() <= 1e-15 * max(H, W)
    s = AR.smooth_image(3, 2, 64, seed=5)
    back = AR.warp(AR.warp(s, th.float()), ti.float())
    e = (back - s)[:, :, 20:-20, 20:-20].abs().max().item()
    print(f'yardstick round trip, interior of a smooth 64² image: {e:.2e} (bar 0.05)')
    assert e <= 0.05
    with pytest.raises(ValueError):
        ops.similarity_inverse(torch.zeros(4))


def test_checks_and_refusals():
    from oodgan import engine as E
    assert E.check_align() == (None, 0.001, 0.0) and E.check_align('similarity') == ('similarity', 0.001, 0.0)
    assert E.check_align('similarity', 0, 0.5) == ('similarity', 0.0, 0.5) and E.check_align(None, -1, 'x') == (None, 0.001, 0.0)
    for bad in (dict(align='affine'), dict(align=True), dict(align='similarity', align_lr=-0.1), dict(align='similarity', align_lr=float('nan')),
                dict(align='similarity', align_lr='0.1'), dict(align='similarity', align_reg=-1.0), dict(align='similarity', align_reg=float('inf')),
                dict(align='similarity', align_lr=True)):
        with pytest.raises(ValueError, match='align'):
            E.check_align(**bad)
    with pytest.raises(ValueError, match='inversion.align_lr'):
        E.check_align('similarity', -1, 0.0, 'inversion.')
    E.refuse_align()
    E.refuse_align(pixel_filter='box')
    for kw, what in ((dict(use_graph=True), 'use_graph'), (dict(lpips=True), 'LPIPS'), (dict(ssim=True), 'SSIM'), (dict(loss_region='blend'), 'loss_region'),
                     (dict(loss_region='fit'), 'loss_region'), (dict(pixel_filter='bicubic'), 'pixel_filter'), (dict(pixel_target=torch.zeros(1)), 'pixel_target'),
                     (dict(latent_space='s'), 'latent_space'), (dict(feature_layer=5), 'feature_layer'), (dict(padded=True), 'zero-padded')):
        with pytest.raises(NotImplementedError, match=what):
            E.refuse_align(**kw)
    assert E.check_align_init(None) is None
    t = torch.zeros(2, 4)
    assert E.check_align_init(t) is t and E.check_align_init(t, 2, 'cpu') is t
    for bad in (torch.zeros(2, 3), torch.zeros(4), torch.zeros(2, 4, dtype=torch.float64), [[0.0] * 4], torch.full((2, 4), float('inf'))):
        with pytest.raises(ValueError, match='align_init'):
            E.check_align_init(bad)
    with pytest.raises(ValueError, match='align_init'):
        E.check_align_init(t, 3, 'cpu')
    # the constructor checks before anything else happens; refuse_mask_fit keeps its signature
    with pytest.raises(ValueError, match='align'):
        E.WPlusInverter(None, align='perspective')
    inv = E.WPlusInverter(None, align='similarity', align_lr=0.002, align_reg=0.1)
    assert (inv.align, inv.align_lr, inv.align_reg, inv.last_alignment, inv.last_aligned_target) == ('similarity', 0.002, 0.1, None, None)
    assert E.WPlusInverter(None).align is None
    import inspect
    assert list(inspect.signature(E.refuse_mask_fit).parameters) == ['use_graph', 'pixel_size', 'pixel_filter', 'pixel_target', 'latent_space',
                                                                     'feature_layer', 'padded']


def test_model_invert_names_the_options():
    """``invert`` has **kwargs: the new names must be real parameters, or an unknown ``align`` would be swallowed in silence."""
    import inspect
    from oodgan.arch import ood_faceGAN_e4e
    p = inspect.signature(ood_faceGAN_e4e.invert).parameters
    assert p['align'].default is None and p['align_lr'].default == 0.001 and p['align_reg'].default == 0.0 and p['align_init'].default is None


def test_abi_keeps_its_number_and_carries_the_entries():
    from ctypes import c_int
    from oodgan import _lib
    assert _lib.ABI_VERSION == 117
    sigs = _lib._SIGS
    assert len(sigs['oodgan_similarity_warp'][1]) == 8 and len(sigs['oodgan_align_grad_step'][1]) == 24
    assert sigs['oodgan_align_grad_nparts'] == (c_int, [c_int, c_int])
    hdr = open(os.path.join(ROOT, 'include', 'oodgan.h')).read()
    for line in ('int oodgan_similarity_warp(const float* src, const float* theta, float* out, int B, int C, int H, int W, void* stream);',
                 'int oodgan_align_grad_nparts(int H, int W);',
                 'int oodgan_align_grad_step(const float* gimg, const float* src, float* theta, float* g, float* m, float* v, int B, int C, int H, int W,'):
        assert line in hdr, line
    assert '"align"' in hdr
    # the number of arguments the header declares is the number the mirror passes
    decl = re.search(r'int oodgan_align_grad_step\((.*?)\);', hdr, re.S).group(1)
    assert len(decl.split(',')) == 24
    h = _lib.lib()          # loads without a GPU; bad arguments come back as a status
    assert h.oodgan_version() == 117
    assert h.oodgan_similarity_warp(None, None, None, 1, 1, 8, 8, None) == -1 and b'similarity_warp' in h.oodgan_last_error()
    assert h.oodgan_align_grad_nparts(64, 64) == 4 and h.oodgan_align_grad_nparts(2, 64) == 0
    assert h.oodgan_dispatch_count(b'align') >= 0
