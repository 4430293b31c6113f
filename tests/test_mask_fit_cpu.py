"""The fitted out-of-domain mask of the W+ loop (loss_region='fit') without a GPU: the float64 yardstick the GPU tests compare
with (tests/mask_fit_ref.py) against autograd and against the reference's MaskLoss as recorded in tests/golden/wplus_maskfit_64.npz, the two
tie rules, the argument checks (which raise before any device work) and the host mirror of the C ABI."""
import math

import pytest
import torch

import mask_fit_ref as MR


@pytest.mark.parametrize('m', [4, 16])
@pytest.mark.parametrize('f', [2, 4, 16])
def test_ut_gather_is_the_adjoint_of_interpolate(f, m):
    """The hand-written gather — each cell over its own tent support of at most 2F x 2F pixels, the clamped edge rows and columns on the edge
    cells — equals autograd through F.interpolate, and W a W^T with the tent matrix is the interpolation itself.  Float64: bars 1e-13."""
    S = f * m
    gen = torch.Generator().manual_seed(100 * f + m)
    a = torch.rand(2, 1, m, m, dtype=torch.float64, generator=gen, requires_grad=True)
    e = torch.randn(2, 1, S, S, dtype=torch.float64, generator=gen)
    beta = MR.upsample(a, S)
    (beta * e).sum().backward()
    W = MR.tent_matrix(S, m)
    assert (W.sum(1) - 1).abs().max() <= 1e-15                      # every pixel's weights sum to one
    assert (W @ a.detach()[:, 0] @ W.t() - beta.detach()[:, 0]).abs().max() <= 1e-13
    got = MR.ut_gather(e, m)
    err = (got - a.grad).abs().max().item() / a.grad.abs().max().item()
    print(f'F {f} m {m}: gather vs autograd {err:.2e} of max')
    assert err <= 1e-13


def test_regulariser_is_the_references_mask_loss(golden):
    """On the masks the reference run passed through (a before steps 1, 10, 20, 30, both images, float64), the yardstick's two terms times
    their weights equal what MaskLoss returned there.  MaskLoss accumulates into float32 tensors whatever it is fed: bar 1e-6 relative
    (+ 1e-9), fp32's rounding of values the yardstick holds in float64."""
    g = golden('wplus_maskfit_64.npz')
    area, wa, wb = (float(v) for v in g['settings'][:3])
    keep = [int(t) for t in g['keep']]
    seen_open = False
    for tag in ('f64', 'f32'):
        for k, t in enumerate(keep):
            a = g[f'a_kept_{tag}'][k]                               # (B,1,m,m)
            hinge, binary = MR.regulariser(a, area)
            for b in range(a.shape[0]):
                want_a, want_b = g[f'ml_area_{tag}'][t - 1, b].item(), g[f'ml_binary_{tag}'][t - 1, b].item()
                assert abs(wa * hinge[b].item() - want_a) <= 1e-6 * abs(want_a) + 1e-9, (tag, t, b)
                assert abs(wb * binary[b].item() - want_b) <= 1e-6 * abs(want_b) + 1e-9, (tag, t, b)
                assert abs((1 - a[b]).mean().item() - g[f'mean_1ma_{tag}'][t - 1, b].item()) <= 1e-6
                seen_open = seen_open or want_a > 0
    # the recorded run stays under its budget; the hinge's open side on a mask of the run against MaskLoss' formula, A below its area
    a = g['a_kept_f64'][-1]
    low = float((1 - a).mean(dim=(1, 2, 3)).min()) - 0.05
    hinge, _ = MR.regulariser(a, low)
    assert torch.allclose(hinge, (1 - a).mean(dim=(1, 2, 3)) - low, rtol=0, atol=1e-15) and (hinge > 0).all()


def test_tie_rules():
    """torch's subgradients: at mean(1 - a) == A the hinge is Python's max(0-tensor, x) = the zero tensor, gradient 0; at a == 1/2
    min(a, 1 - a) has gradient 0.  The written-out gradient agrees with autograd on both sides of both ties and at them."""
    m = 4
    for name, a0, area in (('hinge tie', torch.full((1, 1, m, m), 0.75, dtype=torch.float64), 0.25),
                           ('hinge open', torch.full((1, 1, m, m), 0.75, dtype=torch.float64), 0.20),
                           ('hinge shut', torch.full((1, 1, m, m), 0.75, dtype=torch.float64), 0.30),
                           ('min tie', torch.tensor([0.5, 0.25, 0.75, 0.5], dtype=torch.float64).repeat(4).reshape(1, 1, m, m), 0.9)):
        a = a0.clone().requires_grad_(True)
        over = (1 - a).mean() - area
        hinge = max(torch.tensor(0., dtype=torch.float64), over)           # MaskLoss' own expression
        binary = torch.mean(torch.min(a, 1 - a))
        tot = 5.0 * hinge + 0.2 * binary
        if tot.requires_grad:
            tot.backward()
        auto = a.grad if a.grad is not None else torch.zeros_like(a0)
        mine = MR.regulariser_grad(a0, area, 5.0, 0.2)
        assert (auto - mine).abs().max() <= 1e-15, name
        h2, b2 = MR.regulariser(a0, area)
        assert abs(h2.item() - float(hinge.detach())) <= 1e-15 and abs(b2.item() - float(binary.detach())) <= 1e-15, name
    assert MR.regulariser_grad(torch.full((1, 1, m, m), 0.75, dtype=torch.float64), 0.25, 5.0, 0.0).abs().max() == 0          # the hinge tie
    assert MR.regulariser_grad(torch.full((1, 1, m, m), 0.5, dtype=torch.float64), 0.9, 0.0, 0.2).abs().max() == 0            # the min tie


def test_option_checks_raise_before_any_device_work():
    from oodgan import engine as E
    assert E.check_mask_fit() == (64, 0.1, 0.30, 5.0, 0.2)
    assert E.check_mask_fit(16, image_size=64)[0] == 16
    for bad in (8, 48, 512, 64.0, True, None, '64'):
        with pytest.raises(ValueError, match='mask_size'):
            E.check_mask_fit(bad)
    for size, img in ((64, 64), (128, 64), (256, 256), (64, 96)):
        with pytest.raises(ValueError, match='mask_size'):
            E.check_mask_fit(size, image_size=img)
    for key in ('mask_area_weight', 'mask_binary_weight'):
        for bad in (-1.0, math.nan, math.inf, 'x', True):
            with pytest.raises(ValueError, match=key):
                E.check_mask_fit(**{key: bad})
        assert E.check_mask_fit(**{key: 0})
    for bad in (0.0, -0.1, math.nan, math.inf, None, True):
        with pytest.raises(ValueError, match='mask_lr'):
            E.check_mask_fit(mask_lr=bad)
    for bad in (-0.01, 1.01, math.nan, 'a'):
        with pytest.raises(ValueError, match='mask_area'):
            E.check_mask_fit(mask_area=bad)
    assert E.check_mask_fit(mask_area=0)[2] == 0.0 and E.check_mask_fit(mask_area=1)[2] == 1.0
    with pytest.raises(ValueError, match='inversion.mask_lr'):
        E.check_mask_fit(mask_lr=0, prefix='inversion.')
    # the start of the mask
    assert E.check_mask_init(0.88) == 0.88 and E.check_mask_init('blend') == 'blend'
    for bad in (0.0, 1.0, -0.5, 1.5, math.nan, True, 'full', None):
        with pytest.raises(ValueError, match='mask_init'):
            E.check_mask_init(bad)
    t = torch.full((2, 1, 16, 16), 0.5)
    assert E.check_mask_init(t, 2, 16, 'cpu') is t
    for bad in (t.double(), t[0], t[:, :, :8], torch.zeros(2, 3, 16, 16)):
        with pytest.raises(ValueError, match='mask_init'):
            E.check_mask_init(bad, 2, 16, 'cpu')
    with pytest.raises(ValueError, match='mask_init'):
        E.check_mask_init(t, 2, 16, 'cuda:0')
    # the logits: clipped to [1e-3, 1 - 1e-3] first; values outside [0, 1] (NaN included) refused
    l = E.mask_logits(torch.tensor([0.0, 1.0, 0.88, 0.5]).reshape(1, 1, 2, 2))
    want = torch.tensor([math.log(1e-3 / (1 - 1e-3)), math.log((1 - 1e-3) / 1e-3), math.log(0.88 / 0.12), 0.0]).reshape(1, 1, 2, 2)
    assert (l - want).abs().max() <= 1e-4
    for bad in (torch.tensor([[[[1.5]]]]), torch.tensor([[[[-0.1]]]]), torch.tensor([[[[math.nan]]]])):
        with pytest.raises(ValueError, match='mask_init'):
            E.mask_logits(bad)
    # what the fitted mask does not go with: one place
    E.refuse_mask_fit()
    for kw in (dict(use_graph=True), dict(pixel_size=32), dict(pixel_filter='bicubic'), dict(pixel_target=torch.zeros(1)), dict(latent_space='s'),
               dict(feature_layer=5), dict(padded=True)):
        with pytest.raises(NotImplementedError, match="loss_region='fit'"):
            E.refuse_mask_fit(**kw)
    # the inverter checks its own options in the constructor: no engine is touched
    with pytest.raises(ValueError, match='mask_size'):
        E.WPlusInverter(None, mask_size=20)
    with pytest.raises(ValueError, match='mask_lr'):
        E.WPlusInverter(None, mask_size=16, mask_lr=-1)
    inv = E.WPlusInverter(None, mask_size=16)
    assert (inv.mask_size, inv.mask_lr, inv.mask_area, inv.mask_area_weight, inv.mask_binary_weight) == (16, 0.1, 0.30, 5.0, 0.2)
    assert E.WPlusInverter(None).mask_size is None


def test_lib_mirror_lists_the_entries_and_the_abi():
    from oodgan import _lib
    assert _lib.ABI_VERSION == 117
    names = _lib.exported_symbols()
    for entry, nargs in (('oodgan_maskfit_expand', 7), ('oodgan_maskfit_chain', 9), ('oodgan_maskfit_step', 26)):
        assert entry in names and len(_lib._SIGS[entry][1]) == nargs, entry
    import os
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'oodgan.h')).read()
    for entry in ('oodgan_maskfit_expand', 'oodgan_maskfit_chain', 'oodgan_maskfit_step'):
        assert f'int {entry}(' in header
    assert 'mask_loss.py' in header        # the reference's MaskLoss is named as the anchor
