"""csrc/imgio.hip and the CLI's ``io: device`` chunk post-processing against the host functions of oodgan/imgio.py applied to
the downloaded tensors: the uint8 conversions bit for bit, PSNR exactly, SSIM to 1e-9 (both sides evaluate one float64 formula and differ
by summation order and fma: per map entry the cancellation error is <~ 65025 * 22 * 2^-53 = 1.6e-10 against denominators >= C2 = 58.5)."""
import os

import numpy as np
import pytest
import torch

from oodgan import imgio

pytestmark = pytest.mark.gpu
SHAPES_A = [(1, 1), (5, 7), (37, 53), (64, 64), (256, 256)]
SHAPES_B = [(1, 1), (5, 7), (37, 53), (64, 64), (16, 80)]
RANGES = [(-1, 1), (0, 1), (-0.3, 2.8)]
SSIM_TOL = 1e-9


# ------------------------------------------------------------------------------------------------ kernel a
@pytest.mark.parametrize('B', [1, 3])
@pytest.mark.parametrize('H,W', SHAPES_A)
def test_u8_to_input_is_the_host_expression(B, H, W):
    rng = np.random.default_rng(H * 1000 + W + B)
    bgr = rng.integers(0, 256, (B, H, W, 3), dtype=np.uint8)
    got = imgio.input_from_u8(bgr, size=W, device='cuda')
    want = torch.cat([imgio.image_to_input(bgr[k].astype(np.float64), W) for k in range(B)], 0)
    assert got.shape == (B, 3, H, W) and got.dtype == torch.float32
    assert torch.equal(got.cpu(), want)
    # a device tensor and a single (H,W,3) image are accepted as well
    assert torch.equal(imgio.input_from_u8(torch.from_numpy(bgr[0]).cuda(), size=W).cpu(), want[:1])


def test_input_from_u8_resizes_like_image_to_input():
    bgr = np.random.default_rng(7).integers(0, 256, (40, 56, 3), dtype=np.uint8)
    got = imgio.input_from_u8(bgr, 64, 'cuda')
    want = imgio.image_to_input(bgr.astype(np.float64), 64, device='cuda')
    assert got.shape == (1, 3, 64, 64) and torch.equal(got, want)


# ------------------------------------------------------------------------------------------------ kernel b
def _planted(lo, hi):
    """The float32 nearest each rounding boundary lo + w (k + 0.5) / 255 and its two neighbours; the ends, values beyond them, +-0."""
    w = hi - lo
    mid = (lo + w * (np.arange(255, dtype=np.float64) + 0.5) / 255.0).astype(np.float32)
    vals = [mid, np.nextafter(mid, np.float32(-np.inf)), np.nextafter(mid, np.float32(np.inf)),
            np.array([lo, hi, lo - 0.5, hi + 0.5, lo - 1e-7, hi + 1e-7, lo - 100.0, hi + 100.0, 0.0, -0.0], dtype=np.float32)]
    return np.concatenate(vals).astype(np.float32)


@pytest.mark.parametrize('C', [1, 3])
@pytest.mark.parametrize('B', [1, 3])
@pytest.mark.parametrize('H,W', SHAPES_B)
def test_tensor2img_u8_equals_tensor2img(C, B, H, W):
    for ri, (lo, hi) in enumerate(RANGES):
        rng = np.random.default_rng(((C * 7 + B) * 1000 + H) * 1000 + W + ri)
        t = (1.2 * rng.standard_normal(B * C * H * W)).astype(np.float32)
        planted = rng.permutation(_planted(lo, hi))            # all of them where they fit, else a random subset
        n = min(planted.size, t.size)
        t[rng.permutation(t.size)[:n]] = planted[:n]
        t = torch.from_numpy(t.reshape(B, C, H, W))
        got = imgio.tensor2img_device(t.cuda(), rgb2bgr=True, min_max=(lo, hi))
        assert got.dtype == torch.uint8 and got.shape == ((B, H, W, 3) if C == 3 else (B, H, W))
        got = got.cpu().numpy()
        for k in range(B):
            want = imgio.tensor2img(t[k:k + 1], rgb2bgr=True, min_max=(lo, hi))
            assert np.array_equal(got[k], want), (lo, hi, k, int((got[k] != want).sum()))
        if C == 3:
            rgb = imgio.tensor2img_device(t.cuda(), rgb2bgr=False, min_max=(lo, hi)).cpu().numpy()
            assert np.array_equal(rgb, got[..., ::-1])


def test_tensor2img_u8_sees_every_planted_boundary():
    """The shapes above hold all 775 planted values from 37x53 on; this pins that claim, so that a smaller shape list cannot drop them."""
    assert _planted(-1, 1).size == 775 and 37 * 53 >= 775 and 16 * 80 >= 775 and 64 * 64 >= 775


# ------------------------------------------------------------------------------------------------ kernel c
def _pairs(B, H, W, C, seed):
    rng = np.random.default_rng(seed)
    shape = (B, H, W, C)
    a = rng.integers(0, 256, shape, dtype=np.uint8)
    near = np.clip(a.astype(np.int16) + rng.integers(-9, 10, shape), 0, 255).astype(np.uint8)
    white = np.full(shape, 255, np.uint8)
    stripes = white.copy()
    stripes[:, 1::2] = 254
    return {'random': (a, rng.integers(0, 256, shape, dtype=np.uint8)), 'random+-9': (a, near), 'identical': (a, a.copy()),
            'stripes': (white, stripes), 'black-white': (np.zeros(shape, np.uint8), white)}


@pytest.mark.parametrize('C', [1, 3])
@pytest.mark.parametrize('B', [1, 3])
@pytest.mark.parametrize('H,W,crop', [(11, 11, 0), (15, 15, 2), (12, 40, 0), (45, 70, 2), (45, 70, 5), (64, 64, 0), (256, 256, 2)])
def test_psnr_ssim_u8_vs_host(H, W, crop, B, C):
    for kind, (a, b) in _pairs(B, H, W, C, seed=H * 100 + W + crop + 10 * B + C).items():
        psnr, ssim = imgio.psnr_ssim_device(torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda(), crop)
        assert len(psnr) == B and len(ssim) == B
        for k in range(B):
            hp = imgio.calculate_psnr(a[k], b[k], crop_border=crop)
            hs = imgio.calculate_ssim(a[k], b[k], crop_border=crop)
            print(f'{kind} {H}x{W}x{C} crop {crop} [{k}]: psnr {psnr[k]!r} host {hp!r}; ssim {ssim[k]!r} host {hs!r} diff {abs(ssim[k] - hs):.3e}')
            assert psnr[k] == hp, (kind, k)
            assert abs(ssim[k] - hs) <= SSIM_TOL, (kind, k, ssim[k], hs)
        if kind == 'identical':
            assert all(p == float('inf') for p in psnr)
    if C == 1:          # (B,H,W) images are one channel
        a, b = _pairs(B, H, W, 1, seed=3)['random+-9']
        assert imgio.psnr_ssim_device(torch.from_numpy(a[..., 0]).cuda(), torch.from_numpy(b[..., 0]).cuda(), crop) == \
            imgio.psnr_ssim_device(torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda(), crop)


@pytest.mark.parametrize('H,W,crop', [(10, 10, 0), (14, 14, 2), (10, 64, 0), (64, 14, 2)])
def test_psnr_ssim_u8_refuses_a_cropped_side_under_11(H, W, crop):
    a = torch.zeros(1, H, W, 3, dtype=torch.uint8, device='cuda')
    with pytest.raises(ValueError, match='11x11'):
        imgio.psnr_ssim_device(a, a, crop)


# ------------------------------------------------------------------------------------------------ chunk post-processing
def test_chunk_postprocessing_device_equals_host(tmp_path):
    from oodgan import cli
    size, B = 64, 3
    g = torch.Generator().manual_seed(11)
    out = (0.7 * torch.randn(B, 3, size, size, generator=g)).cuda()
    x = (0.7 * torch.randn(B, 3, size, size, generator=g)).cuda()
    aligns = {i + 1: (1.2 * torch.rand(B, 3, s, s, generator=g) - 0.1).cuda() for i, s in enumerate((8, 16, 32, 64))}
    aligns[size] = (1.2 * torch.rand(B, 3, size, size, generator=g) - 0.1).cuda()
    rng = np.random.default_rng(5)
    bgrs = [rng.integers(0, 256, (64, 64, 3), dtype=np.uint8), rng.integers(0, 256, (40, 40, 3), dtype=np.uint8),
            rng.integers(0, 256, (64, 64, 3), dtype=np.uint8)]
    files = [str(tmp_path / 'data' / n) for n in ('a.png', 'b.png', 'c.png')]
    opts = {'psnr': {'crop_border': 2, 'test_y_channel': False}, 'ssim': {'crop_border': 2, 'test_y_channel': False}}
    hm, hres, hstrips = cli.postprocess_host(out, x, aligns, files, [b.astype(np.float64) for b in bgrs], size, str(tmp_path / 'host'), None, opts)
    with cli.WriterPool(2) as pool:
        dm, dres, dstrips = cli.postprocess_device(out, x, aligns, files, bgrs, size, str(tmp_path / 'dev'), None, opts, pool)
        assert pool.drain() == [None] * (2 * B)
    assert dstrips is not None and dstrips.shape == (B, size, 5 * size) and dres.shape == (B, size, size, 3)
    for k, f in enumerate(files):
        assert np.array_equal(dres[k], hres[k]) and np.array_equal(dstrips[k], hstrips[k])
        name = os.path.basename(f)
        assert np.array_equal(imgio.imread(str(tmp_path / 'dev' / 'inversion' / name)), dres[k])
        from PIL import Image
        with Image.open(tmp_path / 'dev' / 'masks' / name) as im:
            assert np.array_equal(np.asarray(im), dstrips[k])
    print('psnr', dm['psnr'], hm['psnr'], 'ssim diff', [abs(a - b) for a, b in zip(dm['ssim'], hm['ssim'])])
    assert dm['psnr'] == hm['psnr'] and len(dm['psnr']) == B
    assert len(dm['ssim']) == B and all(abs(a - b) <= SSIM_TOL for a, b in zip(dm['ssim'], hm['ssim']))
    # a luma metric runs as the host function on a worker and arrives, in file order, with the drain
    yopts = {'psnr': {'crop_border': 2, 'test_y_channel': True}, 'ssim': {'crop_border': 0, 'test_y_channel': False}}
    hm = cli.postprocess_host(out, x, aligns, files, [b.astype(np.float64) for b in bgrs], size, str(tmp_path / 'host_y'), None, yopts)[0]
    with cli.WriterPool(2) as pool:
        dm = cli.postprocess_device(out, x, aligns, files, [torch.from_numpy(b).cuda() for b in bgrs], size, str(tmp_path / 'dev_y'), None, yopts, pool)[0]
        assert dm['psnr'] == []
        cli.collect_host_metrics(pool.drain(), dm)
    assert dm['psnr'] == hm['psnr'] and all(abs(a - b) <= SSIM_TOL for a, b in zip(dm['ssim'], hm['ssim']))
