"""Image I/O and full-reference metrics — the step AFTER the accelerated path.

Same conventions as the reference harness (run_ood_faceGAN_inversion.py:64-126,159-180) without cv2:
images travel as HxWx3 **BGR** arrays (what ``cv2.imread`` returns), tensors are RGB NCHW in [-1,1].
  img2tensor / tensor2img   BasicSR/basicsr/utils/img_util.py:9-94   (clamp -> [0,1] -> x255 -> round -> uint8)
  calculate_psnr / _ssim    BasicSR/basicsr/metrics/psnr_ssim.py:9-128, metric_util.py:6-45, matlab_functions.py:214-244
  extract_masks             run_ood_faceGAN_inversion.py:74-87       (nearest up-sampling, masks side by side)
PSNR is closed form.  SSIM restates the published algorithm (11x11 Gaussian window sigma 1.5, valid region only);
cv2 is absent from this image, so SSIM is checked against a direct double-loop evaluation, not against cv2 itself.
LPIPS / identity need third-party weights that are not available: the CLI reports them as skipped."""
import math
import os

import numpy as np
import torch


def imread(path):
    """File -> HxWx3 uint8 BGR (cv2.imread convention)."""
    from PIL import Image
    with Image.open(path) as im:
        rgb = np.asarray(im.convert('RGB'))
    return rgb[:, :, ::-1].copy()


def imwrite(path, img):
    """HxWx3 BGR (or HxW gray) uint8 -> file (cv2.imwrite convention)."""
    from PIL import Image
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    arr = np.asarray(img)
    if arr.ndim == 3:
        arr = arr[:, :, ::-1]
    Image.fromarray(np.ascontiguousarray(arr)).save(path)


def img2tensor(imgs, bgr2rgb=True, float32=True):
    """HWC ndarray (or list) -> CHW tensor (or list); BGR->RGB for 3-channel input."""
    def one(img):
        if img.ndim == 3 and img.shape[2] == 3 and bgr2rgb:
            if img.dtype == np.float64:
                img = img.astype(np.float32)
            img = img[:, :, ::-1]
        t = torch.from_numpy(np.ascontiguousarray(img.transpose(2, 0, 1)))
        return t.float() if float32 else t
    return [one(i) for i in imgs] if isinstance(imgs, list) else one(imgs)


def tensor2img(tensor, rgb2bgr=True, out_type=np.uint8, min_max=(0, 1)):
    """(1x)CxHxW / HxW tensor (or list) -> HxWxC BGR / HxW ndarray; uint8 output is ROUNDED (img_util.py:87-90)."""
    if not (torch.is_tensor(tensor) or (isinstance(tensor, list) and all(torch.is_tensor(t) for t in tensor))):
        raise TypeError(f'tensor or list of tensors expected, got {type(tensor)}')
    single = torch.is_tensor(tensor)
    out = []
    for t in ([tensor] if single else tensor):
        t = t.squeeze(0).float().detach().cpu().clamp(*min_max)
        t = (t - min_max[0]) / (min_max[1] - min_max[0])
        if t.dim() == 3:
            a = t.numpy().transpose(1, 2, 0)
            if a.shape[2] == 1:
                a = a[:, :, 0]
            elif rgb2bgr:
                a = a[:, :, ::-1]
        elif t.dim() == 2:
            a = t.numpy()
        else:
            raise TypeError(f'Only 3D or 2D tensors (after squeezing the batch) are supported, got {t.dim()}D')
        if out_type == np.uint8:
            a = (a * 255.0).round()
        out.append(np.ascontiguousarray(a).astype(out_type))
    return out[0] if len(out) == 1 else out


def image_to_input(bgr, size=1024, device=None):
    """What the reference CLI feeds the network (run_ood_faceGAN_inversion.py:159-163): [0,255] BGR -> RGB NCHW in
    [-1,1], bilinearly resized (align_corners=False) to ``size`` if needed.  With a GPU ``device`` the image is uploaded
    at its own size and resized there by ``oodgan_resize_bilinear`` (the harness then runs no torch-ROCm kernel);
    without one the resize is the host-side ATen call the reference makes before its ``.cuda()``."""
    x = (img2tensor(bgr.astype(np.float64) / 255.0, bgr2rgb=True).unsqueeze(0) - 0.5) * 2
    if device is not None:
        x = x.to(device)
    if x.shape[-1] != size:
        if x.is_cuda:
            from . import samm
            x = samm.resize_bilinear(x.contiguous(), size)
        else:
            x = torch.nn.functional.interpolate(x, size=(size, size), mode='bilinear')
    return x


def extract_masks(aligns, size=1024, index=0):
    """aligns: dict level -> (B,3,H,W); channel 2 of every level, nearest-resized to ``size`` and concatenated along
    the width; returns the HxW*n uint8 strip of batch item ``index`` (the reference's CLI feeds one image: item 0; None on any
    failure, like the reference).  Device tensors go through ``oodgan_resize_nearest`` (one strip buffer, written in place); host tensors through ATen."""
    try:
        if all(v.is_cuda for v in aligns.values()):
            from . import samm
            return tensor2img(samm.extract_masks(aligns, size)[index], min_max=(0, 1))
        masks = []
        for k in sorted(aligns.keys()):
            m = aligns[k][:, 2:, ...]
            masks.append(torch.nn.functional.interpolate(m.float(), size=(size, size)))
        return tensor2img(torch.cat(masks, dim=3)[index], min_max=(0, 1))
    except Exception:
        return None


# ----------------------------------------------------------------------------------------------- metrics
def _prepare(img, img2, crop_border, input_order, test_y_channel):
    assert img.shape == img2.shape, f'Image shapes are different: {img.shape}, {img2.shape}.'
    if input_order not in ('HWC', 'CHW'):
        raise ValueError(f'Wrong input_order {input_order}. Supported input_orders are "HWC" and "CHW"')
    out = []
    for a in (img, img2):
        a = np.asarray(a)
        if a.ndim == 2:
            a = a[..., None]
        elif input_order == 'CHW':
            a = a.transpose(1, 2, 0)
        a = a.astype(np.float64)
        if crop_border != 0:
            a = a[crop_border:-crop_border, crop_border:-crop_border, ...]
        if test_y_channel and a.shape[2] == 3:      # ITU-R BT.601 luma of a BGR image, [0,255] in and out
            # metric_util.py:32-46 + matlab_functions.py:236-244,353-359 with their roundings: float32 image / 255, the dot in
            # float64 (the coefficient list is a Python list), / 255 -> float32, x 255 in float32
            y = np.dot(a.astype(np.float32) / 255.0, [24.966, 128.553, 65.481]) + 16.0
            a = ((y / 255.0).astype(np.float32) * 255.0)[..., None]        # stays float32: PSNR's mean / log then run in float32
        out.append(a)
    return out


def calculate_psnr(img, img2, crop_border, input_order='HWC', test_y_channel=False, **kwargs):
    a, b = _prepare(img, img2, crop_border, input_order, test_y_channel)
    mse = np.mean((a - b) ** 2)
    if mse == 0:
        return float('inf')
    return float(20.0 * np.log10(255.0 / np.sqrt(mse)))        # numpy scalar arithmetic in the arrays' dtype, as psnr_ssim.py:43-46


def _gauss_window(n=11, sigma=1.5):
    x = np.arange(n, dtype=np.float64) - (n - 1) / 2.0
    g = np.exp(-(x * x) / (2.0 * sigma * sigma))
    return g / g.sum()


def _filter_valid(a, g):
    """Separable correlation with window g, valid region only (what filter2D(...)[5:-5, 5:-5] keeps)."""
    n = len(g)
    rows = sum(g[i] * a[i:a.shape[0] - n + 1 + i, :] for i in range(n))
    return sum(g[j] * rows[:, j:rows.shape[1] - n + 1 + j] for j in range(n))


def _ssim(a, b):
    a, b = a.astype(np.float64), b.astype(np.float64)
    c1, c2 = (0.01 * 255) ** 2, (0.03 * 255) ** 2
    g = _gauss_window()
    mu1, mu2 = _filter_valid(a, g), _filter_valid(b, g)
    s1 = _filter_valid(a * a, g) - mu1 * mu1
    s2 = _filter_valid(b * b, g) - mu2 * mu2
    s12 = _filter_valid(a * b, g) - mu1 * mu2
    return (((2 * mu1 * mu2 + c1) * (2 * s12 + c2)) / ((mu1 * mu1 + mu2 * mu2 + c1) * (s1 + s2 + c2))).mean()


def calculate_ssim(img, img2, crop_border, input_order='HWC', test_y_channel=False, **kwargs):
    a, b = _prepare(img, img2, crop_border, input_order, test_y_channel)
    return float(np.mean([_ssim(a[..., i], b[..., i]) for i in range(a.shape[2])]))


# ----------------------------------------------------------------------------------------------- device counterparts
# The same conversions and metrics on the GPU (csrc/imgio.hip), for the CLI's `inversion.io: device`: tensors in, tensors
# out, every kernel on the current stream.  The functions above stay the yardstick (tests/test_hip_imgio_device.py).
_U8_TABLES = {}


def u8_input_table():
    """The 256 values ``image_to_input`` / ``img2tensor`` can produce, by their own expression: entry k is the network input of byte k."""
    return ((torch.arange(256, dtype=torch.float64) / 255.0).float() - 0.5) * 2


def _u8_dev(t, name, device=None):
    """A contiguous uint8 device tensor from a uint8 ndarray or tensor (uploaded to ``device`` when it is on the host)."""
    if isinstance(t, np.ndarray):
        if t.dtype != np.uint8:
            raise TypeError(f'{name} must be uint8, got {t.dtype}')
        t = torch.from_numpy(np.ascontiguousarray(t))
    if not torch.is_tensor(t) or t.dtype != torch.uint8:
        raise TypeError(f'{name} must be a uint8 array or tensor, got {type(t).__name__} {getattr(t, "dtype", "")}')
    if not t.is_cuda:
        if device is None:
            raise RuntimeError(f'{name} must be a ROCm (cuda) tensor: the HIP path has no CPU fallback')
        t = t.to(device)
    return t.contiguous()


def input_from_u8(bgr_u8, size=1024, device='cuda'):
    """``image_to_input`` from the file's bytes: (H,W,3) or (B,H,W,3) uint8 BGR (ndarray or tensor; a host array is uploaded as uint8) ->
    (B,3,size,size) float32 RGB in [-1,1] on the device, bit for bit the host's values (a table of its 256 results, ``oodgan_u8_to_input``);
    resized like ``image_to_input`` when the width is not ``size``."""
    from . import _lib, samm
    from .ops import _p, _stream
    u = _u8_dev(bgr_u8, 'bgr_u8', device)
    if u.dim() == 3:
        u = u.unsqueeze(0)
    if u.dim() != 4 or u.shape[3] != 3 or u.numel() == 0:
        raise ValueError(f'bgr_u8 must be (H,W,3) or (B,H,W,3), got {tuple(u.shape)}')
    lut = _U8_TABLES.get(u.device)
    if lut is None:
        lut = _U8_TABLES[u.device] = u8_input_table().to(u.device)
    B, H, W, _ = u.shape
    x = torch.empty(B, 3, H, W, device=u.device, dtype=torch.float32)
    _lib.check(_lib.lib().oodgan_u8_to_input(_p(u), _p(lut), _p(x), B, H, W, _stream()), 'u8_to_input')
    if x.shape[-1] != size:
        x = samm.resize_bilinear(x, size)
    return x


def tensor2img_device(t, rgb2bgr=True, min_max=(0, 1)):
    """``tensor2img`` to uint8 on the device (``oodgan_tensor2img_u8``): (B,C,H,W) float32, C in {1,3} -> uint8 (B,H,W,3), BGR when
    ``rgb2bgr``, or (B,H,W) for C = 1; byte for byte what ``tensor2img`` gives for each batch item."""
    from . import _lib
    from .ops import _dev, _p, _stream
    t = _dev(t, 'tensor')
    if t.dim() != 4 or t.shape[1] not in (1, 3) or t.numel() == 0:
        raise ValueError(f'tensor must be (B,C,H,W) with C in (1, 3), got {tuple(t.shape)}')
    B, C, H, W = t.shape
    out = torch.empty((B, H, W, C) if C == 3 else (B, H, W), device=t.device, dtype=torch.uint8)
    _lib.check(_lib.lib().oodgan_tensor2img_u8(_p(t), _p(out), B, C, H, W, 1 if rgb2bgr else 0, float(min_max[0]), float(min_max[1]),
                                               _stream()), 'tensor2img_u8')
    return out


def extract_masks_device(aligns, size=1024):
    """``extract_masks`` for the whole batch, on the device: the (B, size, size*n) uint8 mask strips (None on any failure, like it)."""
    try:
        from . import samm
        return tensor2img_device(samm.extract_masks(aligns, size), min_max=(0, 1))
    except Exception:
        return None


def psnr_ssim_device(gt_u8, res_u8, crop_border):
    """``calculate_psnr`` / ``calculate_ssim`` (test_y_channel=False) of uint8 device images (B,H,W,C) or (B,H,W): two lists of B float64
    values.  The device returns the exact integer sum of squared differences and the float64 sums of the SSIM maps
    (``oodgan_psnr_ssim_u8``); the closing formulas are the host functions' own.  Synchronises (one small download)."""
    from . import _lib
    from .ops import _p, _stream
    a, b = _u8_dev(gt_u8, 'gt_u8'), _u8_dev(res_u8, 'res_u8')
    if a.shape != b.shape:
        raise ValueError(f'Image shapes are different: {tuple(a.shape)}, {tuple(b.shape)}.')
    if a.dim() == 3:
        a, b = a.unsqueeze(3), b.unsqueeze(3)
    if a.dim() != 4 or a.numel() == 0:
        raise ValueError(f'images must be (B,H,W,C) or (B,H,W), got {tuple(a.shape)}')
    B, H, W, C = a.shape
    crop = int(crop_border)
    hc, wc = H - 2 * crop, W - 2 * crop
    if crop < 0 or hc < 11 or wc < 11:
        raise ValueError(f'SSIM needs a cropped image of at least 11x11, got {H}x{W} with crop_border {crop_border}')
    L = _lib.lib()
    nparts = L.oodgan_psnr_ssim_nparts(C, H, W, crop)
    part_sse = torch.empty(B * nparts, device=a.device, dtype=torch.int64)
    part_ssim = torch.empty(B * nparts, device=a.device, dtype=torch.float64)
    sse = torch.empty(B, device=a.device, dtype=torch.int64)
    ssim_sum = torch.empty(B, C, device=a.device, dtype=torch.float64)
    _lib.check(L.oodgan_psnr_ssim_u8(_p(a), _p(b), _p(part_sse), _p(part_ssim), _p(sse), _p(ssim_sum), B, C, H, W, crop, _stream()),
               'psnr_ssim_u8')
    sse, ssim_sum = sse.cpu().numpy(), ssim_sum.cpu().numpy()
    psnr, ssim = [], []
    for i in range(B):
        mse = np.float64(sse[i]) / (hc * wc * C)
        psnr.append(float('inf') if mse == 0 else float(20.0 * np.log10(255.0 / np.sqrt(mse))))
        ssim.append(float(np.mean(ssim_sum[i] / ((hc - 10) * (wc - 10)))))
    return psnr, ssim
