"""The float64 yardstick of the SSIM loss term: a torch restatement of ``imgio._ssim`` — F.conv2d with the
``imgio._gauss_window`` taps on the valid region — that autograd can differentiate.  tests/test_ssim_cpu.py chains it to
``imgio.calculate_ssim`` (which tests/test_imgio.py pins to the reference function)."""
import torch
import torch.nn.functional as F

from oodgan import imgio

C1, C2 = (0.01 * 255) ** 2, (0.03 * 255) ** 2


def _filt(x, g):
    """Separable valid correlation of (B,C,H,W) with the 1-D window g, every plane on its own."""
    B, C, H, W = x.shape
    x = x.reshape(B * C, 1, H, W)
    x = F.conv2d(x, g.view(1, 1, -1, 1))
    x = F.conv2d(x, g.view(1, 1, 1, -1))
    return x.reshape(B, C, H - len(g) + 1, W - len(g) + 1)


def ssim(v, y):
    """SSIM per image of (B,C,H,W) images on the [0,255] scale, in the dtype of ``v``: the mean over channels and valid positions."""
    g = torch.from_numpy(imgio._gauss_window()).to(v.dtype)
    mu1, mu2 = _filt(v, g), _filt(y, g)
    s1 = _filt(v * v, g) - mu1 * mu1
    s2 = _filt(y * y, g) - mu2 * mu2
    s12 = _filt(v * y, g) - mu1 * mu2
    m = ((2 * mu1 * mu2 + C1) * (2 * s12 + C2)) / ((mu1 * mu1 + mu2 * mu2 + C1) * (s1 + s2 + C2))
    return m.mean(dim=(1, 2, 3))


def ssim_loss(img, target):
    """(1 - SSIM)[B] for generator-range images: v = 127.5 (img + 1), y = 127.5 (target + 1), unclamped and unrounded."""
    return 1.0 - ssim(127.5 * (img + 1.0), 127.5 * (target + 1.0))


def ssim_loss_and_grad(img, target, dtype=torch.float64):
    """(loss[B], d(sum_b loss_b)/d(img)) on the CPU in ``dtype``."""
    a = img.detach().cpu().to(dtype).requires_grad_(True)
    loss = ssim_loss(a, target.detach().cpu().to(dtype))
    loss.sum().backward()
    return loss.detach(), a.grad
