"""The yardstick of the pixel term on an area-pooled view (``pixel_size``), restated from the definition with
``F.avg_pool2d`` and tests/robust_ref.py's rho — never from the kernel — in the dtype it is asked for: float64 is the reference, float32
(torch on the CPU, the same formula) the measure of what the format itself costs.

    r     = P(img) - P(target)                  P = the mean over every f x f window
    r     = P(beta * (img - target))            with a loss weight beta (B,1,H,W): the pooled composite minus the pooled target
    loss  = mean over C*Hs*Ws of rho(r)         rho = r^2 ('mse') or a robust kind at scale s
    dL/dG = gscale * psi(r_q) on every pixel of window q, gscale = grad_mul/(C*H*W) (twice that for 'mse'), times beta(y,x) for wrt='gen'
"""
import torch
import torch.nn.functional as F

import robust_ref

KINDS = ('mse',) + robust_ref.KINDS


def rho(r, kind, s):
    return r * r if kind == 'mse' else robust_ref.rho(r, kind, s)


def psi(r, kind, s):
    return r if kind == 'mse' else robust_ref.psi(r, kind, s)


def residual(a, t, f, w=None):
    """The pooled residual of tensors already in the working dtype."""
    return F.avg_pool2d(a, f) - F.avg_pool2d(t, f) if w is None else F.avg_pool2d(w * (a - t), f)


def unpool(v, f):
    """Every pooled value on all f x f pixels of its window."""
    return v.repeat_interleave(f, dim=2).repeat_interleave(f, dim=3)


def loss_and_grad(img, target, f, kind='mse', s=1.0, beta=None, grad_mul=1.0, wrt='gen', dtype=torch.float64):
    """(loss[B], gradient (B,C,H,W), composite or None, r (B,C,Hs,Ws)) in ``dtype`` on the CPU, from float32 inputs; s is rounded to float32
    first, as the kernel uses it."""
    s = robust_ref.scale32(s)
    a, t = img.detach().cpu().to(dtype), target.detach().cpu().to(dtype)
    w = None if beta is None else beta.detach().cpu().to(dtype)
    r = residual(a, t, f, w)
    n = a[0].numel()
    gscale = (2.0 if kind == 'mse' else 1.0) * grad_mul / n
    g = unpool(gscale * psi(r, kind, s), f)
    if w is not None and wrt == 'gen':
        g = g * w
    c = None if w is None else t + w * (a - t)
    return rho(r, kind, s).mean(dim=(1, 2, 3)), g, c, r


def window_mean_abs_terms(img, target, f, beta=None):
    """mean over each window of |the terms its sum adds| in float64: |img| and |target| windows summed without beta (two sums, one
    difference), |beta*(img - target)| with it — the scale of the any-order summation bound (f^2 + 2) * 2^-24 * this."""
    a, t = img.detach().cpu().double(), target.detach().cpu().double()
    if beta is None:
        return F.avg_pool2d(a.abs(), f) + F.avg_pool2d(t.abs(), f)
    return F.avg_pool2d((beta.detach().cpu().double() * (a - t)).abs(), f)
