"""The yardstick of the pixel term on an antialiased resampled view (``pixel_filter``), restated from the definition with
dense matrices — never from the kernel — in the dtype it is asked for: float64 is the reference, float32 (torch on the CPU, the same
formula) the measure of what the format itself costs.

    T     = s*F taps per output, k[j] = phi((j + 1/2 - T/2) / F); output q reads inputs F*q - (T-F)/2 + j
    D     = the dense (n, H) matrix of one axis: taps outside [0, H) dropped, each row renormalised to sum 1
    view  = Dy · G · Dx^T per plane
    r     = view - y;  loss = mean over C*Hs*Ws of rho(r)
    dL/dG = gs * Dy^T psi(r) Dx, gs = grad_mul/(C*Hs*Ws) (twice that for 'mse')
"""
import math

import torch

import robust_ref

KINDS = ('mse',) + robust_ref.KINDS
SUPPORT = {'bilinear': 2, 'bicubic': 4, 'lanczos3': 6}
FACTORS = (2, 4, 8, 16)


def phi(name, t):
    """The filter at the float64 points t."""
    t = t.abs()
    if name == 'bilinear':
        return torch.where(t < 1, 1 - t, torch.zeros_like(t))
    if name == 'bicubic':
        a = -0.5
        return torch.where(t <= 1, (a + 2) * t ** 3 - (a + 3) * t ** 2 + 1,
                           torch.where(t < 2, a * t ** 3 - 5 * a * t ** 2 + 8 * a * t - 4 * a, torch.zeros_like(t)))
    if name == 'lanczos3':
        px = math.pi * t
        sinc = lambda v: torch.where(v == 0, torch.ones_like(v), torch.sin(v) / v)  # noqa: E731
        return torch.where(t < 3, sinc(px) * sinc(px / 3), torch.zeros_like(t))
    raise ValueError(name)


def taps(filter, F):
    """The float64 taps of a named filter, or the given sequence."""
    if isinstance(filter, str):
        T = SUPPORT[filter] * F
        return phi(filter, (torch.arange(T, dtype=torch.float64) + 0.5 - T / 2) / F)
    return torch.as_tensor(filter, dtype=torch.float64)


def dense_from_taps(filter, H, F):
    """The float64 (H/F, H) matrix of one axis, from the definition."""
    k = taps(filter, F)
    T, n = k.numel(), H // F
    D = torch.zeros(n, H, dtype=torch.float64)
    for q in range(n):
        for j in range(T):
            i = F * q - (T - F) // 2 + j
            if 0 <= i < H:
                D[q, i] += k[j]
    return D / D.sum(dim=1, keepdim=True)


def dense_from_table(A, H, F, dtype=torch.float64):
    """The (n, H) matrix a float32 (n, T) table stands for: the operator the kernel applies, exactly."""
    n, T = A.shape
    D = torch.zeros(n, H, dtype=dtype)
    for q in range(n):
        for j in range(T):
            i = F * q - (T - F) // 2 + j
            if 0 <= i < H:
                D[q, i] += A[q, j].to(dtype)
            else:
                assert A[q, j] == 0, 'a tap outside the axis must have weight 0'
    return D


def view(img, Dy, Dx):
    return Dy @ img @ Dx.transpose(0, 1)


def rho(r, kind, s):
    return r * r if kind == 'mse' else robust_ref.rho(r, kind, s)


def psi(r, kind, s):
    return r if kind == 'mse' else robust_ref.psi(r, kind, s)


def loss_and_grad(img, y, Ay, Ax, F, kind='mse', s=1.0, grad_mul=1.0, dtype=torch.float64):
    """(loss[B], gradient (B,C,H,W), r (B,C,Hs,Ws), view) in ``dtype`` on the CPU from float32 inputs and float32 tables; s is rounded to
    float32 first, as the kernel uses it."""
    s = robust_ref.scale32(s)
    a, t = img.detach().cpu().to(dtype), y.detach().cpu().to(dtype)
    H, W = a.shape[-2:]
    Dy, Dx = dense_from_table(Ay.cpu(), H, F, dtype), dense_from_table(Ax.cpu(), W, F, dtype)
    v = view(a, Dy, Dx)
    r = v - t
    n = r[0].numel()
    gs = (2.0 if kind == 'mse' else 1.0) * grad_mul / n
    g = gs * (Dy.transpose(0, 1) @ psi(r, kind, s) @ Dx)
    return rho(r, kind, s).mean(dim=(1, 2, 3)), g, r, v
