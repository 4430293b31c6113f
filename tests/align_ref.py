"""Yardstick of the similarity alignment: the definition of include/oodgan.h as dense torch-CPU code, differentiable, in
float64 (``warp(x, theta)``) and as the same formula in float32 (``warp(x, theta, torch.float32)``: the offsets in double from the float32
theta, tau rounded to float32 once, the weights and the 16-tap sum in float32, operation by operation in the order the kernel takes).
``theta_grad`` is autograd's dL/dtheta of a loss whose gradient w.r.t. the warped image is given; ``torch_warp`` is the library call the
definition restates."""
import math

import torch
import torch.nn.functional as F

A = -0.75


def _near(x):
    return ((A + 2.0) * x - (A + 3.0)) * x * x + 1.0


def _far(x):
    return ((A * x - 5.0 * A) * x + 8.0 * A) * x - 4.0 * A


def _axis(d, pos, n, dtype):
    """d (B, n_out...) double offsets of one axis, ``pos`` the integer output coordinate (broadcastable), n the axis length: the four clamped
    tap indices (long) and weights (``dtype``)."""
    lo, hi = -2.0 - pos, n + 1.0 - pos
    d = torch.where(d >= lo, d, lo.expand_as(d))          # a NaN goes to the lower end
    d = torch.where(d <= hi, d, hi.expand_as(d))
    fl = torch.floor(d)
    tau = (d - fl).to(dtype)
    i0 = (pos + fl.detach()).long()
    idx = [(i0 - 1 + k).clamp(0, n - 1) for k in range(4)]
    w = [_far(tau + 1.0), _near(tau), _near(1.0 - tau), _far(2.0 - tau)]
    return idx, w


def offsets(theta, H, W):
    """(du, dv), each (B, H, W) float64 and differentiable in theta (B, 4), whatever theta's dtype (its values are float32 numbers)."""
    th = theta.double()
    e = torch.exp(th[:, 0])
    am1 = (e * torch.cos(th[:, 1]) - 1.0).view(-1, 1, 1)
    s = (e * torch.sin(th[:, 1])).view(-1, 1, 1)
    tu = (th[:, 2] * (0.5 * W)).view(-1, 1, 1)
    tv = (th[:, 3] * (0.5 * H)).view(-1, 1, 1)
    px = (torch.arange(W, dtype=torch.float64) - 0.5 * (W - 1)).view(1, 1, W)
    py = (torch.arange(H, dtype=torch.float64) - 0.5 * (H - 1)).view(1, H, 1)
    du = (am1 * px - (s * (W / H)) * py) + tu
    dv = ((s * (H / W)) * px + am1 * py) + tv
    return du, dv


def warp(x, theta, dtype=torch.float64):
    """x (B, C, H, W), theta (B, 4) -> x_theta (B, C, H, W) in ``dtype``; differentiable in theta and x."""
    B, C, H, W = x.shape
    x = x.to(dtype)
    du, dv = offsets(theta, H, W)
    X = torch.arange(W, dtype=torch.float64).view(1, 1, W)
    Y = torch.arange(H, dtype=torch.float64).view(1, H, 1)
    ix, wx = _axis(du, X, W, dtype)
    iy, wy = _axis(dv, Y, H, dtype)
    flat = x.reshape(B, C, H * W)
    rows = []
    for j in range(4):
        taps = []
        for i in range(4):
            lin = (iy[j] * W + ix[i]).view(B, 1, H * W).expand(B, C, H * W)
            taps.append(torch.gather(flat, 2, lin).view(B, C, H, W))
        wxi = [w.unsqueeze(1) for w in wx]
        rows.append(((wxi[0] * taps[0] + wxi[1] * taps[1]) + wxi[2] * taps[2]) + wxi[3] * taps[3])
    wyj = [w.unsqueeze(1) for w in wy]
    return ((wyj[0] * rows[0] + wyj[1] * rows[1]) + wyj[2] * rows[2]) + wyj[3] * rows[3]


def theta_grad(x, theta, g_out, dtype=torch.float64, reg=0.0):
    """dL/dtheta (B, 4) for L = sum(g_out * warp(x, theta)) + reg * sum theta^2, by autograd; g_out (B, C, H, W) = dL/dx_theta."""
    th = theta.detach().clone().to(torch.float64 if dtype == torch.float64 else torch.float32).requires_grad_(True)
    y = warp(x.detach(), th, dtype)
    L = (g_out.to(dtype) * y).sum() + reg * (th.to(dtype) ** 2).sum()
    return torch.autograd.grad(L, th)[0]


def affine(theta):
    """The (B, 2, 3) matrices [[a, -s, tx], [s, a, ty]] of ``F.affine_grid`` for theta (B, 4), in theta's dtype, differentiable."""
    e = torch.exp(theta[:, 0])
    a, s = e * torch.cos(theta[:, 1]), e * torch.sin(theta[:, 1])
    return torch.stack([torch.stack([a, -s, theta[:, 2]], 1), torch.stack([s, a, theta[:, 3]], 1)], 1)


def torch_warp(x, theta):
    """The library call the definition restates (x, theta of one dtype)."""
    grid = F.affine_grid(affine(theta), list(x.shape), align_corners=False)
    return F.grid_sample(x, grid, mode='bicubic', padding_mode='border', align_corners=False)


def inverse(theta):
    """theta^-1 = (-lambda, -phi, -e^-lambda R(-phi) t) in float64 (B, 4): the yardstick of ``ops.similarity_inverse``."""
    th = theta.double()
    e, c, s = torch.exp(-th[:, 0]), torch.cos(th[:, 1]), torch.sin(th[:, 1])
    tx = -e * (c * th[:, 2] + s * th[:, 3])
    ty = -e * (-s * th[:, 2] + c * th[:, 3])
    return torch.stack([-th[:, 0], -th[:, 1], tx, ty], 1)


def smooth_image(B, C, S, seed, waves=6):
    """A smooth (B, C, S, S) float64 image: ``waves`` random sinusoids per channel, seeded."""
    g = torch.Generator().manual_seed(seed)
    yy, xx = torch.meshgrid(torch.arange(S, dtype=torch.float64), torch.arange(S, dtype=torch.float64), indexing='ij')
    out = torch.zeros(B, C, S, S, dtype=torch.float64)
    for b in range(B):
        for c in range(C):
            for _ in range(waves):
                fx, fy = (torch.rand(2, generator=g, dtype=torch.float64) * 2.0 - 1.0) * 3.0
                ph = torch.rand(1, generator=g, dtype=torch.float64) * 2 * math.pi
                amp = torch.rand(1, generator=g, dtype=torch.float64) * 0.5 + 0.25
                out[b, c] += amp * torch.sin(2 * math.pi * (fx * xx + fy * yy) / S + ph)
    return out / waves ** 0.5
