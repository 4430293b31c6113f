"""Yardstick of the colour map of the W+ loop: the definition of include/oodgan.h as dense torch-CPU code in float64 by
default.  theta (B, 12) = (M row-major 3x3, b) per image, the identity (I, 0); images have C = 3.
    c_i(p) = sum_j M_ij G_j(p) + b_i                                    the mapped image
    d = c - x, or beta (c - x) with a loss weight beta (B,1,H,W);       loss[b] = mean over 3 H W of rho(d)
    g_i = gscale psi(d_i), times beta once more with a loss weight;     gscale = grad_mul / (3 H W), twice that for the square
    gimg_j = sum_i M_ij g_i                                             what the backward receives
    dL/dM_ij = sum_p g_i G_j / grad_div,  dL/db_i = sum_p g_i / grad_div
    the regulariser mu sum_k (theta_k - id_k)^2 adds 2 mu (theta_k - id_k); a number that is not free has gradient 0
``term`` writes these formulas out (no autograd); ``formula`` is the same loss as a differentiable einsum expression in any dtype, which
the tests differentiate with autograd — in float64 to check ``term``, in float32 to set the error bar of the kernels."""
import math

import torch

KINDS = ('mse', 'charbonnier', 'huber', 'geman_mcclure')
IDENTITY = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0)
FREE = {'affine': 0xfff, 'gain': 0xf11}           # bit k: theta_k is free ('gain': the diagonal of M and b)
# the two maps of the recovery tests and of the fixture: a gain/offset and a full matrix
THETA_STAR = ((1.15, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.85, 0.05, 0.0, -0.05),
              (0.80, 0.15, 0.05, 0.10, 0.75, 0.05, 0.05, 0.10, 0.60, -0.04, 0.02, 0.06))


def identity(B, dtype=torch.float32):
    return torch.tensor(IDENTITY, dtype=dtype).repeat(B, 1)


def free_mask(kind, dtype=torch.float64):
    """The 12 zeros and ones of a kind."""
    return torch.tensor([(FREE[kind] >> k) & 1 for k in range(12)], dtype=dtype)


def split(theta):
    """theta (B, 12) -> M (B, 3, 3), b (B, 3)."""
    return theta[:, :9].reshape(-1, 3, 3), theta[:, 9:]


def apply(img, theta):
    """C_theta(img): (B, 3, H, W) in img's dtype; differentiable in both."""
    M, b = split(theta.to(img.dtype))
    return torch.einsum('bij,bjhw->bihw', M, img) + b.view(-1, 3, 1, 1)


def rho_psi(d, kind, s):
    """rho(d) and psi(d) = rho'(d) of the pixel terms, elementwise; s a python float (used as its float32 value)."""
    if kind == 'mse':
        return d * d, d
    s = torch.tensor(float(s), dtype=torch.float32).item()         # the scale the kernel uses: s rounded to float32
    s2 = s * s
    if kind == 'charbonnier':
        q = torch.sqrt(d * d + s2)
        return q, d / q
    if kind == 'huber':
        a = d.abs()
        return torch.where(a <= s, 0.5 * d * d, s * (a - 0.5 * s)), d.clamp(-s, s)
    r = s2 / (d * d + s2)
    return 0.5 * d * d * r, d * r * r


def formula(img, x, theta, kind='mse', s=0.1, beta=None):
    """loss (B,) as one differentiable expression in img's dtype: the per-image mean of rho(beta (C_theta(img) - x))."""
    d = apply(img, theta) - x
    if beta is not None:
        d = beta * d
    return rho_psi(d, kind, s)[0].flatten(1).mean(1)


def term(img, x, theta, kind='mse', s=0.1, beta=None, grad_mul=1.0, grad_div=1.0, free='affine', reg=0.0, dtype=torch.float64):
    """(loss (B,), gimg (B,3,H,W), dtheta (B,12), reg_sum (B,)) of the definition, written out in ``dtype``: gimg = grad_mul d(sum_b loss_b)/d(img),
    dtheta = grad_mul / grad_div d(sum_b loss_b)/d(theta) + 2 reg (theta - id), zero where ``free`` has no bit; reg_sum = sum_k (theta_k - id_k)^2."""
    img, x, th = img.to(dtype), x.to(dtype), theta.to(dtype)
    B, C, H, W = img.shape
    assert C == 3
    M, _ = split(th)
    d = apply(img, th) - x
    if beta is not None:
        d = beta.to(dtype) * d
    rho, psi = rho_psi(d, kind, s)
    gscale = grad_mul / (C * H * W) * (2.0 if kind == 'mse' else 1.0)
    g = gscale * psi
    if beta is not None:
        g = g * beta.to(dtype)
    gimg = torch.einsum('bij,bihw->bjhw', M, g)
    dM = torch.einsum('bihw,bjhw->bij', g, img) / grad_div
    db = g.sum((2, 3)) / grad_div
    off = th - identity(B, dtype)
    dth = (torch.cat([dM.reshape(B, 9), db], 1) + 2.0 * reg * off) * free_mask(free, dtype)
    return rho.flatten(1).mean(1), gimg, dth, (off * off).sum(1)


def autograd_term(img, x, theta, kind='mse', s=0.1, beta=None, dtype=torch.float64):
    """(loss, d(sum loss)/d(img), d(sum loss)/d(theta)) of ``formula`` by torch autograd in ``dtype``."""
    a = img.to(dtype).clone().requires_grad_(True)
    th = theta.to(dtype).clone().requires_grad_(True)
    loss = formula(a, x.to(dtype), th, kind, s, None if beta is None else beta.to(dtype))
    ga, gt = torch.autograd.grad(loss.sum(), (a, th))
    return loss.detach(), ga, gt


def inverse(theta):
    """theta^-1 = (M^-1, -M^-1 b) in float64 (B, 12): the yardstick of ``ops.color_inverse``."""
    M, b = split(theta.double())
    Mi = torch.linalg.inv(M)
    return torch.cat([Mi.reshape(-1, 9), -(Mi @ b.unsqueeze(-1)).squeeze(-1)], 1)


def lr_multiplier(i, total_steps, rampup=0.0, rampdown=0.0):
    """The loop's ramp factor r(i) (csrc/wplus_sched.hip)."""
    tau, r = i / total_steps, 1.0
    if rampdown > 0.0:
        r = min(1.0, (1.0 - tau) / rampdown)
        r = 0.5 - 0.5 * math.cos(math.pi * r)
    if rampup > 0.0:
        r *= min(1.0, tau / rampup)
    return r


def adam(theta, g, m, v, t, lr, betas=(0.9, 0.999), eps=1e-8, free='affine', total_steps=100, rampup=0.0, rampdown=0.0):
    """One float64 Adam step of the loop (t = 1, 2, ...) on the free numbers; returns (theta, m, v)."""
    f = free_mask(free, torch.float64)
    b1, b2 = float(torch.tensor(betas[0], dtype=torch.float32)), float(torch.tensor(betas[1], dtype=torch.float32))
    m2 = torch.where(f > 0, m + (g - m) * (1.0 - b1), m)
    v2 = torch.where(f > 0, v * b2 + (1.0 - b2) * g * g, v)
    step = lr * lr_multiplier(t - 1, total_steps, rampup, rampdown) / (1.0 - b1 ** t)
    upd = step * m2 / (v2.sqrt() / math.sqrt(1.0 - b2 ** t) + eps)
    return torch.where(f > 0, theta - upd, theta), m2, v2


def smooth_image(B, C, S, seed, waves=6):
    """A smooth (B, C, S, S) float64 image: ``waves`` random sinusoids per channel, seeded (the image of the alignment's recovery test)."""
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
