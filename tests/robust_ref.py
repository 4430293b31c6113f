"""The float64 yardstick of the robust pixel terms of the W+ loss (csrc/loss_pixel.hip): rho(d) and psi(d) = rho'(d) for a
residual d and a scale s, written from the definitions (never from the kernel), in the dtype of ``d`` so that autograd can differentiate
rho.  tests/test_robust_loss_cpu.py chains them to torch's huber_loss, to the Charbonnier closed form and to autograd."""
import torch

KINDS = ('charbonnier', 'huber', 'geman_mcclure')


def scale32(s):
    """The scale the kernel uses: s rounded to float32, as a Python float."""
    return torch.tensor(float(s), dtype=torch.float32).item()


def rho(d, kind, s):
    """rho(d) element by element.  Geman-McClure goes through r = s^2/(d^2 + s^2), never through s^4."""
    if kind == 'charbonnier':
        return torch.sqrt(d * d + s * s)
    if kind == 'huber':
        a = d.abs()
        return torch.where(a <= s, 0.5 * d * d, s * (a - 0.5 * s))
    if kind == 'geman_mcclure':
        return 0.5 * d * d * (s * s / (d * d + s * s))
    raise ValueError(kind)


def psi(d, kind, s):
    """psi(d) = d rho / d d in closed form."""
    if kind == 'charbonnier':
        return d / torch.sqrt(d * d + s * s)
    if kind == 'huber':
        return d.clamp(-s, s)
    if kind == 'geman_mcclure':
        r = s * s / (d * d + s * s)
        return d * r * r
    raise ValueError(kind)


def loss_and_grad(img, target, kind, s, beta=None, grad_mul=1.0, wrt='gen'):
    """float64 (loss[B], gradient, c) of the per-image mean of rho(d) on float32 inputs: d = img - target, or beta*(img - target) on the
    composite c = target + d.  The gradient is grad_mul/CHW * psi(d), times beta once more for ``wrt='gen'``; s is rounded to float32 first."""
    s = scale32(s)
    a, t = img.detach().cpu().double(), target.detach().cpu().double()
    d = a - t
    w = None if beta is None else beta.detach().cpu().double()
    if w is not None:
        d = w * d
    n = d[0].numel()
    g = grad_mul / n * psi(d, kind, s)
    if w is not None and wrt == 'gen':
        g = g * w
    return rho(d, kind, s).mean(dim=(1, 2, 3)), g, t + d
