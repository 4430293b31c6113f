"""TEST INFRASTRUCTURE — StyleSpace through the plain oracle: the loss and its gradient with respect to an offset on the
per-channel styles, and the float64 Adam loop on that offset.

The oracle is functional over a parameter dict, and ``oracle.ref_cpu.modulated_conv2d`` computes the style of a layer as
``equal_linear(w_lat, mod_weight, mod_bias)`` with lr_mul 1: s = scale * W w + b.  An offset delta on the style of ONE image is therefore
exactly a replaced modulation bias, b + delta[row : row + channels] — so the helper runs ``oracle.ref_cpu.generator_forward`` one image at a
time with those biases replaced by autograd leaves' slices, and torch autograd hands back dL/ddelta.  Nothing under ``oracle/`` changes.

The loss of an image is oracle.ref_cpu.wplus_loss of its picture plus style_reg * mean_r delta_r^2; Adam and the regulariser's gradient are
written out plainly in float64 (``adam_step``), and checked against torch.optim.Adam in tests/test_sspace_cpu.py."""
import math

import torch

from oracle import ref_cpu as R


def layout(P, size, prefix=''):
    """[(module name, latent index, row offset, channels)] in the generator's execution order (oracle.ref_cpu.generator_forward), the
    channels read off the modulation matrices of ``P``: what ``Generator.style_layout()`` must return."""
    log_size = int(math.log2(size))
    names = [('conv1', 0), ('to_rgb1', 1)]
    for j in range(log_size - 2):
        names += [(f'convs.{2 * j}', 2 * j + 1), (f'convs.{2 * j + 1}', 2 * j + 2), (f'to_rgbs.{j}', 2 * j + 3)]
    out, row = [], 0
    for name, lat in names:
        n = int(P[f'{prefix}{name}.conv.modulation.weight'].shape[0])
        out.append((name, lat, row, n))
        row += n
    return out


def n_rows(P, size, prefix=''):
    name, lat, row, n = layout(P, size, prefix)[-1]
    return row + n


def with_offset(P, size, delta, prefix=''):
    """``P`` with every modulation bias replaced by bias + its slice of ``delta`` (R,): the parameters of ONE image's forward."""
    Q = dict(P)
    for name, lat, row, n in layout(P, size, prefix):
        key = f'{prefix}{name}.conv.modulation.bias'
        Q[key] = P[key] + delta[row:row + n]
    return Q


def forward(P, size, w_row, delta, noises):
    """G of one image at the styles style_affine(w_row) + delta.  w_row (n_latent, 512) or (1, n_latent, 512); delta (R,); noises: that
    image's maps (1,1,r,r).  Everything in the dtype of ``P``."""
    return R.generator_forward(with_offset(P, size, delta), w_row.reshape(1, -1, w_row.shape[-1]), noises, size)


def forward_offset_after(P, size, w_row, delta, noises):
    """The same picture with the offset added AFTER the affine's own rounding, s = fl(fl(scale W w + b) + delta) — where the HIP entry
    oodgan_style_affine_fwd_offset adds it — instead of inside the bias, s = fl(scale W w + fl(b + delta)).  In float64 the two agree to
    1e-16; in float32 their distance is the yardstick of the layout test.  ``oracle.ref_cpu.modulated_conv2d`` takes its style from the
    module's ``equal_linear``: for the length of this call that name is wrapped so that a call with one of the modulation biases of ``P``
    gets its slice of ``delta`` added to the result."""
    slices = {id(P[f'{name}.conv.modulation.bias']): (row, n) for name, lat, row, n in layout(P, size)}
    plain = R.equal_linear

    def patched(x, weight, bias=None, lr_mul=1.0, activation=False):
        out = plain(x, weight, bias, lr_mul, activation)
        hit = slices.get(id(bias))
        return out if hit is None else out + delta[hit[0]:hit[0] + hit[1]]

    R.equal_linear = patched
    try:
        return R.generator_forward(P, w_row.reshape(1, -1, w_row.shape[-1]), noises, size)
    finally:
        R.equal_linear = plain


SLOPE_BAND = 2.0 ** -20


class given_slopes:
    """LeakyReLU has no derivative at 0, and a pre-activation that float32 cannot tell from 0 has no defined slope in a float32
    implementation: the kernels' value there differs from float64's by a few ulp of the layer's largest pre-activation (sums of thousands
    of float32 products), so its sign — and with it 0.2 or 1 as the factor of everything back-propagated through that element — is either
    one.  Inside this context ``oracle.ref_cpu.fused_leaky_relu`` takes, for the elements with |x| <= SLOPE_BAND * max|x| of their layer
    (2^-20: 16 ulp of float32 at the layer maximum), the slope side ``positive[k]`` names (k: the k-th call of a forward pass — conv1,
    convs.0, convs.1, ...: bool (1,C,H,W), True = the x > 0 side), and its own everywhere else: a reference for a float32 implementation that
    asks the same of every element float32 can resolve.  ``adopted`` / ``outside`` count, per layer, the elements of the band whose side
    changed and the elements outside it where ``positive`` disagrees with float64 (those keep float64's side)."""

    def __init__(self, positive, band=SLOPE_BAND):
        self.positive, self.band, self.adopted, self.outside, self.k = positive, band, [], [], 0

    def __enter__(self):
        self.plain = R.fused_leaky_relu

        def patched(x, bias=None, negative_slope=0.2, scale=R.SQRT2):
            if bias is not None:
                x = x + bias.reshape((1, -1) + (1,) * (x.ndim - 2))
            given = self.positive[self.k % len(self.positive)]
            self.k += 1
            xd = x.detach()
            own = xd > 0
            amb = xd.abs() <= self.band * xd.abs().max()
            differs = given != own
            self.adopted.append(int((differs & amb).sum()))
            self.outside.append(int((differs & ~amb).sum()))
            return scale * torch.where(torch.where(amb, given, own), x, negative_slope * x)

        R.fused_leaky_relu = patched
        return self

    def __exit__(self, *exc):
        R.fused_leaky_relu = self.plain


def loss_and_grad(P, size, w_row, delta, target, noises, style_reg=0.0):
    """One image: (total loss, pixel term, mean_r delta_r^2, d total / d delta (R,)) in the dtype of ``P``; the gradient by torch autograd
    through the replaced modulation biases, the regulariser included."""
    dt = P['input.input'].dtype
    d = delta.detach().to(dt).clone().requires_grad_(True)
    img = forward(P, size, w_row.detach().to(dt), d, [n.detach().to(dt) for n in noises])
    pix = R.wplus_loss(img, target.detach().to(dt))
    reg = (d ** 2).mean()
    tot = pix + style_reg * reg
    tot.backward()
    return float(tot.detach()), float(pix.detach()), float(reg.detach()), d.grad.detach()


def adam_step(delta, g, m, v, t, lr, betas=(0.9, 0.999), eps=1e-8):
    """torch.optim.Adam's update (no weight decay, no amsgrad) of step t >= 1, written out: returns (delta, m, v) — new tensors."""
    b1, b2 = betas
    m = b1 * m + (1.0 - b1) * g
    v = b2 * v + (1.0 - b2) * g * g
    step = lr / (1.0 - b1 ** t)
    return delta - step * m / ((v / (1.0 - b2 ** t)).sqrt() + eps), m, v


def invert(P, size, w0, target, noises, steps, lr=0.01, style_reg=0.0, lr_of_step=None, keep=()):
    """The StyleSpace loop in the dtype of ``P``, one image at a time: delta from 0, ``steps`` x {loss_and_grad, adam_step}.
    ``lr_of_step(i)``: the learning rate of zero-based step i (default: ``lr``).  Returns (losses (steps, B), reg (steps, B), delta (B, R),
    {t: delta after step t for t in keep})."""
    dt = P['input.input'].dtype
    B, Rn = w0.shape[0], n_rows(P, size)
    losses, regs = torch.zeros(steps, B, dtype=torch.float64), torch.zeros(steps, B, dtype=torch.float64)
    out, kept = torch.zeros(B, Rn, dtype=dt), {t: torch.zeros(B, Rn, dtype=dt) for t in keep}
    for b in range(B):
        d, m, v = torch.zeros(Rn, dtype=dt), torch.zeros(Rn, dtype=dt), torch.zeros(Rn, dtype=dt)
        nz = [n[b:b + 1] if n.shape[0] == B else n for n in noises]
        for i in range(steps):
            tot, pix, reg, g = loss_and_grad(P, size, w0[b], d, target[b:b + 1], nz, style_reg)
            losses[i, b], regs[i, b] = tot, reg
            d, m, v = adam_step(d, g, m, v, i + 1, lr if lr_of_step is None else lr_of_step(i))
            if i + 1 in kept:
                kept[i + 1][b] = d
        out[b] = d
    return losses, regs, out, kept
