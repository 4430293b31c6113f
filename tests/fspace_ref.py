"""TEST INFRASTRUCTURE — the feature offset of the W+ loop through the plain oracle: the picture at x' = x(w) + delta, the loss
and its gradients with respect to the latent and the offset, and the Adam loop on both.

``oracle.ref_cpu.generator_forward`` reaches every styled conv through the module's name ``styled_conv``: for the length of a call that name
is wrapped so that the ONE call with the prefix ``convs.{l - 1}`` — the up-conv that reads latent l — gets ``delta`` added to its input.
ToRGB of the level below and everything under it keep reading x.  Nothing under ``oracle/`` changes.

The loss of an image is oracle.ref_cpu.wplus_loss of its picture plus feature_reg * mean delta^2; Adam is ``sspace_ref.adam_step``, the update
of torch.optim.Adam written out (checked against it in tests/test_sspace_cpu.py and, on two leaves, in tests/test_fspace_cpu.py)."""
import torch

from oracle import ref_cpu as R

from sspace_ref import SLOPE_BAND, adam_step, given_slopes      # noqa: F401  (re-exported: the GPU tests take both from here)

FEATURE_LAYERS = (3, 5, 7)


def feature_shape(P, l):
    """(C, h, h) of the offset for latent l: the input of convs.{l-1}, whose weight is (1, Co, Ci, 3, 3); h = 4 * 2^((l-1)/2)."""
    return (int(P[f'convs.{l - 1}.conv.weight'].shape[2]), 4 << ((l - 1) // 2), 4 << ((l - 1) // 2))


class offset_input:
    """Inside this context ``oracle.ref_cpu.styled_conv`` adds ``delta`` (1|B, C, h, h) to the input of the call with prefix ``convs.{l-1}``."""

    def __init__(self, l, delta, prefix=''):
        self.name, self.delta = f'{prefix}convs.{l - 1}', delta

    def __enter__(self):
        self.plain = R.styled_conv

        def patched(P, prefix, x, *args, **kw):
            return self.plain(P, prefix, x + self.delta if prefix == self.name else x, *args, **kw)

        R.styled_conv = patched
        return self

    def __exit__(self, *exc):
        R.styled_conv = self.plain


def forward(P, size, w, l, delta, noises):
    """G(w) with the offset on the input of latent l's up-conv; w (B, n_latent, 512), delta (B, C, h, h), in the dtype of ``P``."""
    with offset_input(l, delta):
        return R.generator_forward(P, w, noises, size)


def loss_and_grad(P, size, w_row, l, delta, target, noises, feature_reg=0.0):
    """One image: (total loss, pixel term, mean delta^2, d total / d w (n_latent, 512), d total / d delta (C, h, h)) in the dtype of ``P``,
    by torch autograd, the regulariser included.  w_row (n_latent, 512), delta (C, h, h), target (1, 3, S, S), noises: that image's maps."""
    dt = P['input.input'].dtype
    w = w_row.detach().to(dt).clone().reshape(1, -1, w_row.shape[-1]).requires_grad_(True)
    d = delta.detach().to(dt).clone().reshape((1,) + tuple(delta.shape[-3:])).requires_grad_(True)
    img = forward(P, size, w, l, d, [n.detach().to(dt) for n in noises])
    pix = R.wplus_loss(img, target.detach().to(dt))
    reg = (d ** 2).mean()
    tot = pix + feature_reg * reg
    tot.backward()
    return float(tot.detach()), float(pix.detach()), float(reg.detach()), w.grad.detach()[0], d.grad.detach()[0]


def invert(P, size, w0, l, target, noises, steps, lr=0.01, feature_lr=None, feature_reg=0.0, keep=()):
    """The F/W+ loop in the dtype of ``P``, one image at a time: w from w0, delta from 0, ``steps`` x {loss_and_grad, adam_step on each}.
    Returns (losses (steps, B) float64, reg (steps, B) float64, w (B, n_latent, 512), delta (B, C, h, h), {t: (w, delta) after step t})."""
    dt = P['input.input'].dtype
    flr = lr if feature_lr is None else feature_lr
    B, shape = w0.shape[0], feature_shape(P, l)
    losses, regs = torch.zeros(steps, B, dtype=torch.float64), torch.zeros(steps, B, dtype=torch.float64)
    w_out, d_out = torch.zeros(w0.shape, dtype=dt), torch.zeros((B,) + shape, dtype=dt)
    kept = {t: (torch.zeros_like(w_out), torch.zeros_like(d_out)) for t in keep}
    for b in range(B):
        w, wm, wv = w0[b].detach().to(dt).clone(), torch.zeros(w0.shape[1:], dtype=dt), torch.zeros(w0.shape[1:], dtype=dt)
        d, dm, dv = torch.zeros(shape, dtype=dt), torch.zeros(shape, dtype=dt), torch.zeros(shape, dtype=dt)
        nz = [n[b:b + 1] if n.shape[0] == B else n for n in noises]
        for i in range(steps):
            tot, pix, reg, gw, gd = loss_and_grad(P, size, w, l, d, target[b:b + 1], nz, feature_reg)
            losses[i, b], regs[i, b] = tot, reg
            w, wm, wv = adam_step(w, gw, wm, wv, i + 1, lr)
            d, dm, dv = adam_step(d, gd, dm, dv, i + 1, flr)
            if i + 1 in kept:
                kept[i + 1][0][b], kept[i + 1][1][b] = w, d
        w_out[b], d_out[b] = w, d
    return losses, regs, w_out, d_out, kept
