"""TEST INFRASTRUCTURE — the fitted out-of-domain mask of the W+ loop (loss_region='fit') in plain torch, in whatever dtype
it is handed (the tests use float64).

The objective of one image: logits l (1,1,m,m), a = sigmoid(l), beta = U(a) with U = F.interpolate(size=(S,S), mode='bilinear',
align_corners=False), c = x + beta*(G - x),

    L = mean (c - x)^2  [+ other terms on c]  + lambda_a * max(0, mean(1 - a) - A) + lambda_b * mean(min(a, 1 - a)).

The last two are the reference's MaskLoss (src/losses/mask_loss.py) with target 1 on alpha = 1 - a; torch's subgradients: the hinge 0 at a
tie (Python's max returns the zero tensor there), min 0 at a = 1/2.  ``ut_gather`` is U's adjoint written out as the gather the HIP step
performs, ``adam_step`` is sspace_ref's (torch.optim.Adam written out)."""
import torch
import torch.nn.functional as F

from sspace_ref import adam_step      # noqa: F401  (re-exported)

DEFAULTS = dict(area=0.30, area_weight=5.0, binary_weight=0.2, mask_lr=0.1, mask_init=0.88)


def upsample(a, S):
    """beta = U(a): (B,1,m,m) -> (B,1,S,S)."""
    return F.interpolate(a, size=(S, S), mode='bilinear', align_corners=False)


def tent_matrix(S, m, dtype=torch.float64):
    """W (S, m): W[y, j] = the weight pixel y gives cell j along one axis — the tent about the source coordinate (y + 0.5) * m / S - 0.5
    clamped to [0, m - 1] (the lower clamp is F.interpolate's; the upper one is what its index clamp amounts to).  U(a) = W a W^T."""
    src = ((torch.arange(S, dtype=dtype) + 0.5) * (m / S) - 0.5).clamp(0.0, m - 1.0)
    return (1.0 - (src[:, None] - torch.arange(m, dtype=dtype)[None, :]).abs()).clamp_min(0.0)


def ut_gather(e, m):
    """U^T e per cell by gather: e (B,1,S,S) -> (B,1,m,m).  Cell (j, i) adds, over its own support — pixel rows [F j - F/2, F j + 3F/2) and
    columns likewise, clipped to the image: at most 2F x 2F pixels — e times the two tent weights; the clamped edge rows and columns fall to
    the edge cells with their whole weight."""
    B, _, S, _ = e.shape
    f = S // m
    W = tent_matrix(S, m, e.dtype)
    out = torch.zeros(B, 1, m, m, dtype=e.dtype)
    for j in range(m):
        y0, y1 = max(f * j - f // 2, 0), min(f * j + f + f // 2, S)
        assert not W[:y0, j].any() and not W[y1:, j].any()          # nothing outside the support
        rows = (W[y0:y1, j][None, None, :, None] * e[:, :, y0:y1, :]).sum(2)      # (B,1,S)
        for i in range(m):
            x0, x1 = max(f * i - f // 2, 0), min(f * i + f + f // 2, S)
            out[:, 0, j, i] = (rows[:, 0, x0:x1] * W[x0:x1, i][None, :]).sum(1)
    return out


def regulariser(a, area):
    """(hinge, binary) per image of a (B,1,m,m): max(0, mean(1 - a) - area) and mean(min(a, 1 - a)), differentiable (torch's subgradients)."""
    over = (1.0 - a).mean(dim=(1, 2, 3)) - area
    hinge = torch.where(over > 0, over, torch.zeros_like(over))
    return hinge, torch.minimum(a, 1.0 - a).mean(dim=(1, 2, 3))


def regulariser_grad(a, area, area_weight, binary_weight):
    """d(area_weight * hinge + binary_weight * binary)/da written out: -area_weight / m^2 where mean(1 - a) > area (0 at the tie) plus
    +-binary_weight / m^2 on either side of 1/2 (0 at 1/2)."""
    n = a[0].numel()
    open_ = ((1.0 - a).mean(dim=(1, 2, 3), keepdim=True) - area > 0).to(a.dtype)
    return -area_weight / n * open_ * torch.ones_like(a) + binary_weight / n * torch.sign(0.5 - a)


def objective(l, gen, x, area, area_weight, binary_weight, extra=None):
    """Per image: (total, pixel, hinge, binary, beta) for logits l (B,1,m,m), generator images gen and targets x (B,C,S,S); ``extra(c, x)``:
    a further per-image term on the composite, added to the total."""
    a = torch.sigmoid(l)
    beta = upsample(a, x.shape[-1])
    c = x + beta * (gen - x)
    pix = ((c - x) ** 2).mean(dim=(1, 2, 3))
    hinge, binary = regulariser(a, area)
    tot = pix + area_weight * hinge + binary_weight * binary
    if extra is not None:
        tot = tot + extra(c, x)
    return tot, pix, hinge, binary, beta
