"""The cases that pin the pixel terms of the W+ loss (csrc/loss_pixel.hip) to the commit before their kernels became one family: what
tests/golden/make_pixel_terms_parent.py records with that commit's library and tests/test_hip_pixel_terms_parent.py recomputes.

Every case runs one of ``ops.mse_loss_grad`` / ``ops.composite_mse_loss_grad`` / ``ops.robust_loss_grad`` on seeded inputs and yields the
float32 loss values (bits) and the SHA-256 of the raw bytes of the gradient and of the composite where one is written."""
import hashlib

import numpy as np
import torch

from oodgan import synth

B, SCALE = 2, 0.5
# C, H, W: the smallest shapes at which each branch of the walk can go wrong
SHAPES = {
    'plane': (3, 128, 256),     # plane form with beta (HW = 2 * 16384): two chunks per channel plane, partial index c*chunks + j
    'flat4': (3, 96, 96),       # flat float4 form, the second chunk partial
    'scalar': (3, 37, 37),      # scalar form (HW % 4 != 0)
    'chw4': (4, 5, 5),          # CHW % 4 == 0, HW % 4 != 0: the MSE entry takes float4, the beta and robust entries the scalar form
}
KINDS = ('charbonnier', 'huber', 'geman_mcclure')


def inputs(shape):
    """Seeded img, target (B,C,H,W) and a non-binary loss weight (B,1,H,W) in [0,1] with exact zeros and ones (no transcendental: the same
    bits on every host)."""
    C, H, W = shape
    img = synth.normal('pixel_terms.img', (B, C, H, W), 1)
    x = synth.normal('pixel_terms.x', (B, C, H, W), 2, std=0.5)
    beta = (0.5 + 0.4 * synth.normal('pixel_terms.beta', (B, 1, H, W), 3)).clamp_(0.0, 1.0)
    assert (beta == 0).any() and (beta == 1).any() and ((beta > 0) & (beta < 1)).any()
    return img, x, beta.contiguous()


def _sha(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).digest()


def run(ops, shape, dev):
    """All cases of one shape: ({key: float32 loss values}, {key: 32-byte digest})."""
    img, x, beta = inputs(shape)
    a, t, w = img.to(dev), x.to(dev), beta.to(dev)
    gmul = ops.loss_scale_for(a[0].numel())
    losses, digests = {}, {}

    def put(key, loss, g=None, c=None):
        losses[key] = loss.detach().cpu().numpy().astype(np.float32, copy=True).ravel()
        if g is not None:
            digests[key + '/g'] = _sha(g)
        if c is not None:
            digests[key + '/c'] = _sha(c)

    put('mse', *ops.mse_loss_grad(a, t, gmul))
    for wrt in ('gen', 'composite'):
        for comp in (False, True):
            loss, g, c = ops.composite_mse_loss_grad(a, t, w, gmul, wrt=wrt, composite=comp)
            assert (c is not None) == comp
            put(f'composite_mse/{wrt}/c{int(comp)}', loss, g, c)
    for kind in KINDS:
        put(f'{kind}/plain', *ops.robust_loss_grad(a, t, kind, SCALE, grad_mul=gmul))
        loss, g, _ = ops.robust_loss_grad(a, t, kind, SCALE, grad_mul=gmul, grad=False)
        assert g is None
        put(f'{kind}/plain/fwd', loss)
        for wrt in ('gen', 'composite'):
            put(f'{kind}/beta/{wrt}', *ops.robust_loss_grad(a, t, kind, SCALE, w, gmul, wrt=wrt, composite=wrt == 'composite'))
        loss, g, c = ops.robust_loss_grad(a, t, kind, SCALE, w, gmul, composite=True, grad=False)
        assert g is None
        put(f'{kind}/beta/fwd', loss, None, c)
    # the loss-table form, one case per entry point: rows 2 and 9 (clamped to 3) of a 4-row table; the whole table is the loss value
    table_calls = {'mse': lambda **kw: ops.mse_loss_grad(a, t, gmul, **kw),
                   'composite_mse': lambda **kw: ops.composite_mse_loss_grad(a, t, w, gmul, **kw)[:2],
                   'huber': lambda **kw: ops.robust_loss_grad(a, t, 'huber', SCALE, w, gmul, **kw)[:2]}
    for name, call in table_calls.items():
        table = torch.full((4, B), -1.0, device=dev)
        for row in (2, 9):
            none, g = call(table=table, row_dev=torch.tensor([row], dtype=torch.int32, device=dev))
            assert none is None
            put(f'{name}/table/row{row}', table, g)
    return losses, digests
