"""TEST INFRASTRUCTURE — the W+ loop's per-step gradient, read back from the running inverter and checked in float64.

``WPlusInverter`` never hands its gradient dL/dW+ to the caller: every step runs G(w), the loss (engine._WRun._loss_grad), the backward pass and Adam on the device
(steps 4..N replayed from a launch plan).  What the caller can see after each step is (t, w, m) through ``inv.on_step``, and Adam's first
moment is a lerp of the gradient (csrc/elementwise.hip, adam_dev_kernel — the loop's step index is a device counter in every mode:
``m + (g - m) * (1 - beta1)`` in fp32), so

    g_t = m_{t-1} + (m_t - m_{t-1}) / (1 - beta1)

recovers every step's gradient to within 1e-6 of its max (tests/test_wplus_grad_recovery.py), far below the kernels' own error.  The gradient at
step t belongs to the latents w_{t-1}, and ``oracle_grad`` evaluates it there through the plain float64 oracle (oracle.ref_cpu).

The loss is a sum of per-image means (oracle.ref_cpu.wplus_loss), so one image's gradient does not depend on the batch or sub-batch it sits
in: the oracle runs one image at a time."""
import time

import numpy as np
import torch

from oracle import ref_cpu as R


class Capture:
    """(w_t, m_t) of every (sub-)batch after every enqueued step, and w_0 / the cut points of the batch (engine.WPlusInverter._split)."""

    def __init__(self):
        self.steps = {}         # run index (= stream index) -> {t: (w, m)} on the run's device
        self.w0 = None
        self.cuts = None

    def locate(self, k):
        """(run index, row in that run's sub-batch) of image k of the batch."""
        for i in range(len(self.cuts) - 1):
            if self.cuts[i] <= k < self.cuts[i + 1]:
                return i, k - self.cuts[i]
        raise IndexError(k)

    def w(self, k, t):
        """latents of image k after step t (t = 0: the start latents), float64 on the CPU."""
        if t == 0:
            return self.w0[k].double().cpu()
        i, j = self.locate(k)
        return self.steps[i][t][0][j].double().cpu()

    def m(self, k, t):
        """Adam's first moment of image k after step t (zero before the first step), as stored: float32 on the CPU."""
        if t == 0:
            return torch.zeros_like(self.w0[k]).cpu()
        i, j = self.locate(k)
        return self.steps[i][t][1][j].cpu()

    def grad(self, k, t, beta1):
        """the gradient step t applied to image k (at w_{t-1}), recovered from Adam's first moment."""
        return recover_grad(self.m(k, t - 1), self.m(k, t), beta1)


def capture(inv):
    """Install ``inv.on_step`` (and wrap ``inv.invert`` to keep w_0 and the sub-batch cut points); returns the ``Capture`` it fills.

    The callback runs under the run's stream (engine._WRun.advance), so each clone is ordered after the step it follows, replayed steps
    included; synchronise before reading.  A rolled-back window would enqueue the same t twice: callers assert ``inv.last_stats`` shows none."""
    cap = Capture()

    def on_step(run):
        i = next(n for n, r in enumerate(inv._runs) if r is run)
        cap.steps.setdefault(i, {})[run.t] = (run.w.clone(), run.m.clone())

    invert = inv.invert

    def wrapped(target, w0, noises, steps=100, return_trajectory=False, streams=1, use_graph=False):
        B = w0.shape[0]
        ns = max(1, min(int(streams), B))
        cap.steps.clear()
        cap.w0 = w0.detach().clone()
        cap.cuts = [(i * B) // ns for i in range(ns + 1)]          # as engine.WPlusInverter._split cuts the batch
        return invert(target, w0, noises, steps=steps, return_trajectory=return_trajectory, streams=streams, use_graph=use_graph)

    inv.on_step = on_step
    inv.invert = wrapped
    return cap


def recover_grad(m_prev, m_cur, beta1):
    """Invert the fp32 lerp of Adam's first moment, m_cur = m_prev + (g - m_prev) * (1 - beta1), in float64 with the float32 value of
    1 - beta1 (the kernel computes ``1.f - beta1`` in float32)."""
    c = float(np.float32(1.0) - np.float32(beta1))
    mp = m_prev.double()
    return mp + (m_cur.double() - mp) / c


def oracle_grad(size, state, w_row, target, noises):
    """Loss and dL/dw of ONE image through the float64 oracle.  ``w_row`` (n_latent, 512) or (1, n_latent, 512); ``target`` (1, 3, H, W);
    ``noises``: that image's noise maps, each (1, 1, r, r).  ``state`` may already be float64 (callers convert it once per size).
    Returns (loss, grad (n_latent, 512) float64, seconds)."""
    t0 = time.time()
    P = {k: (v if v.dtype == torch.float64 else v.double()) for k, v in state.items()}
    w = w_row.detach().double().cpu().reshape(1, -1, w_row.shape[-1]).clone().requires_grad_(True)
    img = R.generator_forward(P, w, [n.detach().double().cpu() for n in noises], size)
    loss = R.wplus_loss(img, target.detach().double().cpu())
    loss.backward()
    return float(loss.detach()), w.grad[0].detach(), time.time() - t0


def row_layers(r, n_latent):
    """The generator layers latent row r modulates (oracle.ref_cpu.generator_forward)."""
    if r == 0:
        return ['conv1']
    k, odd = (r - 1) // 2, (r - 1) % 2 == 0
    if not odd:                                     # row 2k + 2
        return [f'convs.{2 * k + 1}']
    out = [] if r == n_latent - 1 else [f'convs.{2 * k}']
    out.append('to_rgb1' if k == 0 else f'to_rgbs.{k - 1}')
    return out


def row_label(r, n_latent):
    """'row 5 [convs.4 (up-conv to 32²), to_rgbs.1 (16²)]' — the resolution level names the kernel family a per-row error points at."""
    parts = []
    for name in row_layers(r, n_latent):
        if name == 'conv1':
            parts.append('conv1 (4²)')
        elif name.startswith('convs.'):
            j = int(name.split('.')[1])
            res = 2 ** (j // 2 + 3)
            parts.append(f'{name} ({"up-conv to " if j % 2 == 0 else "conv "}{res}²)')
        elif name == 'to_rgb1':
            parts.append('to_rgb1 (4²)')
        else:
            parts.append(f'{name} ({2 ** (int(name.split(".")[1]) + 3)}²)')
    return f'row {r} [' + ', '.join(parts) + ']'


def row_errors(g, g_ref):
    """(max|g - g_ref| / max|g_ref|, [the same ratio within each latent row]) for gradients of shape (n_latent, 512)."""
    g, g_ref = g.double().cpu(), g_ref.double().cpu()
    assert g.shape == g_ref.shape and g.dim() == 2, (g.shape, g_ref.shape)
    d = (g - g_ref).abs()
    glob = float(d.max() / g_ref.abs().max())
    rows = (d.amax(dim=1) / g_ref.abs().amax(dim=1)).tolist()
    return glob, rows


def recipe(size, gidx):
    """bench.py's synthetic inputs for the global image indices ``gidx`` (CPU tensors): target, start latents, noise maps."""
    from oodgan import synth
    cat = lambda parts: torch.cat(parts, 0)
    target = cat([synth.make_images(size, 1, seed=1000 + g) for g in gidx])
    w0 = cat([synth.make_latents(size, 1, seed=3000 + g, std=0.3) for g in gidx])
    per = [synth.make_noises(size, 1, seed=2000 + g) for g in gidx]
    noises = [cat([n[i] for n in per]) for i in range(len(per[0]))]
    return target, w0, noises
