"""tests/wplus_grads.recover_grad reads the W+ loop's per-step gradient back out of Adam's first moment.  Here, without a GPU: the fp32
lerp of csrc/elementwise.hip's adam kernels (``m + (g - m) * (1.f - beta1)``, rounded after the product or contracted into one fma) and
torch.optim.Adam's own exp_avg, over 100 steps of gradients whose rows span three decades and change sign — g comes back within 1e-6 of
max|g|, globally and in every latent row, i.e. far below the 1e-5 .. 1e-4 the kernels' gradients differ from float64 by."""
import numpy as np
import pytest
import torch

from wplus_grads import recover_grad, row_errors, row_layers, row_label

STEPS, B, ROWS, DIM = 100, 2, 18, 512
BETA1 = 0.9


def _gradients(seed=0):
    """(STEPS, B, ROWS, DIM) float32: per-row scales from 1 down to 1e-3, a slow oscillation (every coordinate changes sign several times)
    plus noise, and a few coordinates that jump by 10x for one step."""
    gen = torch.Generator().manual_seed(seed)
    scale = torch.logspace(0, -3, ROWS, dtype=torch.float64).view(1, 1, ROWS, 1)
    phase = torch.rand(1, B, ROWS, DIM, generator=gen, dtype=torch.float64) * 6.3
    freq = 0.05 + 0.3 * torch.rand(1, B, ROWS, DIM, generator=gen, dtype=torch.float64)
    t = torch.arange(STEPS, dtype=torch.float64).view(STEPS, 1, 1, 1)
    g = torch.sin(phase + freq * t) + 0.5 * torch.randn(STEPS, B, ROWS, DIM, generator=gen, dtype=torch.float64)
    spikes = torch.rand(STEPS, B, ROWS, DIM, generator=gen) < 1e-3
    g = torch.where(spikes, 10 * g, g)
    return (g * scale).float()


def _kernel_lerp(m, g, fma):
    c = np.float32(1.0) - np.float32(BETA1)
    if fma:     # one rounding: the compiler may contract the kernel's multiply-add
        return (m.double() + (g.double() - m.double()) * float(c)).float()
    return m + (g - m) * torch.tensor(c, dtype=torch.float32)


def _check(g_seq, m_seq, tag):
    worst_glob, worst_row = 0.0, 0.0
    for t in range(STEPS):
        m_prev = m_seq[t - 1] if t > 0 else torch.zeros_like(m_seq[0])
        rec = recover_grad(m_prev, m_seq[t], BETA1)
        for b in range(B):
            glob, rows = row_errors(rec[b], g_seq[t, b].double())
            worst_glob, worst_row = max(worst_glob, glob), max(worst_row, max(rows))
    print(f'[{tag}] {STEPS} steps: recovered g within {worst_glob:.2e} of max|g| (worst latent row {worst_row:.2e})')
    assert worst_glob < 1e-6 and worst_row < 1e-6, (worst_glob, worst_row)
    assert g_seq.abs().amax(dim=(0, 1, 3)).max() / g_seq.abs().amax(dim=(0, 1, 3)).min() > 500      # three decades between the rows


@pytest.mark.parametrize('fma', [False, True])
def test_recover_grad_inverts_the_kernels_fp32_lerp(fma):
    g = _gradients(seed=1 + fma)
    m, ms = torch.zeros(B, ROWS, DIM), []
    for t in range(STEPS):
        m = _kernel_lerp(m, g[t], fma)
        ms.append(m.clone())
    _check(g, ms, f'adam kernel lerp, {"fma" if fma else "two roundings"}')


def test_recover_grad_inverts_torch_adam_exp_avg():
    """torch.optim.Adam (the reference's optimiser) keeps exp_avg with lerp_(grad, 1 - beta1): weight 0.1 in float32 instead of the
    kernel's 1.f - 0.9f — 2.4e-7 apart, still within the bar."""
    g = _gradients(seed=3)
    w = torch.zeros(B, ROWS, DIM, requires_grad=True)
    opt = torch.optim.Adam([w], lr=0.01, betas=(BETA1, 0.999), eps=1e-8)
    ms = []
    for t in range(STEPS):
        w.grad = g[t].clone()
        opt.step()
        ms.append(opt.state[w]['exp_avg'].detach().clone())
    _check(g, ms, 'torch.optim.Adam exp_avg')


def test_row_errors_and_row_map():
    """row_errors normalises each latent row by its own max; the row -> layer map follows oracle.ref_cpu.generator_forward."""
    ref = torch.ones(18, 512, dtype=torch.float64)
    ref[5] *= 1e-3
    g = ref.clone()
    g[5, 7] += 1e-6
    glob, rows = row_errors(g, ref)
    assert glob == pytest.approx(1e-6) and rows[5] == pytest.approx(1e-3) and max(rows[:5] + rows[6:]) == 0
    assert row_layers(0, 18) == ['conv1']
    assert row_layers(1, 18) == ['convs.0', 'to_rgb1']
    assert row_layers(2, 18) == ['convs.1']
    assert row_layers(15, 18) == ['convs.14', 'to_rgbs.6']
    assert row_layers(16, 18) == ['convs.15']
    assert row_layers(17, 18) == ['to_rgbs.7']
    assert row_layers(13, 14) == ['to_rgbs.5']
    # every layer of the 1024² generator is modulated by exactly one row
    names = [n for r in range(18) for n in row_layers(r, 18)]
    assert len(names) == len(set(names)) == 1 + 16 + 1 + 8
    assert 'up-conv to 1024²' in row_label(15, 18) and 'conv 1024²' in row_label(16, 18)
