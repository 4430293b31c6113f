"""The float64 references of tests/tail_ref.py are not circular: the backward references equal autograd of the forward formulas, and the
integer data sets of tests/test_hip_style_tail.py lie in the regime where float32 sums are exact in any order.  No GPU."""
import math

import pytest
import torch

import tail_ref as T

F64 = torch.float64


def test_demod_bwd_reference_is_autograd_of_demod():
    """d = rsqrt(scale^2 sum_ci s^2 wsq + 1e-8), upstream gradient gd, r = gd * d"""
    for B, Ci, Co, scale in [(3, 65, 5, 0.25), (1, 1, 1, 1.0), (2, 130, 1030, 0.03)]:
        s = T.normal((B, Ci), 1).to(F64).requires_grad_(True)
        wsq = T.normal((Co, Ci), 2).to(F64) ** 2
        gd = T.normal((B, Co), 3).to(F64)
        d = torch.rsqrt((scale * scale) * ((s ** 2) @ wsq.t()) + 1e-8)
        (g,) = torch.autograd.grad(d, s, gd)
        ref = T.demod_bwd(s.detach(), wsq, d.detach(), gd * d.detach(), scale)
        assert torch.allclose(ref, g, rtol=1e-12, atol=1e-14 * g.abs().max().item())
        assert torch.equal(T.demod_fwd(s.detach(), wsq, scale), d.detach())


def test_style_affine_bwd_reference_is_autograd_of_forward():
    for B, L, S, lat_start, lr_mul, grad_div in [(3, 4, 100, [0, 16, 16, 60, 77], 0.5, 4.0), (2, 1, 64, [0, 5], 1.0, 1.0)]:
        R = lat_start[-1]
        lat = T.normal((B, L, S), 4).to(F64).requires_grad_(True)
        w, bias, gs = T.normal((R, S), 5).to(F64), T.normal((R,), 6).to(F64), T.normal((B, R), 7).to(F64)
        s, _ = T.style_affine(lat, w, bias, T.row_lat_of(lat_start, R), lr_mul)
        (g,) = torch.autograd.grad(s, lat, gs)
        ref = T.style_affine_backward(gs, w, lat_start, L, lr_mul, grad_div)
        assert torch.allclose(ref * grad_div, g, rtol=1e-12, atol=1e-13)
        if L == 4:          # latent 1 has no rows
            assert torch.equal(ref[:, 1], torch.zeros(B, S, dtype=F64)) and torch.equal(g[:, 1], torch.zeros(B, S, dtype=F64))


def test_style_affine_forward_reference_rows():
    """the einsum against a plain loop over rows, with a row_lat that changes inside a group of 16"""
    B, L, S, R = 2, 3, 33, 20
    lat, w, bias = T.normal((B, L, S), 8), T.normal((R, S), 9), T.normal((R,), 10)
    rl = [1] * 7 + [0] * 9 + [2] * 4
    s, bound = T.style_affine(lat, w, bias, rl, 0.5)
    for r in range(R):
        e = (lat[:, rl[r]].to(F64) * w[r].to(F64)).sum(1) * (0.5 / math.sqrt(S)) + bias[r].to(F64) * 0.5
        assert torch.allclose(s[:, r], e, rtol=1e-13, atol=1e-15)
    assert (bound >= s.abs() - 1e-15).all()


def test_range_exp_reference_meets_the_contract():
    m = T.contract_values()
    sc = torch.tensor([2.0 ** T.range_exp(v) for v in m.tolist()], dtype=torch.float32)
    assert T.contract_ok(m, sc, 1.0 / sc).all()
    assert T.range_exp(0.0) == 0 and T.range_exp(math.inf) == 0 and T.range_exp(math.nan) == 0
    assert T.range_exp(2.0 ** -140) == 100 and T.range_exp(2.0 ** 120) == -100
    # the contract test itself can fail: an exponent taken from a correctly rounded float32 log2 breaks it just below 2^k
    import numpy as np
    bad = torch.tensor([2.0 ** (9 - int(np.floor(np.log2(np.float32(v))))) for v in m.tolist()], dtype=torch.float32)
    assert not T.contract_ok(m, bad).all()


# every integer-valued term set of the exact comparisons of tests/test_hip_style_tail.py: name -> terms (..., n), the products a kernel sums
def _exact_sets():
    import test_hip_style_tail as G
    return G.exact_term_sets()


def test_integer_data_sets_are_in_the_exact_regime():
    sets = _exact_sets()
    assert len(sets) >= 8
    for name, terms in sets.items():
        assert terms.dtype == torch.float32, name
        assert T.exact_regime(terms), name


def test_exact_regime_check_can_fail():
    assert not T.exact_regime(torch.tensor([[2.0 ** 24, 1.0, 1.0, -2.0 ** 24]]))
    assert not T.exact_regime(torch.tensor([[1.0, 2.0 ** -24, 2.0 ** -24]]))
    assert T.exact_regime(torch.tensor([[4.0, -3.0, 0.25]]))
