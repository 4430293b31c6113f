"""The P_N+ prior of the W+ loop, the parts that need no GPU: the option checks of the engine and of the CLI's ``inversion``
block, the float64 yardstick tests/pn_ref.py against a case worked by hand, ``PNStats`` against the yardstick, and the refusal of
statistics whose variances are not positive."""
import pytest
import torch

from oodgan import cli
from oodgan.engine import WPlusInverter, check_pn, check_pn_options
from oodgan.pn import PNStats, leaky5, pn_stats
import pn_ref


def _stats(dim, seed=0, device=None):
    st = pn_ref.synthetic_stats(dim, seed)
    return st, PNStats(st['mean'], st['components'], st['variance'], n=0, seed=seed, floor=0.0, device=device)


def test_engine_option_checks():
    assert WPlusInverter(None).pn_reg == 0.0 and WPlusInverter(None, pn_reg=2).pn_reg == 2.0
    assert WPlusInverter(None, pn_reg=1e-3, latent_space='w').pn_reg == 1e-3
    for bad in (-1.0, float('nan'), float('inf'), 'x', None):
        with pytest.raises(ValueError, match='pn_reg'):
            WPlusInverter(None, pn_reg=bad)
    # the latents do not move in StyleSpace: the message names both options
    with pytest.raises(ValueError, match=r"pn_reg.*latent_space 's'"):
        WPlusInverter(None, pn_reg=0.1, latent_space='s')
    assert WPlusInverter(None, pn_reg=0.0, latent_space='s').pn_reg == 0.0
    # the statistics, where the loop is about to run: required, of the right kind, width, dtype and device
    _, st = _stats(8)
    assert check_pn(0.5, 'w+', st, 8, torch.device('cpu'), need_stats=True) == 0.5
    assert check_pn(0.0, 'w+', None, 8, torch.device('cpu'), need_stats=True) == 0.0           # off: not looked at
    assert check_pn(0.0, 'w+', 'anything', 8, torch.device('cpu'), need_stats=True) == 0.0
    with pytest.raises(ValueError, match='pn_reg > 0 needs pn_stats'):
        check_pn(0.5, 'w+', None, 8, need_stats=True)
    with pytest.raises(ValueError, match='pn_stats must be an oodgan.pn.PNStats'):
        check_pn(0.5, 'w+', dict(mean=st.mean), 8, need_stats=True)
    with pytest.raises(ValueError, match=r'pn_stats must hold a \(16,\) mean'):
        check_pn(0.5, 'w+', st, 16, need_stats=True)
    with pytest.raises(ValueError, match='pn_stats must be on meta'):
        check_pn(0.5, 'w+', st, 8, torch.device('meta'), need_stats=True)
    wrong = PNStats(st.mean64, st.components, st.variance, 0, 0, 0.0)
    wrong.matrix = wrong.matrix.double()
    with pytest.raises(ValueError, match='pn_stats must hold float32'):
        check_pn(0.5, 'w+', wrong, 8, need_stats=True)
    with pytest.raises(ValueError, match='inversion.pn_reg'):
        check_pn(-1, prefix='inversion.')


def test_option_tuple_and_cli_block():
    assert check_pn_options(0.0) == (0.0, 100000, 0, 0.0)
    assert cli.pn_options({}) == dict(pn_reg=0.0, pn_samples=100000, pn_seed=0, pn_floor=0.0)
    assert cli.pn_options({'pn_reg': 1e-3, 'pn_samples': 4096, 'pn_seed': 3, 'pn_floor': 1e-4, 'latent_space': 'w'}) == dict(
        pn_reg=1e-3, pn_samples=4096, pn_seed=3, pn_floor=1e-4)
    for block, name in (({'pn_reg': -1}, 'inversion.pn_reg'), ({'pn_reg': float('nan')}, 'inversion.pn_reg'), ({'pn_reg': 'big'}, 'inversion.pn_reg'),
                        ({'pn_samples': 1}, 'inversion.pn_samples'), ({'pn_samples': 4096.0}, 'inversion.pn_samples'),
                        ({'pn_samples': True}, 'inversion.pn_samples'), ({'pn_seed': -1}, 'inversion.pn_seed'),
                        ({'pn_seed': 1.5}, 'inversion.pn_seed'), ({'pn_floor': -1e-4}, 'inversion.pn_floor'),
                        ({'pn_floor': float('inf')}, 'inversion.pn_floor'), ({'pn_reg': 0.1, 'latent_space': 's'}, 'inversion.latent_space')):
        with pytest.raises(ValueError, match=name):
            cli.pn_options(block)
        with pytest.raises(ValueError, match=name):         # ``run`` checks the block before it asks for a GPU or builds the model
            cli.run({'name': 'x', 'datasets': {}, 'inversion': block})
    assert 'pn_reg' in cli.__doc__ and 'pn_samples' in cli.__doc__ and 'pn_floor' in cli.__doc__


def test_yardstick_on_a_case_worked_by_hand():
    """D = 3, C a permutation, sigma^2 = (1, 4, 1/4) in C's order, mu = (1, -1, 0); w = (3, -0.4, 0.5): x = l5(w) = (3, -2, 0.5), q = (2, -1, 0.5),
    and with column k of C the unit vector of axis (1, 2, 0)[k] the whitened squares are (-1)^2/1 + 0.5^2/4 + 2^2/(1/4) = 17.0625: pn = 5.6875.
    Gradient: 2/3 * l5'(w) * q / sigma^2 per axis = 2/3 * (1 * 2 * 4, 5 * -1 / 1, 1 * 0.5 / 4)."""
    comp = torch.zeros(3, 3, dtype=torch.float64)
    comp[1, 0] = comp[2, 1] = comp[0, 2] = 1.0
    var = torch.tensor([1.0, 4.0, 0.25], dtype=torch.float64)
    st = dict(mean=torch.tensor([1.0, -1.0, 0.0], dtype=torch.float64), components=comp, variance=var, matrix=(comp / var) @ comp.T)
    w = torch.tensor([[[3.0, -0.4, 0.5]]], dtype=torch.float64, requires_grad=True)
    pn = pn_ref.term(w, st)
    assert abs(pn.item() - 5.6875) <= 1e-14
    pn.sum().backward()
    want = torch.tensor([16.0 / 3.0, -10.0 / 3.0, 1.0 / 12.0], dtype=torch.float64)
    assert (w.grad[0, 0] - want).abs().max().item() <= 1e-14
    # the quadratic form the kernel evaluates is the same number
    assert abs(pn_ref.term_matrix(w.detach(), st['mean'], st['matrix']).item() - 5.6875) <= 1e-14
    assert abs(PNStats(st['mean'], comp, var, 0, 0, 0.0).distance(w.detach()).item() - 5.6875) <= 1e-14


def test_slope_at_zero_is_five():
    """l5'(0) = 5, torch's leaky_relu backward, for +0.0 and -0.0; the package's l5 agrees with the yardstick's everywhere."""
    w = torch.tensor([0.0, -0.0, 1.0, -1.0], dtype=torch.float64, requires_grad=True)
    pn_ref.leaky5(w).sum().backward()
    assert w.grad.tolist() == [5.0, 5.0, 1.0, 5.0]
    x = torch.tensor([0.0, -0.0, 2.0, -2.0, 1e-30, -1e-30])
    assert torch.equal(leaky5(x), pn_ref.leaky5(x))
    # through the term: at w = 0 the gradient carries the factor 5
    st = pn_ref.synthetic_stats(4, 1)
    w = torch.zeros(1, 1, 4, dtype=torch.float64, requires_grad=True)
    pn_ref.term(w, st).sum().backward()
    want = 5.0 * (2.0 / 4.0) * (st['matrix'] @ (-st['mean']))
    assert (w.grad[0, 0] - want).abs().max().item() <= 1e-12 * want.abs().max().item()


@pytest.mark.parametrize('shape', [(2, 18, 64), (3, 1, 37), (2, 37)])
def test_distance_is_the_yardsticks_term(shape):
    D = shape[-1]
    ref, st = _stats(D, seed=5)
    w = pn_ref.sample(ref, shape, seed=6)
    want = pn_ref.term(w.double(), ref)
    got = st.distance(w)
    assert got.dtype == torch.float64 and got.shape == (shape[0],)
    assert ((got - want).abs() / want).max().item() <= 1e-12
    # the float32 matrix is the float64 one rounded once, symmetric to the bit
    assert torch.equal(st.matrix, st.matrix.T) and st.matrix.dtype == torch.float32 and st.mean.dtype == torch.float32
    assert (st.matrix.double() - ref['matrix']).abs().max().item() <= 2.0 ** -24 * ref['matrix'].abs().max().item()
    assert st.to('cpu') is st
    with pytest.raises(ValueError, match='distance'):
        st.distance(w[..., :-1])


class _Mapping(torch.nn.Module):
    """A plain-torch stand-in for the mapping network: pixel norm, two linear layers, LeakyReLU(0.2) last."""

    def __init__(self, dim):
        super().__init__()
        g = torch.Generator().manual_seed(11)
        self.a = torch.randn(dim, dim, generator=g) / dim ** 0.5
        self.b = torch.randn(dim, dim, generator=g) / dim ** 0.5
        self.c = 0.3 * torch.randn(dim, generator=g)

    def forward(self, z):
        z = z * torch.rsqrt((z * z).mean(1, keepdim=True) + 1e-8)
        return torch.nn.functional.leaky_relu(torch.nn.functional.leaky_relu(z @ self.a, 0.2) @ self.b + self.c, 0.2)


def test_statistics_against_the_yardstick_and_the_refusal():
    D = 24
    style = _Mapping(D)
    got = pn_stats(style, D, 'cpu', n=25000, seed=3)         # three chunks, the last one short
    ref = pn_ref.stats(style, D, 25000, seed=3)
    assert (got.n, got.seed, got.floor, got.dim) == (25000, 3, 0.0, D)
    assert (got.mean64 - ref['mean']).abs().max().item() <= 1e-12
    w = pn_ref.sample(ref, (4, 3, D), seed=8)
    want = pn_ref.term(w.double(), ref)
    assert ((got.distance(w) - want).abs() / want).max().item() <= 1e-9           # the quadratic form, never the eigenvectors
    assert (got.matrix.double() - ref['matrix']).abs().max().item() <= 1e-6 * ref['matrix'].abs().max().item()
    # the floor: variances below floor * max are raised to it
    fl = pn_stats(style, D, 'cpu', n=25000, seed=3, floor=0.05)
    assert fl.floor == 0.05 and abs(fl.variance.min().item() - 0.05 * fl.variance.max().item()) <= 1e-15
    assert (fl.variance >= got.variance - 1e-15).all() and (fl.variance > got.variance).any()
    # another seed: other statistics
    assert not torch.equal(pn_stats(style, D, 'cpu', n=25000, seed=4).mean64, got.mean64)
    # n <= D without a floor: the covariance has no full rank, the message names both options
    for n in (D, D // 2, 2):
        with pytest.raises(ValueError, match=r'pn_samples.*pn_floor'):
            pn_stats(style, D, 'cpu', n=n, seed=0, floor=0.0)
        with pytest.raises(ValueError, match=r'pn_samples.*pn_floor'):
            pn_ref.stats(style, D, n, seed=0, floor=0.0)
    assert pn_stats(style, D, 'cpu', n=D, seed=0, floor=1e-3).variance.min().item() > 0         # a floor makes them usable
    with pytest.raises(ValueError, match='pn_samples'):
        pn_stats(style, D, 'cpu', n=1)
    with pytest.raises(ValueError, match='pn_floor'):
        pn_stats(style, D, 'cpu', n=100, floor=-1.0)
