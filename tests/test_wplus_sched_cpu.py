"""CPU checks of the projector schedule's host side: the float64 restatement of the latent noise that the GPU tests compare the
kernel with (tests/latent_noise_ref.py) against Philox's known answers, the learning-rate multiplier, and the argument checks of the CLI and
of ``WPlusInverter``."""
import math

import numpy as np
import pytest

import latent_noise_ref as N


@pytest.mark.parametrize('counter,key,want', [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
])
def test_philox_known_answers(counter, key, want):
    got = tuple(int(x) for x in N.philox4x32_10(counter, key))
    assert got == want, [hex(x) for x in got]


def test_philox_vectorised_equals_one_by_one():
    q = np.arange(5, dtype=np.uint64)
    many = N.philox4x32_10((q, 7, 3, 2), (11, 13))
    for j in range(5):
        assert tuple(int(x[j]) for x in many) == tuple(int(x) for x in N.philox4x32_10((j, 7, 3, 2), (11, 13)))


def test_uniforms_are_open_and_exact():
    u = N.uniforms([np.array([0, 0xFFFFFFFF, 0x100], dtype=np.uint64)])[0]
    assert u[0] == 2.0 ** -25 and u[1] == 1.0 - 2.0 ** -25 and u[2] == 1.5 * 2.0 ** -24


def test_noise_sanity():
    n = 9216
    a = N.unit_normals(0, 0, 0, n)
    print(f'(seed 0, id 0, step 0), {n} values: mean {a.mean():.2e}, std {a.std():.4f}, max |n| {np.abs(a).max():.2f}')
    assert a.shape == (n,) and abs(a.mean()) < 0.05 and abs(a.std() - 1.0) < 0.05
    for name, other in (('id 1', N.unit_normals(0, 1, 0, n)), ('step 1', N.unit_normals(0, 0, 1, n)), ('seed 1', N.unit_normals(1, 0, 0, n)),
                        ('id 2^32', N.unit_normals(0, 2 ** 32, 0, n))):
        c = np.corrcoef(a, other)[0, 1]
        print(f'correlation with ({name}): {c:.4f}')
        assert abs(c) < 0.05
    # a tail that is no multiple of 4 is a prefix of the longer draw; |n| <= sqrt(-2 ln 2^-25) by construction
    assert np.array_equal(N.unit_normals(0, 0, 0, 37), a[:37])
    assert np.abs(a).max() <= math.sqrt(50.0 * math.log(2.0))


def test_sigma_schedule():
    assert N.sigma(0, 100, 0.05, 0.75) == 0.05
    assert N.sigma(30, 100, 0.05, 0.75) == pytest.approx(0.05 * 0.6 ** 2, rel=1e-12)
    assert N.sigma(75, 100, 0.05, 0.75) == 0.0 and N.sigma(99, 100, 0.05, 0.75) == 0.0
    assert N.sigma(99, 100, 0.05, 0.0) == 0.05
    z = N.latent_noise(0, [3, 4], 80, 16, 100, 0.05, 0.75)
    assert z.shape == (2, 16) and not z.any()


def test_lr_multiplier():
    from oodgan.ops import lr_multiplier
    want = {0: 0.0, 1: 0.2, 4: 0.8, 5: 1.0, 50: 1.0, 75: 1.0, 90: 0.3455, 99: 0.0039}
    for i, r in want.items():
        assert lr_multiplier(i, 100, 0.05, 0.25) == pytest.approx(r, abs=5e-5), i
    for i in range(100):            # the formula
        tau = i / 100
        r = min(1.0, (1.0 - tau) / 0.25)
        assert lr_multiplier(i, 100, 0.05, 0.25) == pytest.approx((0.5 - 0.5 * math.cos(math.pi * r)) * min(1.0, tau / 0.05), abs=1e-15)
        # a ramp at 0 switches its factor off
        assert lr_multiplier(i, 100, 0.0, 0.0) == 1.0
        assert lr_multiplier(i, 100, 0.05, 0.0) == pytest.approx(min(1.0, tau / 0.05), abs=1e-15)
        assert lr_multiplier(i, 100, 0.0, 0.25) == pytest.approx(0.5 - 0.5 * math.cos(math.pi * r), abs=1e-15)


_OPTIONS = ('lr_rampup', 'lr_rampdown', 'latent_noise', 'noise_ramp', 'noise_seed', 'latent_reg')


@pytest.mark.parametrize('bad', [-1, float('nan'), 'much'])
@pytest.mark.parametrize('name', _OPTIONS)
def test_cli_rejects_a_bad_schedule_option_before_it_asks_for_a_gpu(name, bad):
    from oodgan import cli
    with pytest.raises(ValueError, match='inversion.' + name):
        cli.run({'name': 'x', 'datasets': {}, 'network_g': {'type': 'ood_faceGAN_e4e'}, 'inversion': {name: bad}})


def test_cli_rejects_an_unknown_latent_anchor():
    from oodgan import cli
    with pytest.raises(ValueError, match='latent_anchor'):
        cli.run({'name': 'x', 'datasets': {}, 'network_g': {'type': 'ood_faceGAN_e4e'}, 'inversion': {'latent_anchor': 'median'}})
    kw = cli.schedule_options({'lr_rampup': 0.05, 'latent_noise': 0.05, 'noise_seed': 3, 'latent_anchor': 'mean'})
    assert kw == dict(lr_rampup=0.05, lr_rampdown=0.0, latent_noise=0.05, noise_ramp=0.75, latent_reg=0.0, noise_seed=3, latent_anchor='mean')


def test_inverter_rejects_bad_schedule_arguments():
    from oodgan.engine import WPlusInverter
    for name in _OPTIONS:
        for bad in (-1, float('nan'), 'much'):
            with pytest.raises(ValueError, match=name):
                WPlusInverter(None, **{name: bad})
    inv = WPlusInverter(None)
    assert (inv.lr_rampup, inv.lr_rampdown, inv.latent_noise, inv.noise_ramp, inv.noise_seed, inv.latent_reg) == (0.0, 0.0, 0.0, 0.75, 0, 0.0)
