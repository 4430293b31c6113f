"""The pixel terms of the W+ loss (csrc/loss_pixel.hip: one plane and one flat kernel template behind the MSE, the composite MSE and the
robust entry points) compute, bit for bit, what the three separate kernel sets of the commit before computed.

tests/golden/pixel_terms_parent.npz was recorded on the MI355X with that commit's library (tests/golden/make_pixel_terms_parent.py);
tests/pixel_terms_cases.py lists the cases: per shape the MSE, the composite MSE for both ``wrt`` with and without the composite, every
robust kind plain and with beta for both ``wrt`` and forward only, and the loss-table form of each entry point.  Asserted: equal loss
bits, equal SHA-256 of the gradient's and of the composite's raw bytes."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import pixel_terms_cases as PC  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'pixel_terms_parent.npz')


@pytest.fixture(scope='module')
def parent():
    return np.load(GOLDEN)


@pytest.mark.parametrize('name', list(PC.SHAPES))
def test_bits_of_the_parent_commit(parent, name):
    from oodgan import ops
    assert torch.cuda.is_available()
    losses, digests = PC.run(ops, PC.SHAPES[name], torch.device('cuda:0'))
    keys = [str(k) for k in parent[f'{name}/loss_keys']]
    want = dict(zip(keys, np.split(parent[f'{name}/losses'], np.cumsum(parent[f'{name}/loss_sizes'])[:-1])))
    assert sorted(losses) == sorted(want)
    bad = [k for k in keys if not np.array_equal(losses[k].view(np.uint32), want[k].view(np.uint32))]
    for k in bad:
        print(f'{name} {k}: loss {losses[k].tolist()}, parent {want[k].tolist()}')
    dkeys = [str(k) for k in parent[f'{name}/digest_keys']]
    dwant = {k: bytes(d) for k, d in zip(dkeys, parent[f'{name}/digests'])}
    assert sorted(digests) == sorted(dwant)
    dbad = [k for k in dkeys if digests[k] != dwant[k]]
    print(f'{name} {PC.SHAPES[name]}: {len(keys) - len(bad)}/{len(keys)} losses and {len(dkeys) - len(dbad)}/{len(dkeys)} digests equal the parent\'s')
    assert not bad and not dbad, (bad, dbad)
