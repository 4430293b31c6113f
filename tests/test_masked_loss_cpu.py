"""CPU checks of the masked W+ objective's host side: the CLI's per-file loss masks (``inversion.mask_dir``) and the
batch-sharding of a per-image loss weight (oodgan/parallel.py, world size 2 over gloo)."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp


def _png(path, arr):
    from PIL import Image
    Image.fromarray(arr).save(path)


def test_mask_dir_png_to_loss_weight(tmp_path):
    from oodgan import cli
    masks = tmp_path / 'masks'
    masks.mkdir()
    rng = np.random.default_rng(0)
    gray = rng.integers(0, 256, size=(5, 7), dtype=np.uint8)
    rgb = np.stack([gray, 255 - gray, np.zeros_like(gray)], -1)             # only the first channel is read
    _png(masks / 'a.png', gray)
    _png(masks / 'b.png', rgb)
    files = [str(tmp_path / 'in' / 'a.jpg'), str(tmp_path / 'in' / 'b.png')]
    beta = cli.load_loss_weights(files, str(masks), 16)
    assert beta.shape == (2, 1, 16, 16) and beta.dtype == torch.float32
    # nearest resize as F.interpolate(mode='nearest'): src = floor(dst * in / out)
    want = torch.nn.functional.interpolate(torch.from_numpy(gray).double().view(1, 1, 5, 7) / 255.0, size=(16, 16), mode='nearest')
    assert torch.allclose(beta[0:1].double(), want, atol=1e-7, rtol=0) and torch.equal(beta[0], beta[1])
    assert beta.min() >= 0 and beta.max() <= 1
    with pytest.raises(FileNotFoundError):
        cli.load_loss_weights(files + [str(tmp_path / 'in' / 'c.png')], str(masks), 16)
    for bad in (np.full((4, 4), 256.0), np.full((4, 4), -1.0), np.full((4, 4), np.nan), np.zeros((0, 3))):
        with pytest.raises(ValueError):
            cli.mask_to_weight(bad, 8)


def test_cli_rejects_conflicting_or_unknown_regions():
    from oodgan import cli
    for inv in ({'loss_region': 'masked'}, {'loss_region': 'blend', 'mask_dir': 'masks'}):
        with pytest.raises(ValueError, match='loss_region'):
            cli.run({'name': 'x', 'datasets': {}, 'network_g': {'type': 'ood_faceGAN_e4e'}, 'inversion': inv})


def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _fake_invert(target, w0, noises, loss_weight):
    # stands in for WPlusInverter.invert(..., loss_weight=): a per-image function of this rank's slice that depends on its loss weight
    assert loss_weight.shape[0] == w0.shape[0] == target.shape[0]
    return w0 + (loss_weight * target).mean(dim=(1, 2, 3)).view(-1, 1, 1) + 10.0 * loss_weight.sum(dim=(1, 2, 3)).view(-1, 1, 1)


def _worker(rank, world, port, gB, q):
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, 'ood-gan-inversion_amd'))
    import torch.distributed as dist
    from oodgan import parallel, synth
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port))
    dist.init_process_group('gloo', rank=rank, world_size=world)
    target = synth.make_images(8, gB, seed=1)
    w0 = synth.make_latents(16, gB, seed=3)
    noises = [synth.normal('n', (gB, 1, 4, 4), 2)]
    beta = torch.sigmoid(synth.normal('beta', (gB, 1, 8, 8), 4))
    beta[-1] = 0.0                                                           # the last image ignores every pixel
    full = _fake_invert(target, w0, noises, beta)
    got = parallel.invert_sharded(_fake_invert, dict(target=target, w0=w0, noises=noises, loss_weight=beta), gB, rank, world)
    sl = parallel.shard_slice(gB, rank, world)
    mine = _fake_invert(target[sl], w0[sl], [noises[0][sl]], beta[sl])
    q.put((rank, bool(got.shape == full.shape and torch.equal(got, full) and torch.equal(mine, full[sl]))))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize('gB', [4, 3])
def test_loss_weight_is_sharded_with_its_images(gB):
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, gB, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = dict(q.get(timeout=120) for _ in procs)
    for p in procs:
        p.join(timeout=60)
    assert res == {0: True, 1: True}
