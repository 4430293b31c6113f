"""The host side of the CLI's ``inversion.io`` pipeline, without a GPU: the 256-entry input table, the checks of the two
options, and the writer pool (order, bound on in-flight writes, a worker's exception, no thread left behind)."""
import threading

import numpy as np
import pytest
import torch

from oodgan import imgio


def test_u8_table_is_the_host_expression_on_all_256_values():
    table = imgio.u8_input_table()
    assert table.shape == (256,) and table.dtype == torch.float32
    bgr = np.arange(256 * 3, dtype=np.int64).reshape(16, 16, 3) % 256          # every byte value in every channel
    assert set(bgr[:, :, 0].ravel()) == set(range(256))
    host = imgio.image_to_input(bgr.astype(np.float64), 16)                      # (1,3,16,16) RGB
    want = torch.from_numpy(bgr[:, :, ::-1].copy()).permute(2, 0, 1).unsqueeze(0)
    assert torch.equal(table[want], host)
    # and the way back: the uint8 of the table is the byte (the CLI's ground truth of a resized file is tensor2img of such values)
    back = imgio.tensor2img(table.reshape(1, 1, 16, 16), min_max=(-1, 1))
    assert np.array_equal(back.ravel(), np.arange(256))


@pytest.mark.parametrize('bad', [{'io': 'gpu'}, {'io_workers': 0}, {'io_workers': 17}, {'io_workers': 2.5}, {'io_workers': True}])
def test_bad_io_options_raise_before_the_gpu_check(bad):
    from oodgan import cli
    with pytest.raises(ValueError, match='inversion.io'):
        cli.run({'name': 'x', 'datasets': {}, 'inversion': bad})
    assert cli.io_options({}) == ('device', 4) and cli.io_options({'io': 'host', 'io_workers': 16}) == ('host', 16)


def _io_threads():
    return [t for t in threading.enumerate() if t.name.startswith('oodgan-io')]


def _write(path, arr, tag):
    imgio.imwrite(path, arr)
    return tag


def test_writer_pool_keeps_order_and_bounds_in_flight_writes(tmp_path):
    from oodgan import cli
    rng = np.random.default_rng(0)
    # sizes vary, so the workers finish out of order
    imgs = [rng.integers(0, 256, (8 + 37 * (i % 5), 16 + 11 * (i % 3), 3), dtype=np.uint8) for i in range(23)]
    workers = 2
    with cli.WriterPool(workers) as pool:
        for i, a in enumerate(imgs):
            pool.submit(_write, str(tmp_path / 'out' / f'{i:03d}.png'), a, i)
            assert len(pool._pending) <= 2 * workers
        assert pool.max_pending == 2 * workers
        assert pool.drain() == list(range(len(imgs)))
        assert pool.drain() == []
        assert len(_io_threads()) <= workers
    assert not _io_threads()
    for i, a in enumerate(imgs):
        assert np.array_equal(imgio.imread(str(tmp_path / 'out' / f'{i:03d}.png')), a)


def test_writer_pool_raises_a_workers_exception_and_leaves_nothing_running(tmp_path):
    from oodgan import cli
    (tmp_path / 'blocker').write_bytes(b'a file where a directory is needed')
    img = np.zeros((4, 4, 3), np.uint8)
    with pytest.raises(OSError):
        with cli.WriterPool(2) as pool:
            pool.submit(_write, str(tmp_path / 'ok' / 'a.png'), img, 0)
            pool.submit(_write, str(tmp_path / 'blocker' / 'sub' / 'b.png'), img, 1)
            pool.submit(_write, str(tmp_path / 'ok' / 'c.png'), img, 2)
            pool.drain()
    assert not _io_threads()
    # the failure also surfaces from a later submit that has to make room, not only from drain
    with pytest.raises(OSError):
        with cli.WriterPool(1) as pool:
            pool.submit(_write, str(tmp_path / 'blocker' / 'sub' / 'b.png'), img, 0)
            for i in range(3):
                pool.submit(_write, str(tmp_path / 'ok' / f'd{i}.png'), img, i)
    assert not _io_threads()
