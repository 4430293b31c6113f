"""``inversion.pixel_filter`` / ``inversion.pixel_target: file`` of the CLI, end to end: the tool's loop on the 64² model of
tests/test_hip_wplus_sched.py (no encoder, no modulation blocks: the latents are handed in), two 16² files in one chunk.  The files' own pixels
reach ``model.invert`` as the pixel target, unresized, while the bilinearly enlarged image stays the model's input."""
import os

import numpy as np
import pytest
import torch

from oodgan import synth

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('io', ['host', 'device'])
def test_files_supply_their_own_pixels(tmp_path, monkeypatch, io):
    import test_hip_wplus_sched as S
    from oodgan import _lib, cli, imgio
    size, n, files = 64, 16, ('00001.png', '00002.png')
    os.makedirs(tmp_path / 'data')
    pixels = [np.random.default_rng(k).integers(0, 256, (n, n, 3), dtype=np.uint8) for k in range(len(files))]
    for f, px in zip(files, pixels):
        imgio.imwrite(str(tmp_path / 'data' / f), px)
    enc = synth.make_latents(size, len(files), seed=42, std=0.3)
    noise = synth.make_noises(size, len(files), seed=45)
    calls = []

    def load(opts):
        m = S._model_64('cpu')
        inner = m.invert

        def invert(x, **k):
            calls.append((x, {name: k.get(name) for name in ('pixel_size', 'pixel_filter', 'pixel_target')}))
            return inner(x, enc_lats=enc.to(x.device), noise=[t.to(x.device) for t in noise], **k)

        m.invert = invert
        return m

    monkeypatch.setattr(cli, 'load_model', load)
    opts = {'name': 'rs', 'save_dir': str(tmp_path / 'out'), 'datasets': {'val': {'dataroot': str(tmp_path / 'data')}},
            'network_g': {'type': 'ood_faceGAN_e4e', 'out_size': size}, 'metrics': {'psnr': {'crop_border': 0, 'test_y_channel': False}},
            'inversion': {'wplus_steps': 3, 'batch': 2, 'io': io, 'pixel_filter': 'bicubic', 'pixel_target': 'file'}}
    _lib.dispatch_reset()
    summary = cli.run(opts)
    (x, kw), = calls
    assert tuple(x.shape) == (2, 3, size, size) and kw['pixel_filter'] == 'bicubic' and kw['pixel_size'] is None
    want = torch.cat([imgio.image_to_input(imgio.imread(str(tmp_path / 'data' / f)).astype(np.float64), n, device='cuda') for f in files], 0)
    assert tuple(kw['pixel_target'].shape) == (2, 3, n, n) and torch.equal(kw['pixel_target'], want)
    assert _lib.dispatch_count('resampled_pixel') >= 1 and _lib.dispatch_count('pooled_pixel') == 0
    assert np.isfinite(summary['val']['psnr']) and os.path.isfile(tmp_path / 'out' / 'rs' / 'val' / 'inversion' / files[0])
    # a stated pixel_size has to be the files' size; the box takes the files' pixels too
    opts['inversion'].update(pixel_size=32)
    with pytest.raises(ValueError, match='pixel_size'):
        cli.run(opts)
    del calls[:]
    opts['inversion'].update(pixel_size=n, pixel_filter='box')
    _lib.dispatch_reset()
    cli.run(opts)
    assert calls[0][1]['pixel_filter'] is None and torch.equal(calls[0][1]['pixel_target'], want)
    assert _lib.dispatch_count('pooled_pixel') >= 1 and _lib.dispatch_count('resampled_pixel') == 0
