"""``inversion.align`` and its keys in the CLI: checked before the GPU is touched, handed to ``model.invert``.  The end-to-end
case runs the tool's loop on the 64² model of tests/test_hip_wplus_sched.py (no encoder, no modulation blocks: the latents are handed in),
two files in one chunk."""
import os

import numpy as np
import pytest
import torch

from oodgan import synth

KEYS = ('align', 'align_lr', 'align_reg')


def test_keys_are_checked_before_the_gpu():
    from oodgan import cli
    assert cli.align_options({}) == {} and cli.align_options({'loss_region': 'blend'}) == {}
    assert cli.align_options({'align': 'similarity'}) == dict(align='similarity', align_lr=0.001, align_reg=0.0)
    assert cli.align_options({'align': 'similarity', 'align_lr': 0.002, 'align_reg': 0.5, 'pixel_size': 32, 'pixel_loss': 'huber',
                              'latent_space': 'w'}) == dict(align='similarity', align_lr=0.002, align_reg=0.5)
    on = {'align': 'similarity'}
    for block, name in (({'align': 'affine'}, 'inversion.align'), ({'align': True}, 'inversion.align'), ({**on, 'align_lr': -1}, 'inversion.align_lr'),
                        ({**on, 'align_lr': float('nan')}, 'inversion.align_lr'), ({**on, 'align_lr': '0.1'}, 'inversion.align_lr'),
                        ({**on, 'align_reg': -0.5}, 'inversion.align_reg'), ({**on, 'align_reg': float('inf')}, 'inversion.align_reg'),
                        ({'align_lr': 0.01}, 'inversion.align_lr'), ({'align_reg': 0.1}, 'inversion.align_reg')):
        with pytest.raises(ValueError, match=name):
            cli.run({'name': 'x', 'datasets': {}, 'inversion': block})
    for block, name in (({**on, 'ssim_weight': 0.5}, 'SSIM'), ({**on, 'lpips_weight': 0.8}, 'LPIPS'), ({**on, 'loss_region': 'blend'}, 'loss_region'),
                        ({**on, 'mask_dir': '/masks'}, 'loss_region'), ({**on, 'pixel_size': 32, 'pixel_filter': 'bicubic'}, 'pixel_filter'),
                        ({**on, 'pixel_target': 'file'}, 'pixel_target'), ({**on, 'latent_space': 's'}, 'latent_space'),
                        ({**on, 'feature_layer': 5}, 'feature_layer')):
        with pytest.raises(NotImplementedError, match=name):
            cli.run({'name': 'x', 'datasets': {}, 'inversion': block})


@pytest.mark.gpu
def test_cli_keys_reach_the_loop(tmp_path, monkeypatch):
    import test_hip_wplus_sched as S
    from oodgan import cli, imgio
    size, files = 64, ('00001.png', '00002.png')
    os.makedirs(tmp_path / 'data')
    for k, f in enumerate(files):
        imgio.imwrite(str(tmp_path / 'data' / f), np.random.default_rng(k).integers(0, 256, (size, size, 3), dtype=np.uint8))
    enc = synth.make_latents(size, len(files), seed=42, std=0.3)
    noise = synth.make_noises(size, len(files), seed=45)
    calls = []

    def load(opts):
        m = S._model_64('cpu')
        inner = m.invert

        def invert(x, **k):
            calls.append({n: k.get(n) for n in KEYS})
            return inner(x, enc_lats=enc.to(x.device), noise=[n.to(x.device) for n in noise], **k)

        m.invert = invert
        calls.append(m)
        return m

    monkeypatch.setattr(cli, 'load_model', load)
    block = {'wplus_steps': 4, 'batch': 2, 'align': 'similarity', 'align_lr': 0.002, 'align_reg': 0.25}
    opts = {'name': 'al', 'save_dir': str(tmp_path / 'out'), 'datasets': {'val': {'dataroot': str(tmp_path / 'data')}},
            'network_g': {'type': 'ood_faceGAN_e4e', 'out_size': size}, 'metrics': {'psnr': {'crop_border': 0, 'test_y_channel': False}},
            'inversion': block}
    summary = cli.run(opts)
    model, call = calls
    assert call == {k: block[k] for k in KEYS}
    th, t = model.last_alignment, model.last_loss_terms
    assert th.shape == (2, 4) and (th != 0).all() and (th.abs() <= 4 * 0.002 * 3.2).all() and t['align'].shape == (4, 2)
    assert (t['align'][0] == 0).all() and (t['align'][1:] > 0).all()           # sum theta^2 before each step, from the identity
    assert model.last_aligned_input.shape == (2, 3, size, size)
    assert np.isfinite(summary['val']['psnr']) and os.path.isfile(tmp_path / 'out' / 'al' / 'val' / 'inversion' / files[0])
    # a bad value fails loudly, before the model is built
    del calls[:]
    opts['inversion'] = {**block, 'align': 'rigid'}
    with pytest.raises(ValueError, match='inversion.align'):
        cli.run(opts)
    assert not calls
    # without the keys the loop runs without the alignment
    opts['inversion'] = {'wplus_steps': 3, 'batch': 2}
    cli.run(opts)
    assert calls[0].last_alignment is None and calls[1]['align'] is None
