"""``inversion.loss_region: fit`` and its keys in the CLI: checked before the GPU is touched, handed to ``model.invert``.  The
end-to-end case runs the tool's loop on the 64² model of tests/test_hip_wplus_sched.py (no encoder, no modulation blocks: the latents are
handed in), two files in one chunk."""
import os

import numpy as np
import pytest
import torch

from oodgan import synth

KEYS = ('loss_region', 'mask_size', 'mask_lr', 'mask_area', 'mask_area_weight', 'mask_binary_weight', 'mask_init', 'fit_blend')


def test_keys_are_checked_before_the_gpu():
    from oodgan import cli
    assert cli.mask_fit_options({}) == {} and cli.mask_fit_options({'loss_region': 'blend'}) == {}
    assert cli.mask_fit_options({'loss_region': 'fit'}) == dict(mask_size=64, mask_lr=0.1, mask_area=0.30, mask_area_weight=5.0,
                                                                  mask_binary_weight=0.2, mask_init=0.88, fit_blend=False)
    got = cli.mask_fit_options({'loss_region': 'fit', 'mask_size': 16, 'mask_init': 'blend', 'fit_blend': True, 'mask_lr': 0.05}, 64)
    assert (got['mask_size'], got['mask_init'], got['fit_blend'], got['mask_lr']) == (16, 'blend', True, 0.05)
    fit = {'loss_region': 'fit'}
    for block, name in (({**fit, 'mask_size': 48}, 'inversion.mask_size'), ({**fit, 'mask_size': '64'}, 'inversion.mask_size'),
                        ({**fit, 'mask_lr': 0}, 'inversion.mask_lr'), ({**fit, 'mask_lr': float('nan')}, 'inversion.mask_lr'),
                        ({**fit, 'mask_area': 1.2}, 'inversion.mask_area'), ({**fit, 'mask_area_weight': -1}, 'inversion.mask_area_weight'),
                        ({**fit, 'mask_binary_weight': float('inf')}, 'inversion.mask_binary_weight'),
                        ({**fit, 'mask_init': 1.0}, 'inversion.mask_init'), ({**fit, 'mask_init': 'full'}, 'inversion.mask_init'),
                        ({**fit, 'fit_blend': 'yes'}, 'inversion.fit_blend'), ({**fit, 'mask_dir': '/masks'}, 'inversion.mask_dir'),
                        ({'mask_size': 64}, 'inversion.mask_size'), ({'loss_region': 'blend', 'fit_blend': True}, 'inversion.fit_blend'),
                        ({'loss_region': 'fitted'}, 'inversion.loss_region')):
        with pytest.raises(ValueError, match=name):
            cli.run({'name': 'x', 'datasets': {}, 'inversion': block})
    with pytest.raises(ValueError, match='inversion.mask_size'):          # against the configured generator size
        cli.run({'name': 'x', 'datasets': {}, 'network_g': {'out_size': 64}, 'inversion': {**fit, 'mask_size': 64}})
    for block, name in (({**fit, 'pixel_size': 32}, 'pixel_size'), ({**fit, 'latent_space': 's'}, 'latent_space'),
                        ({**fit, 'feature_layer': 5}, 'feature_layer'), ({**fit, 'pixel_target': 'file'}, 'pixel_target')):
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
    block = {'wplus_steps': 4, 'batch': 2, 'loss_region': 'fit', 'mask_size': 16, 'mask_lr': 0.05, 'mask_area': 0.2, 'mask_area_weight': 3.0,
             'mask_binary_weight': 0.1, 'mask_init': 0.7, 'fit_blend': True}
    opts = {'name': 'fit', 'save_dir': str(tmp_path / 'out'), 'datasets': {'val': {'dataroot': str(tmp_path / 'data')}},
            'network_g': {'type': 'ood_faceGAN_e4e', 'out_size': size}, 'metrics': {'psnr': {'crop_border': 0, 'test_y_channel': False}},
            'inversion': block}
    summary = cli.run(opts)
    model, call = calls
    assert call == {k: block[k] for k in KEYS}
    a, beta, t = model.last_fitted_mask, model.last_loss_weight, model.last_loss_terms
    assert a.shape == (2, 1, 16, 16) and beta.shape == (2, 1, size, size) and t['mask_area'].shape == (4, 2)
    assert abs(t['mask_area'][0, 0].item() - 0.1) < 1e-6 and abs(t['mask_binary'][0, 0].item() - 0.3) < 1e-6        # a = 0.7: 1 - 0.7 - 0.2; min = 0.3
    assert np.isfinite(summary['val']['psnr']) and os.path.isfile(tmp_path / 'out' / 'fit' / 'val' / 'inversion' / files[0])
    # a bad value fails loudly, before the model is built
    del calls[:]
    opts['inversion'] = {**block, 'mask_size': 20}
    with pytest.raises(ValueError, match='inversion.mask_size'):
        cli.run(opts)
    assert not calls
    # without the keys the loop runs without the mask
    opts['inversion'] = {'wplus_steps': 3, 'batch': 2}
    cli.run(opts)
    assert calls[0].last_fitted_mask is None and calls[1]['loss_region'] == 'full' and calls[1]['mask_size'] is None
