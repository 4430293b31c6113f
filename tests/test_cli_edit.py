"""``inversion.edit`` of the CLI: where a data set's editing direction goes when the W+ loop runs.  The model, the checkpoint
and the files of tests/test_cli.py::test_cli_end_to_end, one file per data set; the generator's noise maps are preset so that two runs of the
tool are comparable byte for byte."""
import os

import numpy as np
import pytest
import torch
import yaml

from oodgan import synth

pytestmark = pytest.mark.gpu


def _options(tmp, save, edit=None, editing=True):
    inv = {} if edit is None else {'edit': edit}
    sets = {'val_0': {'dataroot': str(tmp / 'data'), 'editing': {'direction': 'Smiling', 'intensity': 2}}} if editing else {}
    if edit == 'final' or not editing:
        sets['val_1'] = {'dataroot': str(tmp / 'data')}              # no ``editing`` block
    return {
        'name': 'OOD_faceGAN_e4e', 'save_dir': str(tmp / save), 'directions_dir': str(tmp / 'directions'), 'datasets': sets,
        'network_g': {'type': 'ood_faceGAN_e4e', 'out_size': 1024, 'style_dim': 512, 'encoder': 'E4E', 'enable_modulation': True,
                      'warp_scale': 0.08, 'cycle_align': 2, 'blend_with_gen': True, 'ModSize': 256},
        'path': {'pretrain_network_g': str(tmp / 'net_g.pth'), 'param_key_g': 'params_ema', 'strict_load_g': False},
        'metrics': {'psnr': {'crop_border': 2, 'test_y_channel': False}},
        'inversion': inv,
    }


def _bytes(tmp, save, name, kind):
    with open(tmp / save / 'OOD_faceGAN_e4e' / name / kind / '00001.png', 'rb') as f:
        return f.read()


def test_cli_edit_final_and_start(tmp_path, monkeypatch):
    from oodgan import cli, imgio, modules
    from oodgan.arch import ood_faceGAN_e4e
    opts = _options(tmp_path, 'r')
    m = ood_faceGAN_e4e(**{k: v for k, v in opts['network_g'].items() if k != 'type'})
    sd = synth.ood_state(1024, seed=31)
    enc = synth.encoder_state({k: tuple(v.shape) for k, v in m.encoder.state_dict().items()}, seed=41)
    sd.update({'encoder.' + k: (v * 0.1 if k.endswith('linear.weight') else v) for k, v in enc.items()})
    torch.save({'params_ema': sd}, tmp_path / 'net_g.pth')
    del m
    os.makedirs(tmp_path / 'directions')
    np.save(tmp_path / 'directions' / 'Smiling.npy', (0.05 * np.random.default_rng(0).standard_normal((18, 512))).astype(np.float32))
    os.makedirs(tmp_path / 'data')
    imgio.imwrite(str(tmp_path / 'data' / '00001.png'), np.random.default_rng(1).integers(0, 256, (256, 256, 3), dtype=np.uint8))
    # without ``noise=`` ``invert`` draws fresh noise maps per call (Generator.make_noise): preset them, so that two runs are comparable
    presets = synth.make_noises(1024, 1, seed=35)
    monkeypatch.setattr(modules.Generator, 'make_noise', lambda self: [n.to(self.input.input.device) for n in presets])
    # a wrapper around model.invert: the refined latents, the edit it was handed and delta_latent while it ran
    models, calls = [], []
    load = cli.load_model

    def load_wrapped(o):
        model = load(o)
        models.append((model, model.delta_latent.detach().cpu().clone()))       # load_model returns the model on the host
        inner = model.invert

        def invert(*a, **k):
            r = inner(*a, **k)
            calls.append(dict(refined=model.last_refined_lats.clone(), lats=r[1].clone(), edit=k.get('edit'), delta=model.delta_latent.detach().clone()))
            return r

        model.invert = invert
        return model

    monkeypatch.setattr(cli, 'load_model', load_wrapped)

    def run(save, **kw):
        with open(tmp_path / f'{save}.yml', 'w') as f:
            yaml.safe_dump(_options(tmp_path, save, **kw), f)
        del calls[:]
        summary = cli.main(['--opt', str(tmp_path / f'{save}.yml'), '--wplus-steps', '2'])
        return summary, list(calls)

    direction = 2 * torch.from_numpy(np.load(tmp_path / 'directions' / 'Smiling.npy'))[None]
    # edit: final — val_0 with the direction, val_1 (the same file) without an ``editing`` block
    s_final, c_final = run('final', edit='final')
    model, delta0 = models[-1]
    assert set(s_final) == {'val_0', 'val_1'} and len(c_final) == 2 and np.isfinite(s_final['val_0']['psnr'])
    assert imgio.imread(str(tmp_path / 'final' / 'OOD_faceGAN_e4e' / 'val_0' / 'inversion' / '00001.png')).shape == (1024, 1024, 3)
    assert torch.equal(model.delta_latent.detach().cpu(), delta0) and not delta0.any()
    edited, plain = c_final
    assert torch.equal(edited['delta'].cpu(), delta0) and torch.equal(edited['edit'].cpu(), direction) and plain['edit'] is None
    # the loop never saw the direction: the refined latents of a data set without one; the output was generated from refined + direction
    assert torch.equal(edited['refined'], plain['refined'])
    assert torch.equal(edited['lats'], edited['refined'] + edited['edit']) and torch.equal(plain['lats'], plain['refined'])
    assert _bytes(tmp_path, 'final', 'val_0', 'inversion') != _bytes(tmp_path, 'final', 'val_1', 'inversion')
    # the same against a run of its own whose only data set has no ``editing`` block
    _, c_plain = run('plain', editing=False)
    assert len(c_plain) == 1 and c_plain[0]['edit'] is None and torch.equal(c_plain[0]['refined'], edited['refined'])
    assert _bytes(tmp_path, 'plain', 'val_1', 'inversion') == _bytes(tmp_path, 'final', 'val_1', 'inversion')
    # edit: start — today's behaviour: the direction is in delta_latent while the loop runs, nothing is handed to invert
    s_start, c_start = run('start', edit='start')
    assert len(c_start) == 1 and c_start[0]['edit'] is None and torch.equal(c_start[0]['delta'].cpu(), delta0 + direction)
    assert not torch.equal(c_start[0]['refined'], edited['refined'])
    assert _bytes(tmp_path, 'start', 'val_0', 'inversion') != _bytes(tmp_path, 'final', 'val_0', 'inversion')
    # ... and byte-identical to a run without the key
    s_none, c_none = run('nokey')
    assert len(c_none) == 1 and torch.equal(c_none[0]['refined'], c_start[0]['refined'])
    for kind in ('inversion', 'masks'):
        assert _bytes(tmp_path, 'nokey', 'val_0', kind) == _bytes(tmp_path, 'start', 'val_0', kind), kind
    assert s_none['val_0']['psnr'] == s_start['val_0']['psnr']
