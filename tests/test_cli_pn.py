"""``inversion.pn_reg`` / ``pn_samples`` / ``pn_seed`` / ``pn_floor`` of the CLI: checked before the GPU is touched, handed to
``model.invert``, and each file's final P_N+ distance in the summary — the last row of the loop's own table.  The end-to-end case runs the tool's
loop on the 64² model of tests/test_hip_wplus_sched.py (no encoder, no modulation blocks: the latents are handed in), two files in one chunk."""
import logging
import os

import numpy as np
import pytest
import torch

from oodgan import synth


def test_keys_are_checked_before_the_gpu():
    from oodgan import cli
    assert cli.pn_options({'pn_reg': 0.002})['pn_reg'] == 0.002
    for block, name in (({'pn_reg': -0.5}, 'inversion.pn_reg'), ({'pn_reg': 1e-3, 'pn_samples': 0}, 'inversion.pn_samples'),
                        ({'pn_reg': 1e-3, 'pn_seed': 'a'}, 'inversion.pn_seed'), ({'pn_reg': 1e-3, 'pn_floor': float('nan')}, 'inversion.pn_floor'),
                        ({'pn_reg': 1e-3, 'latent_space': 's'}, 'inversion.pn_reg')):
        with pytest.raises(ValueError, match=name):
            cli.run({'name': 'x', 'datasets': {}, 'inversion': block})


@pytest.mark.gpu
def test_cli_keys_reach_the_loop(tmp_path, monkeypatch, caplog):
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
            calls.append({n: k.get(n) for n in ('pn_reg', 'pn_samples', 'pn_seed', 'pn_floor')})
            return inner(x, enc_lats=enc.to(x.device), noise=[n.to(x.device) for n in noise], **k)

        m.invert = invert
        calls.append(m)
        return m

    monkeypatch.setattr(cli, 'load_model', load)
    opts = {'name': 'pn', 'save_dir': str(tmp_path / 'out'), 'datasets': {'val': {'dataroot': str(tmp_path / 'data')}},
            'network_g': {'type': 'ood_faceGAN_e4e', 'out_size': size}, 'metrics': {'psnr': {'crop_border': 0, 'test_y_channel': False}},
            'inversion': {'wplus_steps': 3, 'batch': 2, 'pn_reg': 1e-3, 'pn_samples': 4096, 'pn_seed': 2, 'pn_floor': 1e-4}}
    with caplog.at_level(logging.INFO, logger='oodgan.cli'):
        summary = cli.run(opts)
    model, call = calls
    assert call == dict(pn_reg=1e-3, pn_samples=4096, pn_seed=2, pn_floor=1e-4)
    st = model.last_pn_stats
    assert (st.n, st.seed, st.floor) == (4096, 2, 1e-4)
    table = model.last_loss_terms['pn']
    assert table.shape == (3, 2) and set(summary['val']['pn']) == set(files)
    assert [summary['val']['pn'][f] for f in files] == table[-1].tolist()            # the last row, no extra pass
    assert all(f'Final P_N+ distance of val/{f}' in caplog.text for f in files)
    assert np.isfinite(summary['val']['psnr']) and os.path.isfile(tmp_path / 'out' / 'pn' / 'val' / 'inversion' / files[0])
    # without the keys: no entry, and the loop runs without the term
    del calls[:]
    opts['inversion'] = {'wplus_steps': 3, 'batch': 2}
    summary = cli.run(opts)
    assert 'pn' not in summary['val'] and calls[0].last_loss_terms['pn'] is None and calls[1]['pn_reg'] == 0.0
