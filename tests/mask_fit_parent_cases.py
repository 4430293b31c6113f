"""The runs that pin ``loss_region='full'`` and ``'blend'`` to the commit before the fitted mask entered ``_WRun``: what
tests/golden/make_wplus_maskfit_parent.py records on that commit and tests/test_hip_mask_fit.py recomputes.

Model level, 256², B = 2, six steps (the carry path and three replayed steps): 'full' (the plain MSE), 'blend' (the composite MSE alone: one
kernel writes beta*dL/dc) and 'blend_ssim' (the composite route with a second term: dL/dc, c, then ``scale_by_plane`` — the call the fitted
mask's chain kernel stands in for).  Per run the float32 bits of the losses, the SHA-256 of the latents and of the output image,
``last_invert_stats``, the launches of the recorded plan and every dispatch counter that existed on that commit.  Only ``invert``'s public
surface is used, so the same code drives both commits."""
import hashlib

import numpy as np
import torch

from oodgan import synth

SIZE, B, STEPS = 256, 2, 6
CASES = {'full': dict(loss_region='full'), 'blend': dict(loss_region='blend'), 'blend_ssim': dict(loss_region='blend', ssim_weight=0.5)}
COUNTERS = ('stripx', 'strip', 's1big', 's1v2', 's1pp', 'tiny', 't2big', 't2v2', 't2gen', 's2big', 's2v2', 's2gen', 'upvb', 's1big_ys',
            's2big_fuse', 's2big_dotx_sform', 's1big_g2', 's2big_g2', 'stripx_g2', 's2big_xh', 's1big_xh', 'composite_mse', 'ssim', 'robust',
            'area_pool', 'pooled_pixel', 'pn', 'resampled_pixel')


def model(dev):
    from oodgan.arch import ood_faceGAN_e4e
    m = ood_faceGAN_e4e(out_size=SIZE, style_dim=512, encoder='E4E', enable_modulation=True, warp_scale=0.08, cycle_align=2, blend_with_gen=True,
                        ModSize=256, build_encoder=False)
    res = m.load_state_dict(synth.ood_state(SIZE, seed=41), strict=False)
    assert not res.missing_keys and not res.unexpected_keys, res
    return m.to(dev).eval()


def inputs(dev):
    x = synth.make_images(SIZE, B, seed=44).to(dev)
    return x, dict(enc_lats=synth.make_latents(SIZE, B, seed=42, std=0.3).to(dev), enc_feats=[f.to(dev) for f in synth.make_encoder_feats(B, seed=43)],
                   noise=[n.to(dev) for n in synth.make_noises(SIZE, B, seed=45)])


def _sha(t):
    return np.frombuffer(hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).digest(), dtype=np.uint8)


def record(m, x, kw, name):
    """dict(loss_bits, w_sha, out_sha, steps_run, rollbacks, launches, counters) of one case on the model ``m``."""
    from oodgan import _lib
    _lib.dispatch_reset()
    out, lats, losses = m.invert(x, steps=STEPS, **CASES[name], **kw)
    torch.cuda.synchronize()
    return dict(loss_bits=losses.detach().cpu().contiguous().numpy().view(np.uint32).copy(), w_sha=_sha(lats), out_sha=_sha(out),
                steps_run=np.array(m.last_invert_stats['steps_run'], dtype=np.int64),
                rollbacks=np.array(m.last_invert_stats['rollbacks'], dtype=np.int64),
                launches=np.array(m.last_invert_plan['launches'], dtype=np.int64),
                counters=np.array([_lib.dispatch_count(c) for c in COUNTERS], dtype=np.int64))
