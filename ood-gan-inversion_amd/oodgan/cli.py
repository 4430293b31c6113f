"""``python -m oodgan.cli --opt options/test/E4E_Face_test.yml`` — the harness around the accelerated path, with the
YAML option surface of the reference's run_ood_faceGAN_inversion.py:

    name, save_dir, directions_dir
    datasets: {<name>: {dataroot, editing: {direction, intensity}}}
    network_g: {type: ood_faceGAN_e4e, ...constructor kwargs...}
    path: {pretrain_network_g, param_key_g, strict_load_g}
    metrics: {psnr|ssim|lpips|identity: {crop_border, test_y_channel[, model_path]}}

Per image it does what the reference does (read -> [-1,1] RGB 1024² -> model -> save inversion + mask strip -> metrics)
and, when the build-defined block ``inversion: {wplus_steps: N, lr: 0.01, batch: B}`` (or ``--wplus-steps``) is
present, refines the encoder latents with N W+ Adam steps before the OOD forward (``streams: S``
in the same block advances the loop on S concurrent HIP streams, default 1; ``graph: true`` replays the plain forward from a
captured hipGraph).
Where the W+ loss looks, in the same block:

    loss_region: full | blend | fit    full (default): every pixel.  blend: the blended output the model returns, x + beta*(G - x) with
                                 beta = (1 - alpha)^blend_cnt from the mask of the OOD forward at the start latents.  fit:
                                 the loop fits a low-resolution mask beside the latents, under the reference's mask objective (an area
                                 budget and a binarisation term), and weights the loss with it; its options, all optional:
                                 mask_size (64; 16, 32, 64, 128 or 256, dividing the generator size by >= 2), mask_lr (0.1),
                                 mask_area (0.30), mask_area_weight (5.0), mask_binary_weight (0.2), mask_init (0.88: a number in
                                 (0, 1), or blend), fit_blend (false; true: the output is blended with the fitted mask instead of
                                 the SAMM mask).  Not with mask_dir, pixel_size, pixel_filter / pixel_target, latent_space: s or
                                 feature_layer.  A bad value is an error.
    align: similarity            the loop fits, beside the latents, a similarity (log-scale, rotation, translation) per image and compares
                                 G(w) with the input warped by it: a photograph a few pixels or a degree off the generator's
                                 canonical frame is registered instead of costing the latents.  The saved inversion is in the ALIGNED frame,
                                 while the metrics still compare it with the input file in ITS frame: with this option they are taken
                                 across two frames and understate the fit (a warning says so once per run).
                                 align_lr (0.001: about half a pixel per step at 1024²; not a measured optimum; >= 0), align_reg (0:
                                 the weight of sum theta^2; >= 0).  Not with lpips_weight, ssim_weight, loss_region other than full,
                                 mask_dir, a non-box pixel_filter, pixel_target, latent_space: s or feature_layer.  A bad value is an error.
    color: gain | affine         the loop fits, beside the latents, a colour map (M, b) per image and takes the pixel term on M G + b
                                 (DESIGN.md §26): a colour cast, another exposure or faded film is explained by twelve numbers (gain: six,
                                 per-channel gain and offset) instead of costing the latents.  The saved inversion blends the input with the
                                 MAPPED generator image: it is in the input's colours.  The fitted map itself is not saved.
                                 color_lr (0.002: at most 0.2 of gain or 25 grey levels of offset over 100 steps; a choice, not a measured
                                 optimum; >= 0), color_reg (0: the weight of sum (theta - identity)^2; >= 0).  Goes with loss_region: blend
                                 and mask_dir.  Not with lpips_weight, ssim_weight, loss_region: fit, align, pixel_size, pixel_filter /
                                 pixel_target, latent_space: s or feature_layer.  A bad value is an error.
    mask_dir: <dir>              a caller mask per input file: <dir>/<base name>.png (grayscale; the first channel / 255 is beta,
                                 0 = ignore the pixel), resized nearest to the generator size.  A file without a mask is an error.
                                 Excludes ``loss_region: blend``.
    ssim_weight: <lambda>        adds lambda * (1 - SSIM) per image to the W+ loss: the SSIM this tool reports (11-tap Gaussian
                                 window, per channel), on the unrounded images, of the composite where a region is set.  Default 0 = off;
                                 negative or non-finite is an error.
    pixel_loss: mse | charbonnier | huber | geman_mcclure
                                 the pixel term: the mean of d^2 (default), sqrt(d^2 + s^2), Huber's d^2/2 up to |d| = s and
                                 s(|d| - s/2) beyond, or d^2/2 * s^2/(d^2 + s^2) over the residual d — robust kinds for occluders nobody masked.
    pixel_scale: <s>             their scale in image units ([-1,1] images), a finite number > 0.  Default 0.1, a tenth of the half-range (about
                                 13 grey levels): a choice, not a measured optimum.  huber with a very large s is half the MSE.
    lpips_size: <int>            the size the LPIPS term (``lpips_weight``) is taken at: the image and the target are area-pooled to
                                 it first; the projectors' value is 256.  Absent (default): the image's own size.  It must be >= 64 and divide the
                                 generator size by 1, 2, 4, 8 or 16; anything else is an error.
    pixel_size: <int>            the size the pixel term is taken at: the mean of rho over the residual of the area-pooled image
                                 and target, one fused kernel.  Absent (default) or the generator size: the full-resolution term.  It must divide
                                 the generator size by 1, 2, 4, 8 or 16; anything else is an error.  For a low-resolution photograph: feed it
                                 nearest-upsampled and give its own size here.
    pixel_filter: <name>         the filter of the ``pixel_size`` view: box (default: the area pool), bilinear, bicubic or lanczos3 —
                                 the antialiased resize a real low-resolution photograph was made with (PIL, OpenCV, F.interpolate(antialias=True)).
                                 Needs ``pixel_size`` or ``pixel_target``; not with ``loss_region: blend`` or ``mask_dir``.
    pixel_target: file           an input file of side n with generator size / n in 2, 4, 8, 16 supplies its own pixels as the target of the pixel
                                 term (the same uint8 -> [-1, 1] RGB conversion as the input, no resize) and fixes ``pixel_size`` = n; the
                                 bilinearly enlarged image still feeds the encoder and the OOD forward.  The files of one batch must share one
                                 size; a file already at the generator size is an error.  Absent (default): the target's view is made from the
                                 enlarged input.
The projector schedule of the W+ loop (rosinality's projector.py), in the same block, everything off by default:

    lr_rampup, lr_rampdown: <f>  fractions of the run over which the learning rate ramps up linearly / follows a cosine down (projector: 0.05, 0.25)
    latent_noise: <f>            Gaussian noise on the latent the generator reads, in multiples of the generator's latent standard deviation
                                 (projector: 0.05), decaying as max(0, 1 - (t / steps) / noise_ramp)^2; noise_ramp: <f> (default 0.75)
    noise_seed: <int>            the seed of those draws (default 0); a file's draws depend on its index in the data set's sorted list, not on
                                 ``batch`` or ``streams``
    latent_reg: <lambda>         adds lambda * mean (w - anchor)^2 per image; latent_anchor: start | mean (the start latents of the run, default;
                                 avg_latent + delta_latent)
Edits and the latent controls of the W+ loop, in the same block:

    edit: start | final          where a data set's ``editing`` direction goes when the loop runs.  start (default): into ``delta_latent``, as the
                                 reference does for the plain forward — the loop then fits the unedited input from edited start latents and
                                 works the edit off again (logged once as a warning).  final: the loop runs on the unedited latents and the
                                 direction is added to the refined latents for the final forward (``invert(edit=...)``).  Without W+ steps both
                                 are the reference's ``delta_latent += direction``.
    latent_space: w+ | w | s     w+ (default): every layer its own vector.  w: one 512-vector per image, started at the layer mean.  s: StyleSpace
                                  — the latents stay at their start and an offset on the per-channel styles is fitted; not with
                                 ``delta_reg``, ``latent_noise``, ``latent_reg``, nor with ``edit: final`` and a data set's (W+) editing direction.
    style_reg: <lambda>          ``latent_space: s`` only: adds lambda * the mean squared style offset per image.  Default 0 = off.
    layer_lr: [f, ...]           one factor >= 0 of ``lr`` per generator layer (18 at 1024²); 0 freezes a layer.  Not with ``latent_space: w``.
    delta_reg: <lambda>          adds lambda * the squared spread of the layers about their mean per image (the symmetric form of e4e's
                                 regulariser, which measures from layer 0).  Default 0 = off.  Not with ``latent_space: w``.
The feature offset of the W+ loop (the F/W+ family), in the same block:

    feature_layer: 3 | 5 | 7     beside the latents, fit an offset on the 8² / 16² / 32² input of the styled up-conv that reads that latent (5:
                                 Feature-Style's index): a code for content no latent can express.  Not with ``latent_space: s``.  Default: off.
    feature_lr: <f>              the offset's learning rate (default: ``lr`` — a choice, not a measured optimum); 0 leaves the offset at zero
    feature_reg: <lambda>        adds lambda * the mean squared offset per image.  Default 0 = off.
The P_N+ prior of the W+ loop (II2S, Zhu et al.), in the same block:

    pn_reg: <lambda>             adds lambda * the squared length of the latent in the whitened space of the mapping network's outputs (after
                                 undoing its last LeakyReLU), the mean over layers and columns, per image: the Mahalanobis distance to the
                                 latents the generator was trained on — for fits that reconstruct well and edit badly.  Default 0 = off.  Not
                                 with ``latent_space: s``.  The summary logs each file's final value.
    pn_samples: <int>            the mapping-network samples the statistics are taken over (default 100000; at least 2, more than 512 without
                                 a floor); pn_seed: <int> their seed (default 0)
    pn_floor: <f>                the variances are floored at f * the largest one (default 0: no floor)
Where the host work around a chunk runs, in the same block:

    io: device | host            device (default): files are uploaded as uint8 and converted on the GPU, the inversion, the mask strip, PSNR and
                                 SSIM are computed there as uint8 / from uint8, the uint8 arrays are downloaded, PNG encoding and writing go to
                                 ``io_workers`` threads, and the next chunk's files are decoded while the GPU works on this one.  host: every
                                 step on the calling thread, in numpy.  Same files and the same PSNR either way; SSIM agrees to 1e-9.
    io_workers: <int>            the threads that encode and write under ``io: device`` (as many again decode ahead): an integer in [1, 16], default 4
``summary[name]['time']`` is the model call per image; ``summary[name]['wall']`` the data set's whole loop per image, files in to files out.
``model_dict`` holds the reference's three variants (run_ood_faceGAN_inversion.py:23-27): the ``network_g`` blocks of
options/test/{E4E,ReStyle,FeatureStyle}_Face_test.yml resolve unchanged.  LPIPS / identity need third-party weights that
do not ship: they are reported as skipped."""
import argparse
import collections
import logging
import os
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch
import yaml

from . import imgio
from .arch import ood_faceGAN_e4e, ood_faceGAN_FeatureStyle, ood_faceGAN_restyle
from .engine import check_latent_controls, check_style_space, check_lpips_size, check_noise_seed, check_pixel_filter, check_pixel_loss, check_pixel_size, check_nonneg, check_feature_offset, check_feature_layer, check_pn_options, check_mask_fit, check_mask_init, refuse_mask_fit, check_align, refuse_align, check_color, refuse_color
from .io import load_direction, load_network_g

model_dict = {                                   # run_ood_faceGAN_inversion.py:23-27
    'ood_faceGAN_e4e': ood_faceGAN_e4e,
    'ood_faceGAN_restyle': ood_faceGAN_restyle,
    'ood_faceGAN_FeatureStyle': ood_faceGAN_FeatureStyle,
}
IMG_EXT = ('.png', '.jpg', '.jpeg', '.bmp', '.webp')


def load_model(opts):
    """run_ood_faceGAN_inversion.py:30-47."""
    opt = dict(opts['network_g'])
    model_type = opt.pop('type')
    if model_type not in model_dict:
        raise KeyError(f'network_g.type {model_type!r} is not available in this build (have: {sorted(model_dict)})')
    model = model_dict[model_type](**opt)
    p = opts.get('path') or {}
    if p.get('pretrain_network_g'):
        load_network_g(model, p['pretrain_network_g'], p.get('param_key_g', 'params_ema'), p.get('strict_load_g', False))
    return model


def load_files_from_path(opt, directions_dir=None):
    """:49-62 — sorted by file name without its extension."""
    root = opt['dataroot']
    names = [n for n in os.listdir(root) if n.lower().endswith(IMG_EXT)]
    names = sorted(names, key=lambda x: x[:-4])
    return [os.path.join(root, n) for n in names], load_direction(directions_dir, opt.get('editing'))


def mask_to_weight(mask, size):
    """An HxW(xC) mask image (uint8 values 0..255; the first channel is read) -> the (1,1,size,size) float32 loss weight mask/255, resized
    nearest (F.interpolate(mode='nearest'): src = floor(dst*in/out))."""
    m = np.asarray(mask)
    if m.ndim == 3:
        m = m[:, :, 0]
    if m.ndim != 2 or m.size == 0:
        raise ValueError(f'a loss mask must be an HxW or HxWxC image, got shape {np.asarray(mask).shape}')
    m = m.astype(np.float64)
    if not (np.isfinite(m).all() and m.min() >= 0.0 and m.max() <= 255.0):
        raise ValueError(f'loss mask values must lie in [0, 255], got [{m.min()}, {m.max()}]')
    H, W = m.shape
    rows = (np.arange(size) * H) // size
    cols = (np.arange(size) * W) // size
    beta = (m[rows][:, cols] / 255.0).astype(np.float32)
    return torch.from_numpy(np.ascontiguousarray(beta)).reshape(1, 1, size, size)


def load_loss_weights(files, mask_dir, size):
    """beta (B,1,size,size) float32 for the input ``files``: <mask_dir>/<base name>.png each (``mask_to_weight``); a missing mask raises."""
    out = []
    for f in files:
        path = os.path.join(mask_dir, os.path.splitext(os.path.basename(f))[0] + '.png')
        if not os.path.isfile(path):
            raise FileNotFoundError(f'inversion.mask_dir: no mask {path} for input {f}')
        out.append(mask_to_weight(imgio.imread(path)[:, :, ::-1], size))     # imread gives BGR: its last channel is the file's first
    return torch.cat(out, 0)


def evaluate(gt_bgr, res_bgr, metrics, opt):
    """:89-126 — gt and result as [0,255] BGR arrays."""
    if metrics is None:
        metrics = {'psnr': [], 'ssim': [], 'lpips': [], 'identity': []}
    opt = opt or {}
    if opt.get('psnr'):
        metrics['psnr'].append(imgio.calculate_psnr(gt_bgr, res_bgr, crop_border=opt['psnr']['crop_border'],
                                                    test_y_channel=opt['psnr']['test_y_channel']))
    if opt.get('ssim'):
        metrics['ssim'].append(imgio.calculate_ssim(gt_bgr, res_bgr, crop_border=opt['ssim']['crop_border'],
                                                    test_y_channel=opt['ssim']['test_y_channel']))
    return metrics


def pixel_target_option(inv):
    """``inversion.pixel_target``: absent / None (the view of the enlarged input) or 'file' (each input file's own pixels); returns True for 'file'."""
    v = inv.get('pixel_target')
    if v is not None and v != 'file':
        raise ValueError(f"inversion.pixel_target must be absent or 'file', got {v!r}")
    return v == 'file'


def pixel_target_from_files(bgrs, files, size):
    """The pixel target of one batch under ``inversion.pixel_target: file``: the files' own pixels, (B,3,n,n) float32 RGB in [-1, 1] on the
    device, converted as the input is and never resized.  ``bgrs``: the decoded files, (n,n,3) uint8 tensors on the device or host arrays
    (any dtype holding 0..255).  ValueError for files of different sizes, a file that is not square, one already at the generator size and
    a side n with size / n not in 2, 4, 8, 16."""
    shapes = {tuple(b.shape[:2]) for b in bgrs}
    if len(shapes) != 1:
        raise ValueError(f'inversion.pixel_target: file needs the files of one batch at one size, got {sorted(shapes)} for {list(files)}')
    h, n = next(iter(shapes))
    if h != n or n >= size or size % n != 0 or size // n not in (2, 4, 8, 16):
        raise ValueError(f'inversion.pixel_target: file needs square inputs of side n with {size} / n in [2, 4, 8, 16], got {h}x{n} for '
                         f'{list(files)}' + (' (already at the generator size: drop the option)' if (h, n) == (size, size) else ''))
    if isinstance(bgrs[0], torch.Tensor):
        return imgio.input_from_u8(torch.stack(bgrs), n)
    return torch.cat([imgio.image_to_input(bgr, n, device='cuda') for bgr in bgrs], 0)


def schedule_options(inv):
    """The projector-schedule keywords of ``model.invert`` from the ``inversion`` block, checked (ValueError names the option)."""
    defaults = dict(lr_rampup=0.0, lr_rampdown=0.0, latent_noise=0.0, noise_ramp=0.75, latent_reg=0.0)
    kw = {k: check_nonneg(inv.get(k, d), f'inversion.{k}') for k, d in defaults.items()}
    kw['noise_seed'] = check_noise_seed(inv.get('noise_seed', 0), 'inversion.noise_seed')
    kw['latent_anchor'] = inv.get('latent_anchor', 'start')
    if kw['latent_anchor'] not in ('start', 'mean'):
        raise ValueError(f"inversion.latent_anchor must be 'start' or 'mean', got {kw['latent_anchor']!r}")
    return kw


def latent_options(inv, n_layers=None):
    """The latent-control keywords of ``model.invert`` from the ``inversion`` block, checked (ValueError names the option); ``n_layers``: the
    generator's layer count once the model exists."""
    space, rates, reg = check_latent_controls(inv.get('latent_space', 'w+'), inv.get('layer_lr'), inv.get('delta_reg', 0.0), n_layers, 'inversion.')
    return dict(latent_space=space, layer_lr=None if rates is None else list(rates), delta_reg=reg)


def style_options(inv):
    """``inversion.style_reg`` for ``model.invert``, checked against ``inversion.latent_space`` and the options StyleSpace excludes (ValueError
    names the option)."""
    return dict(style_reg=check_style_space(inv.get('latent_space', 'w+'), inv.get('style_reg', 0.0), inv.get('delta_reg', 0.0),
                                            inv.get('latent_noise', 0.0), inv.get('latent_reg', 0.0), 'inversion.'))


def feature_options(inv, n_latent=None):
    """``inversion.feature_layer`` / ``feature_lr`` / ``feature_reg`` for ``model.invert``, checked one by one and against
    ``inversion.latent_space`` (ValueError names the option); ``n_latent``: the generator's latent count once the model exists."""
    layer, rate, reg = check_feature_offset(inv.get('feature_layer'), inv.get('feature_lr'), inv.get('feature_reg', 0.0), None,
                                            inv.get('latent_space', 'w+'), 'inversion.')
    check_feature_layer(layer, n_latent, 'inversion.feature_layer')
    return dict(feature_layer=layer, feature_lr=rate, feature_reg=reg)


MASK_FIT_KEYS = ('mask_size', 'mask_lr', 'mask_area', 'mask_area_weight', 'mask_binary_weight', 'mask_init', 'fit_blend')


def mask_fit_options(inv, image_size=None):
    """``inversion.loss_region: fit`` and its keys (MASK_FIT_KEYS) for ``model.invert``, checked one by one (ValueError names the option;
    NotImplementedError for what the fitted mask does not go with) — before the GPU is touched.  {} unless the region is 'fit'; any of the keys
    without it is an error."""
    if inv.get('loss_region', 'full') != 'fit':
        stray = [k for k in MASK_FIT_KEYS if k in inv]
        if stray:
            raise ValueError(f'inversion.{stray[0]} needs inversion.loss_region: fit')
        return {}
    if inv.get('mask_dir'):
        raise ValueError('inversion.mask_dir and inversion.loss_region: fit exclude each other')
    m, rate, area, wa, wb = check_mask_fit(inv.get('mask_size', 64), inv.get('mask_lr', 0.1), inv.get('mask_area', 0.30),
                                           inv.get('mask_area_weight', 5.0), inv.get('mask_binary_weight', 0.2), image_size, 'inversion.')
    init = inv.get('mask_init', 0.88)
    if isinstance(init, torch.Tensor):
        raise ValueError("inversion.mask_init must be a number in (0, 1) or 'blend'")
    init = check_mask_init(init, name='inversion.mask_init')
    blend = inv.get('fit_blend', False)
    if not isinstance(blend, bool):
        raise ValueError(f'inversion.fit_blend must be true or false, got {blend!r}')
    refuse_mask_fit(False, inv.get('pixel_size'), check_pixel_filter(inv.get('pixel_filter'), 'inversion.pixel_filter'),
                    inv.get('pixel_target'), inv.get('latent_space', 'w+'), inv.get('feature_layer'))
    return dict(mask_size=m, mask_lr=rate, mask_area=area, mask_area_weight=wa, mask_binary_weight=wb, mask_init=init, fit_blend=blend)


ALIGN_KEYS = ('align', 'align_lr', 'align_reg')


def align_options(inv):
    """``inversion.align`` / ``align_lr`` / ``align_reg`` for ``model.invert``, checked one by one (ValueError names the option;
    NotImplementedError for what the alignment does not go with) — before the GPU is touched.  {} without ``align``; either of the other
    two without it is an error."""
    if inv.get('align') is None:
        stray = [k for k in ALIGN_KEYS[1:] if k in inv]
        if stray:
            raise ValueError(f'inversion.{stray[0]} needs inversion.align')
        return {}
    kind, rate, reg = check_align(inv['align'], inv.get('align_lr', 0.001), inv.get('align_reg', 0.0), 'inversion.')
    lpips_weight, ssim_weight = inv.get('lpips_weight', 0.0), inv.get('ssim_weight', 0.0)
    refuse_align(False, bool(lpips_weight), bool(ssim_weight), 'mask_dir' if inv.get('mask_dir') else inv.get('loss_region', 'full'),
                 check_pixel_filter(inv.get('pixel_filter'), 'inversion.pixel_filter'), inv.get('pixel_target'), inv.get('latent_space', 'w+'),
                 inv.get('feature_layer'))
    return dict(align=kind, align_lr=rate, align_reg=reg)


COLOR_KEYS = ('color', 'color_lr', 'color_reg')


def color_options(inv):
    """``inversion.color`` / ``color_lr`` / ``color_reg`` for ``model.invert``, checked one by one (ValueError names the option;
    NotImplementedError for what the colour map does not go with) — before the GPU is touched.  {} without ``color``; either of the other
    two without it is an error."""
    if inv.get('color') is None:
        stray = [k for k in COLOR_KEYS[1:] if k in inv]
        if stray:
            raise ValueError(f'inversion.{stray[0]} needs inversion.color')
        return {}
    kind, rate, reg = check_color(inv['color'], inv.get('color_lr', 0.002), inv.get('color_reg', 0.0), 'inversion.')
    refuse_color(False, bool(inv.get('lpips_weight', 0.0)), bool(inv.get('ssim_weight', 0.0)), inv.get('loss_region', 'full'), inv.get('align'),
                 inv.get('pixel_size'), check_pixel_filter(inv.get('pixel_filter'), 'inversion.pixel_filter'), inv.get('pixel_target'),
                 inv.get('latent_space', 'w+'), inv.get('feature_layer'))
    return dict(color=kind, color_lr=rate, color_reg=reg)


def pn_options(inv):
    """``inversion.pn_reg`` / ``pn_samples`` / ``pn_seed`` / ``pn_floor`` for ``model.invert``, checked one by one and against
    ``inversion.latent_space`` (ValueError names the option) — before the GPU is touched."""
    reg, n, seed, floor = check_pn_options(inv.get('pn_reg', 0.0), inv.get('pn_samples', 100000), inv.get('pn_seed', 0), inv.get('pn_floor', 0.0),
                                           inv.get('latent_space', 'w+'), 'inversion.')
    return dict(pn_reg=reg, pn_samples=n, pn_seed=seed, pn_floor=floor)


def check_edit_space(edit_at, latent_space, has_direction, name=''):
    """``edit: final`` hands the data set's direction to ``invert(edit=)``; with ``latent_space: s`` that must be a StyleSpace direction, and
    the direction files of the reference are W+ (there is no S-direction file format): ValueError."""
    if edit_at == 'final' and latent_space == 's' and has_direction:
        raise ValueError(f"inversion.edit: final with inversion.latent_space: s: the editing direction of data set {name!r} is a W+ direction, "
                         "the fit runs in StyleSpace and takes StyleSpace directions only (there is no file format for those); use "
                         "inversion.edit: start, or latent_space: w+")


def edit_option(inv):
    """``inversion.edit``: 'start' (default) or 'final'; anything else raises ValueError."""
    edit = inv.get('edit', 'start')
    if edit not in ('start', 'final'):
        raise ValueError(f"inversion.edit must be 'start' or 'final', got {edit!r}")
    return edit


def io_options(inv):
    """(``inversion.io``, ``inversion.io_workers``), checked.  The worker count is the user's: never derived from the machine's CPU count, which on a
    shared box says nothing about the CPUs this process may use."""
    io, workers = inv.get('io', 'device'), inv.get('io_workers', 4)
    if io not in ('device', 'host'):
        raise ValueError(f"inversion.io must be 'device' or 'host', got {io!r}")
    if isinstance(workers, bool) or not isinstance(workers, int) or not 1 <= workers <= 16:
        raise ValueError(f'inversion.io_workers must be an integer in [1, 16], got {workers!r}')
    return io, workers


class WriterPool:
    """``workers`` threads for the PIL / numpy side of a chunk (PNG encode + write, host metrics): ``submit`` hands a call over and blocks while
    2 * workers are in flight, ``drain`` waits for all of them and returns their results in submission order.  A worker's exception is raised
    from the ``submit`` or ``drain`` that collects it; leaving the ``with`` block cancels what has not started and joins the threads.
    The tasks must not touch HIP or torch-ROCm: the library's calls belong to the thread that owns the stream."""

    def __init__(self, workers):
        self.limit = 2 * workers
        self.max_pending = 0                    # the most tasks that were in flight at once
        self._executor = ThreadPoolExecutor(max_workers=workers, thread_name_prefix='oodgan-io')
        self._pending, self._results = collections.deque(), []

    def submit(self, fn, *args):
        while len(self._pending) >= self.limit:
            self._results.append(self._pending.popleft().result())
        self._pending.append(self._executor.submit(fn, *args))
        self.max_pending = max(self.max_pending, len(self._pending))

    def drain(self):
        while self._pending:
            self._results.append(self._pending.popleft().result())
        results, self._results = self._results, []
        return results

    def close(self):
        self._executor.shutdown(wait=True, cancel_futures=True)
        self._pending.clear()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def postprocess_host(out, x, aligns, files, bgrs, size, save_dir, metrics, metric_opts):
    """``io: host`` — a chunk's outputs on the calling thread: per file the inversion and the mask strip as uint8 (``tensor2img``), written, and
    the metrics against the file (its own pixels when it is size x size, else the uint8 of ``x``).  Returns (metrics, inversions, strips)."""
    results, strips = [], []
    for k, (f, bgr) in enumerate(zip(files, bgrs)):
        res = imgio.tensor2img(out[k:k + 1], rgb2bgr=True, min_max=(-1, 1))
        imgio.imwrite(os.path.join(save_dir, 'inversion', os.path.basename(f)), res)
        gt = bgr if bgr.shape[:2] == (size, size) else imgio.tensor2img(x[k:k + 1], rgb2bgr=True, min_max=(-1, 1)).astype(np.float64)
        metrics = evaluate(gt, res, metrics, metric_opts)
        masks = imgio.extract_masks(aligns, size, index=k)
        if masks is not None:
            imgio.imwrite(os.path.join(save_dir, 'masks', os.path.basename(f)), masks)
        results.append(res)
        strips.append(masks)
    return metrics, results, strips


def _host_metric(kind, gt, res, opt):
    fn = imgio.calculate_psnr if kind == 'psnr' else imgio.calculate_ssim
    return kind, fn(gt, res, crop_border=opt['crop_border'], test_y_channel=opt['test_y_channel'])


def postprocess_device(out, x, aligns, files, bgrs, size, save_dir, metrics, metric_opts, pool):
    """``io: device`` — the same outputs with the arithmetic on the GPU (oodgan/imgio.py, device counterparts): the calling thread converts the
    chunk to uint8, takes PSNR / SSIM there, downloads the uint8 arrays and hands each file's encode + write to ``pool``.  ``bgrs``: the files
    as uint8 BGR, host arrays or device tensors.  A metric with test_y_channel runs as the host function on a worker; its value arrives with
    ``collect_host_metrics(pool.drain(), metrics)``.  Returns (metrics, inversions, strips) — host arrays, (B,size,size,3) and (B,size,size*n) or None."""
    if metrics is None:
        metrics = {'psnr': [], 'ssim': [], 'lpips': [], 'identity': []}
    opt = {k: v for k, v in (metric_opts or {}).items() if k in ('psnr', 'ssim') and v}
    res = imgio.tensor2img_device(out, rgb2bgr=True, min_max=(-1, 1))
    strips = imgio.extract_masks_device(aligns, size)
    gt = None
    if opt:
        own = [tuple(b.shape[:2]) == (size, size) for b in bgrs]
        gt = torch.empty_like(res) if all(own) else imgio.tensor2img_device(x, rgb2bgr=True, min_max=(-1, 1))
        for k, b in enumerate(bgrs):
            if own[k]:
                gt[k].copy_(torch.as_tensor(b))
        on_device = {k: v for k, v in opt.items() if not v['test_y_channel']}
        for crop in sorted({v['crop_border'] for v in on_device.values()}):
            psnr, ssim = imgio.psnr_ssim_device(gt, res, crop)
            for kind, values in (('psnr', psnr), ('ssim', ssim)):
                if kind in on_device and on_device[kind]['crop_border'] == crop:
                    metrics[kind] += values
    res = res.cpu().numpy()
    strips = None if strips is None else strips.cpu().numpy()
    luma = {k: v for k, v in opt.items() if v['test_y_channel']}
    gt = gt.cpu().numpy() if luma else None
    for k, f in enumerate(files):
        pool.submit(imgio.imwrite, os.path.join(save_dir, 'inversion', os.path.basename(f)), res[k])
        if strips is not None:
            pool.submit(imgio.imwrite, os.path.join(save_dir, 'masks', os.path.basename(f)), strips[k])
        for kind, v in luma.items():
            pool.submit(_host_metric, kind, gt[k], res[k], v)
    return metrics, res, strips


def collect_host_metrics(results, metrics):
    """Appends the (kind, value) results of the pool's metric tasks to ``metrics`` — submission order is file order."""
    for r in results:
        if r is not None:
            metrics[r[0]].append(r[1])
    return metrics


def run(opts, wplus_steps=None, log=None):
    log = log or logging.getLogger('oodgan.cli')
    inv = opts.get('inversion') or {}
    io, io_workers = io_options(inv)
    loss_region, mask_dir = inv.get('loss_region', 'full'), inv.get('mask_dir')
    if loss_region not in ('full', 'blend', 'fit'):
        raise ValueError(f"inversion.loss_region must be 'full', 'blend' or 'fit', got {loss_region!r}")
    if mask_dir and loss_region == 'blend':
        raise ValueError('inversion.mask_dir and inversion.loss_region: blend exclude each other')
    out_size0 = (opts.get('network_g') or {}).get('out_size')
    fit_opts = mask_fit_options(inv, out_size0 if isinstance(out_size0, int) else None)
    ssim_weight = check_nonneg(inv.get('ssim_weight', 0.0), 'inversion.ssim_weight')
    pixel_loss, pixel_scale = check_pixel_loss(inv.get('pixel_loss', 'mse'), inv.get('pixel_scale', 0.1), 'inversion.pixel_loss',
                                               'inversion.pixel_scale')
    out_size = (opts.get('network_g') or {}).get('out_size')
    lpips_size = check_lpips_size(inv.get('lpips_size'), out_size if isinstance(out_size, int) else None, 'inversion.lpips_size')
    pixel_size = check_pixel_size(inv.get('pixel_size'), out_size if isinstance(out_size, int) else None, 'inversion.pixel_size')
    pixel_filter = check_pixel_filter(inv.get('pixel_filter'), 'inversion.pixel_filter')
    target_from_file = pixel_target_option(inv)
    if (pixel_filter is not None or target_from_file) and (mask_dir or loss_region != 'full'):
        raise ValueError('inversion.pixel_filter / inversion.pixel_target take neither inversion.mask_dir nor inversion.loss_region: blend')
    if pixel_filter is not None and pixel_size is None and not target_from_file:
        raise ValueError(f'inversion.pixel_filter: {pixel_filter} needs inversion.pixel_size or inversion.pixel_target: file')
    sched = schedule_options(inv)
    sched.update(latent_options(inv))
    sched.update(style_options(inv))
    sched.update(feature_options(inv))
    sched.update(pn_options(inv))
    sched.update(fit_opts)
    sched.update(align_options(inv))
    sched.update(color_options(inv))
    edit_at = edit_option(inv)
    steps = int(wplus_steps if wplus_steps is not None else inv.get('wplus_steps', 0))
    directions_dir = opts.get('directions_dir', './directions')
    if edit_at == 'final' and steps > 0 and sched['latent_space'] == 's':      # before the model is built and any data set is processed
        for name, dopt in opts['datasets'].items():
            check_edit_space(edit_at, 's', load_direction(directions_dir, dopt.get('editing')).dim() > 0, name)
    if not torch.cuda.is_available():
        raise RuntimeError('oodgan.cli needs a ROCm GPU: the HIP path has no CPU fallback')
    model = load_model(opts).cuda().eval()
    save_root = os.path.join(opts.get('save_dir', './results'), opts['name'])
    lr = float(inv.get('lr', 0.01))
    streams = int(inv.get('streams', 1))
    lpips_weight = float(inv.get('lpips_weight', 0.0))       # opt-in perceptual term of the W+ loss (oodgan/lpips.py)
    lpips_state = torch.load(inv['lpips_path'], map_location='cpu') if inv.get('lpips_path') else None
    if sched.get('align') is not None and opts.get('metrics'):
        log.warning('inversion.align: the saved inversions are in the aligned frame, the metrics compare them with the input files in their own '
                    'frame — they are taken across two frames')
    if lpips_weight and lpips_state is None:
        log.warning('inversion.lpips_weight without inversion.lpips_path: the LPIPS term runs on SEEDED AlexNet / lin weights (the lpips package\'s '
                    'pretrained weights are not part of this build)')
    graphed = None
    if inv.get('graph', False) and steps == 0:
        from .arch import GraphedForward
        graphed = GraphedForward(model)          # model(x) replayed from a hipGraph: -6 % latency per image at batch 1
    size = model.generator.size
    check_lpips_size(lpips_size, size, 'inversion.lpips_size')
    pixel_size = check_pixel_size(pixel_size, size, 'inversion.pixel_size')
    if pixel_filter is not None and pixel_size is None and not target_from_file:
        raise ValueError(f'inversion.pixel_filter: {pixel_filter} needs inversion.pixel_size below the generator size {size}')
    latent_options(inv, model.generator.n_latent)
    feature_options(inv, model.generator.n_latent)
    mask_fit_options(inv, size)
    summary = {}
    for name, dopt in opts['datasets'].items():
        files, direction = load_files_from_path(dopt, directions_dir)
        save_dir = os.path.join(save_root, name)
        # ``edit: final`` with a W+ loop: the direction stays out of the start latents and goes on after the fit (invert(edit=...))
        edit_final = edit_at == 'final' and steps > 0
        edit = None
        if edit_final:
            if direction.dim() > 0:
                edit = direction.cuda().float().contiguous()
        else:
            if steps > 0 and bool((direction != 0).any()):
                log.warning('inversion.wplus_steps with an editing direction and inversion.edit: start — the W+ loop fits the UNEDITED input '
                            'starting from edited latents (it works the edit off again); inversion.edit: final applies the direction after the fit')
            model.delta_latent.data += direction.cuda()
        times, metrics, pn_final = [], None, []
        # ``inversion.batch`` files per call (default 1 = the reference's per-file loop, run_ood_faceGAN_inversion.py:158-182): images are
        # independent on this path, and the W+ loop of one image leaves most of the GPU idle (284 ms per image alone, 131 ms in a batch of 8)
        nb = max(1, int(inv.get('batch', 1)))
        chunks = [files[c0:c0 + nb] for c0 in range(0, len(files), nb)]
        wall0 = time.time()
        with WriterPool(io_workers) as pool, ThreadPoolExecutor(max_workers=io_workers, thread_name_prefix='oodgan-read') as reader:
            # io: device — the next chunk's files are decoded by ``reader`` while the GPU works on this one
            ahead = [reader.submit(imgio.imread, f) for f in chunks[0]] if (io == 'device' and chunks) else None
            for ci, chunk in enumerate(chunks):
                c0 = ci * nb
                if io == 'device':
                    bgrs = [torch.from_numpy(t.result()).cuda() for t in ahead]
                    ahead = [reader.submit(imgio.imread, f) for f in chunks[ci + 1]] if ci + 1 < len(chunks) else None
                    if len({tuple(b.shape) for b in bgrs}) == 1:
                        x = imgio.input_from_u8(torch.stack(bgrs), size)
                    else:
                        x = torch.cat([imgio.input_from_u8(bgr, size) for bgr in bgrs], 0)
                else:
                    bgrs = [imgio.imread(f).astype(np.float64) for f in chunk]
                    x = torch.cat([imgio.image_to_input(bgr, size, device='cuda') for bgr in bgrs], 0)
                region = load_loss_weights(chunk, mask_dir, size).cuda() if (mask_dir and steps > 0) else loss_region
                pixel_target = pixel_target_from_files(bgrs, chunk, size) if (target_from_file and steps > 0) else None
                with torch.no_grad():
                    t0 = time.time()
                    if steps > 0:
                        out = model.invert(x, steps=steps, lr=lr, streams=streams, lpips_weight=lpips_weight, lpips_state=lpips_state,
                                           loss_region=region, ssim_weight=ssim_weight, pixel_loss=pixel_loss, pixel_scale=pixel_scale, lpips_size=lpips_size, pixel_size=pixel_size,
                                           pixel_filter=pixel_filter, pixel_target=pixel_target,
                                           noise_ids=torch.arange(c0, c0 + len(chunk), dtype=torch.int64, device='cuda'), edit=edit, **sched)[0]
                        pn_table = (getattr(model, 'last_loss_terms', None) or {}).get('pn')
                        if pn_table is not None:        # the last row of the loop's own table: no extra pass
                            pn_final += [(os.path.basename(f), v) for f, v in zip(chunk, pn_table[-1].tolist())]
                    else:
                        out = (graphed(x) if graphed is not None else model(x))[0]
                    torch.cuda.synchronize()
                    times += [(time.time() - t0) / len(chunk)] * len(chunk)
                if io == 'device':
                    metrics = postprocess_device(out, x, model.aligns, chunk, bgrs, size, save_dir, metrics, opts.get('metrics'), pool)[0]
                else:
                    metrics = postprocess_host(out, x, model.aligns, chunk, bgrs, size, save_dir, metrics, opts.get('metrics'))[0]
            done = pool.drain()                 # every file is written (or its worker's exception raised) before the summary is logged
            if metrics is not None:
                collect_host_metrics(done, metrics)
        wall = (time.time() - wall0) / max(len(files), 1)
        if not edit_final:
            model.delta_latent.data -= direction.cuda()
        mean = lambda v: float(np.mean(v)) if v else float('nan')
        summary[name] = dict(n=len(files), time=mean(times), wall=wall, psnr=mean((metrics or {}).get('psnr')),
                             ssim=mean((metrics or {}).get('ssim')))
        log.info('Average process time of %s: %f', name, summary[name]['time'])
        log.info('Average wall time per image of %s (files in to files out): %f', name, summary[name]['wall'])
        log.info('Average PSNR of %s: %f', name, summary[name]['psnr'])
        log.info('Average SSIM of %s: %f', name, summary[name]['ssim'])
        if pn_final:
            summary[name]['pn'] = dict(pn_final)
            for f, v in pn_final:
                log.info('Final P_N+ distance of %s/%s: %f', name, f, v)
        for skipped in ('lpips', 'identity'):
            if (opts.get('metrics') or {}).get(skipped):
                log.info('%s of %s: skipped (third-party weights not available in this build)', skipped.upper(), name)
    return summary


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--opt', default=None, required=True, help='the testing option file path')
    ap.add_argument('--wplus-steps', type=int, default=None, help='W+ refinement steps per image (default: inversion.wplus_steps or 0)')
    args = ap.parse_args(argv)
    logging.basicConfig(level=logging.INFO, format='%(asctime)s - %(name)s - %(levelname)s - %(message)s')
    with open(args.opt) as f:
        opts = yaml.load(f, Loader=yaml.FullLoader)
    return run(opts, args.wplus_steps)


if __name__ == '__main__':
    main()
