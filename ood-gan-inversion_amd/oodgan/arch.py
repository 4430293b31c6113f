"""``ood_faceGAN_e4e`` — the drop-in top level of the path (reference
src/archs/OOD_faceGAN_e4e_arch.py:28-347): same constructor surface (the ``network_g`` block of
options/test/E4E_Face_test.yml), ``forward(x, **kw) -> (out, lats)``, side channels ``.aligns``,
``.delta_latent``, ``.avg_latent``, ``.generator.size``, ``random_gen``; plus the build-defined W+
refinement (``invert``) that the north star adds in front of the OOD forward.

The e4e encoder (the step *before* the path) is pluggable: ``self.encoder`` is any
callable ``encoder(x256, return_feats=True) -> (lats (B,18,512), feats[>=4])``; alternatively the
encoder outputs can be passed to ``forward`` as ``enc_lats=`` / ``enc_feats=``."""
import math
import os

import numpy as np
import torch
from torch import nn

from . import ops, samm
from .engine import WPlusInverter, check_latent_controls, check_style_space, check_lpips_size, check_noise_seed, check_pixel_filter, check_pixel_loss, check_pixel_size, check_pixel_target, check_nonneg, check_feature_offset, check_feature_layer, check_pn_options, check_mask_fit, check_mask_init, mask_logits, refuse_mask_fit, check_align, check_align_init, refuse_align, check_color, check_color_init, refuse_color
from .modules import Generator
from .synth import generator_channels


class Registry:
    """name -> class registry, the plugin mechanism of BasicSR (basicsr/utils/registry.py:30-66)."""

    def __init__(self, name):
        self._name, self._obj_map = name, {}

    def register(self, obj=None):
        def deco(o):
            assert o.__name__ not in self._obj_map, f'{o.__name__} already registered in {self._name}'
            self._obj_map[o.__name__] = o
            return o
        return deco if obj is None else deco(obj)

    def get(self, name):
        if name not in self._obj_map:
            raise KeyError(f"No object named '{name}' found in '{self._name}' registry!")
        return self._obj_map[name]

    def __contains__(self, name):
        return name in self._obj_map

    def keys(self):
        return self._obj_map.keys()


ARCH_REGISTRY = Registry('arch')


def build_network(opt):
    """basicsr.archs.build_network (BasicSR/basicsr/archs/__init__.py:19-25): pops ``type``."""
    opt = dict(opt)
    return ARCH_REGISTRY.get(opt.pop('type'))(**opt)


class _MissingEncoder(nn.Module):
    channels = [64, 64, 128, 256, 512]
    progressive_stage = None

    def forward(self, x, return_feats=False):
        raise RuntimeError('no e4e encoder attached: pass enc_lats=/enc_feats= to forward(), or assign a callable '
                           'to model.encoder (the encoder is the step before the accelerated path, SURVEY.md §8f N1)')


@ARCH_REGISTRY.register()
class ood_faceGAN_e4e(nn.Module):
    def __init__(self,
                 out_size=1024, style_dim=512, n_mlp=8, channel_multiplier=2, narrow=1, merge='',
                 StyleGAN_pth=None, StyleGAN_pth_key='params_ema',
                 aug_alignment=False, aug_inputcolor=False,
                 stage='Inference', encoder='E4E', E4E_pth=None, avg_latent_pth=None,
                 optim_delta_latent=False, delta_latent_pth=None,
                 enable_modulation=True, modulation_type='NOISE', warp_scale=0.02,
                 blend_with_gen=True, ModSize=None,
                 progressiveModSize=[16, 32, 64, 128, 256], progressiveStart=20000,
                 progressiveStep=2000, progressiveStageSteps=[999999999], eval_path_length=None,
                 **kwargs):
        super().__init__()
        if aug_alignment or aug_inputcolor:
            # the reference reads undefined names for these options (OOD_faceGAN_e4e_arch.py:88-97 -> NameError)
            raise NotImplementedError('aug_alignment / aug_inputcolor are unusable in the reference as well')
        if encoder != 'E4E':
            raise NotImplementedError("only encoder='E4E' is on the accelerated path")
        if modulation_type != 'NOISE':
            raise NotImplementedError("only modulation_type='NOISE' (every shipped YAML)")
        if narrow != 1:
            raise NotImplementedError('narrow != 1')
        self.encoder_type = encoder
        log_outsize = int(math.log(out_size, 2))
        self.style_cnt = log_outsize * 2 - 2
        self.style_dim = style_dim
        self.channels = generator_channels(channel_multiplier, narrow)
        if kwargs.get('build_encoder', True):
            from .encoder import ProgressiveStage
            from .encoder_hip import Encoder4EditingHIP as Encoder4Editing     # the e4e encoder on the HIP kernels
            self.encoder = Encoder4Editing(num_layers=50, mode='ir_se', opts={'stylegan_size': out_size}, bn=True)
            self.encoder.progressive_stage = ProgressiveStage[stage]
        else:
            self.encoder = _MissingEncoder()   # encoder outputs are then passed to forward() as enc_lats / enc_feats
        self.aligns = {}
        self.log_outsize = int(math.log(256, 2))
        self.stage = stage
        if enable_modulation:
            self.feats_conv = nn.ModuleList()
            featsize = 256
            for i in range(4):
                self.feats_conv.append(nn.Conv2d(_MissingEncoder.channels[i], self.channels[featsize], 1, 1, 0))
                featsize //= 2
            self.modulation = nn.ModuleList()
            self.progressiveModSize = list(progressiveModSize)
            self.modulation_type = modulation_type
            self.blend_with_gen = blend_with_gen
            self.blend_cnt = kwargs.get('blend_cnt', 1)
            self.skip_SA = kwargs.get('skip_SA', False)
            self.randomTransform = None
            self.colorTransform = None
            self.ModSize = self.progressiveModSize.pop(0) if ModSize is None else ModSize
            self.warp_scale = warp_scale
            self.cycle_align = kwargs.get('cycle_align', 1)
            for i in range(self.log_outsize, 4, -1):
                chn = self.channels[2 ** i]
                chn_mul = 2 if modulation_type == 'SFT' else 1      # reference :110-112 (only matters with a mod_btn extractor)
                self.modulation.append(samm.StyledscaleNshfitBlock(chn, chn * chn_mul, style_dim, scale=warp_scale,
                                                                   btn=kwargs.get('mod_btn', None),
                                                                   cycle_align=self.cycle_align,
                                                                   diff_fAndg=kwargs.get('diff_fAndg', True)))
        else:
            self.modulation = None
            self.ModSize = 0
        self.generator = Generator(size=out_size, n_mlp=n_mlp, style_dim=style_dim, channel_multiplier=channel_multiplier)
        self.avg_latent = nn.Parameter(torch.zeros((1, style_dim)), requires_grad=False)
        if optim_delta_latent:
            self.delta_latent = nn.Parameter(torch.randn((1, self.style_cnt, style_dim)) * 0.1, requires_grad=True)
        else:
            self.delta_latent = nn.Parameter(torch.zeros((1, self.style_cnt, style_dim)), requires_grad=False)
        self.progressiveStageSteps = progressiveStageSteps
        if self.progressiveStageSteps is None:
            self.progressiveStageSteps = [progressiveStart + progressiveStep * i for i in range(self.style_cnt)]
        if StyleGAN_pth is not None:
            from .io import load_generator_checkpoint
            load_generator_checkpoint(self.generator, StyleGAN_pth, StyleGAN_pth_key)
        if E4E_pth is not None:
            from collections import OrderedDict
            enc_ckpt = torch.load(E4E_pth, map_location='cpu')
            enc_dict = OrderedDict((k[len('encoder.'):], v) for k, v in enc_ckpt['state_dict'].items() if k.startswith('encoder.'))
            self.encoder.load_state_dict(enc_dict, strict=True)
        if avg_latent_pth is not None:
            self.avg_latent.data = torch.load(avg_latent_pth, map_location='cpu')
        if delta_latent_pth is not None:
            self.delta_latent.data = torch.load(delta_latent_pth, map_location='cpu')
        self.eval_path_length = bool(eval_path_length) if eval_path_length is not None else False

    # ---------------------------------------------------------------- reference helpers
    def get_style_mlp(self, x):
        return self.generator.style(x)

    def random_gen(self, batch_size=1, gen=True):
        style = torch.randn((batch_size, self.style_dim), device=self.avg_latent.device)
        lats = self.get_style_mlp(style).unsqueeze(1).repeat(1, self.style_cnt, 1)
        out = self.generator(lats, input_is_tensor=True, input_is_latent=True)[0] if gen else None
        return out, lats

    def random_gen_center(self, scale=0.1, gen=True):
        lats = self.avg_latent + (torch.randn_like(self.avg_latent) * scale)
        lats = lats.unsqueeze(1).repeat(1, self.style_cnt, 1)
        out = self.generator(lats, input_is_tensor=True, input_is_latent=True)[0] if gen else None
        return out, lats

    def feats2condition(self, feats, **kwargs):
        conditions = []
        if self.ModSize > 0:
            max_size = int(np.floor(math.log(self.ModSize, 2)))
            min_size = int(np.floor(math.log(feats[-1].shape[-1], 2)))
            cond_len = min(max((1 + max_size - min_size), 0), len(feats))
            conditions = [[None, None] for _ in range(cond_len)]
        return conditions

    def _cond_hook(self, k, raw, style, noise, noise_weight):
        """feats2condition_callback (OOD_faceGAN_e4e_arch.py:224-242) in its algebraically reduced
        form: the layer becomes aligned_target + w*noise (model.py:292), so the aligned feature
        itself is returned and the engine adds noise/bias/activation."""
        ind = k + 1
        feat = self.feats[-ind]
        mod = self.modulation[-ind]
        aligned = self.aligns[ind - 1] if ind > 1 else None
        cond, align = mod(feat, style, image=raw, aligned=aligned)
        self.aligns[ind] = align
        return cond

    def encode(self, x, **kwargs):
        """Step 1-2 of forward (:256-267): encoder at 256², + avg_latent + delta_latent (+ truncation)."""
        enc_lats, enc_feats = kwargs.get('enc_lats', None), kwargs.get('enc_feats', None)
        if enc_lats is None or (self.modulation is not None and enc_feats is None):
            x256 = samm.resize_bilinear(x, 256)
            with torch.no_grad():
                if self.encoder.training:       # the reference calls eval() on every forward (:257): 1 ms of host time per call over 529 modules
                    self.encoder.eval()
                enc_lats, enc_feats = self.encoder(x256, return_feats=True)
        lats = enc_lats + self.avg_latent.reshape(1, 1, -1) + self.delta_latent
        truncation = kwargs.get('truncation', 1.0)
        if truncation < 1.0:
            lats = self.avg_latent.reshape(1, 1, -1) * (1. - truncation) + (lats * truncation)
        return lats.contiguous(), enc_feats

    def forward(self, x, **kwargs):
        if kwargs.get('random_gen', False):
            return self.random_gen(batch_size=kwargs.get('batch_size', 1), gen=kwargs.get('gen', True))
        lats, enc_feats = self.encode(x, **kwargs)
        if kwargs.get('lats', None) is not None:                 # W+ refined latents replace the encoder's
            lats = kwargs['lats']
        return self._ood_forward(x, lats, enc_feats, **{k: v for k, v in kwargs.items() if k not in ('lats', 'enc_lats', 'enc_feats')})

    def _ood_forward(self, x, lats, enc_feats, **kwargs):
        """generate() of the reference (e4e :268-313 / restyle :246-283): feats_conv -> hooked generator -> mask blend."""
        self.ori_lats = lats
        noise = kwargs.get('noise', None)
        offs = kwargs.get('style_offsets', None)        # StyleSpace offsets (B, R) on the generator's styles; the hooks read ``lats``
        # feature offset (B, C, h, h) on the input of latent ``feature_layer``'s up-conv; a SAMM hook on that latent
        # receives the raw up-conv output as ever, which now includes the offset's effect
        fo = dict(feature_offset=kwargs.get('feature_offset', None), feature_layer=kwargs.get('feature_layer', None))
        # fitted colour map theta (B,12) = (M, b): the generator image is mapped once, C(G) = M G + b, before the blend — the
        # output alpha x + (1 - alpha) C(G) is in the photograph's colours, without a tint seam where the mask switches
        color = kwargs.get('color', None)
        if self.modulation is None:
            out, _ = self.generator(lats, input_is_tensor=True, input_is_latent=True, noise=noise, style_offsets=offs, **fo)
            return (out if color is None else ops.color_apply(out.contiguous(), color)), lats
        out = self._hooked_generate(lats, enc_feats, noise, offs, **fo)
        if self.blend_with_gen and self.skip_SA:
            out, _ = self.generator(lats, input_is_tensor=True, input_is_latent=True, noise=noise, style_offsets=offs, **fo)
        if color is not None:
            out = ops.color_apply(out.contiguous(), color)
        if self.blend_with_gen:
            for _ in range(self.blend_cnt):
                out = self.blend(x, out, alpha_scale=None)
        return out, lats

    def _hooked_generate(self, lats, enc_feats, noise, style_offsets=None, feature_offset=None, feature_layer=None):
        """The generator pass with the SAMM hooks (e4e :268-297): fills ``self.aligns`` with the per-level fields; returns G's image."""
        self.feats = [samm.conv1x1(enc_feats[i], self.feats_conv[i].weight, self.feats_conv[i].bias) for i in range(4)]
        self.lats = lats
        self.aligns = {}
        conditions = self.feats2condition(self.feats)
        cond_ind = [(2 * (k + 2)) + 1 for k in range(len(conditions))]
        out, _ = self.generator(lats, input_is_tensor=True, input_is_latent=True, conditions=conditions,
                                cond_layers=cond_ind, cond_type=self.modulation_type, cond_hook=self._cond_hook,
                                noise=noise, style_offsets=style_offsets, feature_offset=feature_offset, feature_layer=feature_layer)
        return out

    def blending_mask(self):
        """:315-339 — compose the up-sampled alpha channels (coarse -> fine), clip; stores aligns[size]."""
        self.aligns.pop(self.generator.size, None)
        keys = sorted(self.aligns.keys())
        if not keys:
            return None
        alpha, _ = samm.mask_blend([self.aligns[k] for k in keys], size=self.generator.size)
        self.aligns[self.generator.size] = alpha.repeat(1, 3, 1, 1)
        return alpha

    def blend(self, target, output, detach=True, alpha_scale=None):
        """:341-347; with alpha_scale=None the mask is composed and applied in one fused kernel."""
        if alpha_scale is not None:
            return alpha_scale * target + output * (1 - alpha_scale)
        self.aligns.pop(self.generator.size, None)
        keys = sorted(self.aligns.keys())
        if not keys:
            return None
        alpha, out = samm.mask_blend([self.aligns[k] for k in keys], target, output, size=self.generator.size)
        self.aligns[self.generator.size] = alpha.repeat(1, 3, 1, 1)
        return out

    # ---------------------------------------------------------------- build-defined: W+ refinement
    def invert(self, x, steps=100, lr=0.01, noise=None, streams=1, use_graph=False, lpips_weight=0.0, lpips_state=None, loss_region='full',
               ssim_weight=0.0, lr_rampup=0.0, lr_rampdown=0.0, latent_noise=0.0, noise_ramp=0.75, noise_seed=0, noise_ids=None, latent_reg=0.0,
               latent_anchor='start', pixel_loss='mse', pixel_scale=0.1, lpips_size=None, edit=None, latent_space='w+', layer_lr=None,
               delta_reg=0.0, style_reg=0.0, pixel_size=None, feature_layer=None, feature_lr=None, feature_reg=0.0, pn_reg=0.0,
               pn_samples=100000, pn_seed=0, pn_floor=0.0, pn_stats=None, pixel_filter=None, pixel_target=None, mask_size=64, mask_lr=0.1,
               mask_area=0.30, mask_area_weight=5.0, mask_binary_weight=0.2, mask_init=0.88, fit_blend=False, align=None, align_lr=0.001,
               align_reg=0.0, align_init=None, color=None, color_lr=0.002, color_reg=0.0, color_init=None, **kwargs):
        """Optimisation-based inversion: w0 = encoder latents (+avg+delta), ``steps``
        Adam steps on per-image MSE with fixed noise, then ONE full OOD forward with the refined
        latents (masks + blend).  Returns (out, lats, losses[steps,B]).  ``lpips_weight`` > 0 adds that multiple of LPIPS(alex) per image to the
        loss (opt-in; ``losses`` is then the total, ``self.last_loss_terms`` holds the tables).
        ``ssim_weight`` > 0 adds that multiple of 1 - SSIM per image: the SSIM the CLI reports (BasicSR's calculate_ssim, 11-tap
        Gaussian window, per channel) on the unrounded images — on the composite where ``loss_region`` selects one; ``last_loss_terms['ssim']`` is
        its table (None when off).  A negative or non-finite weight raises ValueError.
        ``streams`` (opt-in; ``bench.py`` uses 2, the CLI's ``inversion.streams`` sets it): the W+ loop advances the batch as
        that many independent sub-batches on concurrent HIP streams (images are independent; the HBM-bound layout
        kernels of one sub-batch run beside the matrix kernels of the other: +4 % at batch 8).  The
        default 1 keeps every kernel alone on the GPU: concurrent queues are only exact for kernels built without
        packed-fp32 instructions (this library's are; a caller's own torch-ROCm work on another stream is not covered).
        Results are bit-reproducible run to run for a given (batch, streams); they are NOT bit-invariant under the
        stream count or an image's position in the batch — kernel selection follows the sub-batch geometry (8-wave
        kernels from 128 work items) and every sub-batch carries its own range scales — the difference is fp32
        rounding on the first step (loss within 1e-5 relative) and Adam's sign choice for ~0 gradient coordinates afterwards
        (0.003 % of the coordinates, losses within 1e-3 relative after three steps: ``tests/test_hip_generator.py``).
        ``loss_region``: where the W+ loss looks.  'full' (default): every pixel, the plain per-image MSE.  'blend': the
        composite x + beta*(G(w) - x) with beta = (1 - alpha0)^blend_cnt, alpha0 the mask of the OOD forward at the start latents with the
        same ``noise`` — the error of the blended output this method returns, with the mask frozen for the run.  A float32 (B,1,S,S) tensor
        in [0,1] on the model's device: that beta (a caller mask: 0 = ignore the pixel).  ``self.last_loss_weight`` is the beta optimised
        (None for 'full').
        Projector schedule (rosinality's projector.py), all off by default.  ``lr_rampup`` / ``lr_rampdown`` (the projector's
        0.05 / 0.25): fractions of the run over which the learning rate ramps up linearly and follows a cosine down.  ``latent_noise`` (its
        ``--noise``, 0.05): Gaussian noise on the latent the generator reads, of strength latent_noise * ``generator.latent_std()`` *
        max(0, 1 - (t / steps) / noise_ramp)^2; the draws depend on (``noise_seed``, the image's entry of ``noise_ids`` — int64 (B,), default
        arange(B) —, step, element) only, not on the batch or the streams.  ``latent_reg`` > 0 adds latent_reg * mean (w - anchor)^2 per image
        with ``latent_anchor`` = 'start' (the start latents of the run), 'mean' (avg_latent + delta_latent) or a (L,512) / (B,L,512) tensor;
        ``last_loss_terms['latent']`` is its table (None when off).  Negative or non-finite values raise ValueError.
        ``pixel_loss``: the pixel term, the per-image mean of rho(d) over the residual d = G - x (beta*(G - x) where ``loss_region``
        selects a composite).  'mse' (default): d^2, the path above unchanged.  Robust kinds, for occluders nobody masked, with the scale
        s = ``pixel_scale`` in image units: 'charbonnier' sqrt(d^2 + s^2) (BasicSR's CharbonnierLoss with eps = s^2), 'huber' d^2/2 up to
        |d| = s and s(|d| - s/2) beyond (a very large s is half the MSE), 'geman_mcclure' d^2/2 * s^2/(d^2 + s^2), whose pull on the latent
        goes to zero for an outlier.  The default s = 0.1 is a tenth of the image half-range, about 13 grey levels: a choice, not a measured
        optimum.  ``last_loss_terms['pixel']`` is the term's table whatever its kind; ``['mse']`` is that table for 'mse' and None otherwise.
        An unknown name, or a scale that is not a finite number > 0, raises ValueError; ``use_graph`` with a robust kind NotImplementedError.
        ``lpips_size``: the size the LPIPS term is taken at.  None (default): the image's own, the path above unchanged.  An int:
        the image (the composite where ``loss_region`` selects one) and the target are area-pooled to lpips_size x lpips_size first — mean
        over f x f windows, f = size / lpips_size in {1, 2, 4, 8, 16} — and the term's gradient comes back through the pool's adjoint; the pixel
        and SSIM terms stay at full resolution.  256 is the projectors' value (rosinality's projector.py and the StyleGAN2-ADA projector pool
        to 256² before LPIPS): AlexNet's fields then cover facial structure, and the term costs a fraction of its full-resolution time.
        A value that is not an int, is below 64, or does not divide the image size by one of those factors raises ValueError.
        ``pixel_size``: the size the pixel term is taken at.  None (default) or the image's own size: the path above unchanged.
        An int: the term is the mean of rho over the residual of the area-pooled views, P(G) - P(x) (with ``loss_region``: P(beta*(G - x)), the
        pooled composite minus the pooled target), f = size / pixel_size in {2, 4, 8, 16}; every pixel of a window receives its window's
        gradient, at the magnitude of the full-resolution term.  One fused kernel, no more launches per step.  With ``lpips_size`` of the same
        value both terms see one view (256: the projectors' horizon), and detail the generator cannot produce — hair strands, sensor noise, JPEG
        blocks — stops pulling the latent.  A low-resolution photograph is inverted by passing it nearest-upsampled to the generator's size with
        ``pixel_size`` = its own size: the area pool of a nearest-upsampled image is the image itself, so the term compares pool(G) with exactly
        the pixels there are, while the encoder and the OOD forward keep their full-size input.  A value that is not an int or does not divide the
        image size by one of those factors raises ValueError; ``use_graph`` with it NotImplementedError.
        ``edit``: an editing direction applied AFTER the fit — a float32 (L,512), (1,L,512) or (B,L,512) tensor on the model's
        device.  The loop runs exactly as without it (the same ``losses``, the same refined latents w); the final OOD forward is taken at w + edit
        and the returned ``lats`` are those latents, the ones the output was generated from.  ``self.last_refined_lats`` holds w after every call,
        with an edit or without.  (A direction in ``delta_latent`` is part of the START latents instead: the loop then fits the unedited input
        from an edited start and works the edit off again.)  A wrong shape, dtype or device raises ValueError.
        Latent controls of the loop, off by default.  ``latent_space``: 'w+' (every layer its own vector) or 'w': one vector
        per image, started at the layer mean of the start latents and kept on every layer — the most editable, least faithful end of e4e's
        editability-distortion trade-off; the latent noise is then one vector repeated over the layers.  ``layer_lr``: L finite factors >= 0 of
        ``lr``, one per layer; 0 freezes a layer (e.g. fit the coarse layers only).  ``delta_reg`` = lambda >= 0 adds lambda * mean_le
        (w_le - mean_l w_le)^2 per image, the squared spread of the layers about their mean — the symmetric, build-defined form (e4e's own
        regulariser measures the distance from layer 0); W is its lambda -> infinity limit.  ``last_loss_terms['delta']`` is its table (None
        when off).  'w' together with ``layer_lr`` or ``delta_reg``, a wrong length, a negative or a non-finite entry raise ValueError;
        ``use_graph`` with any of the three NotImplementedError.
        StyleSpace (Wu et al., CVPR 2021): ``latent_space='s'`` keeps the latents at their start w0 and fits an offset delta
        (B, R) on the per-channel styles the modulated convs consume, s = A(w0) + delta, from 0 — the space with the lowest reconstruction
        error of Z / W / W+ / S, and the one single-channel edits live in; ``generator.style_layout()`` names the columns.  The returned
        ``lats`` (and ``self.last_refined_lats``) are w0, ``self.last_style_offsets`` is delta (None for the other spaces), and
        ``model(x, lats=lats, style_offsets=self.last_style_offsets)`` reproduces the output; the SAMM hooks keep reading w0.  ``style_reg`` =
        lambda >= 0 adds lambda * mean_r delta_r^2 per image, a build-defined pull towards styles some w can produce
        (``last_loss_terms['style']``, None when off).  ``edit`` is then a StyleSpace direction, float32 (R,), (1,R) or (B,R), added to delta for
        the final forward only.  ``layer_lr`` scales the step of each layer's style rows.  's' with delta_reg, latent_noise or latent_reg,
        ``style_reg`` without 's', or a W+-shaped edit in 's' raise ValueError; ``use_graph`` with 's' and a zero-padded (narrow) generator
        NotImplementedError.
        Feature offset (the F/W+ family: BDInvert, Feature-Style), off by default.  ``feature_layer`` = 3, 5 or 7: beside the
        latents the loop fits an offset delta (B, C, h, h), from 0, on the 8², 16² or 32² input of the styled up-conv that reads that latent
        (5: Feature-Style's index) — content no latent can express, a hat or a hand in front of the face, has a code there.  Adam with
        ``feature_lr`` (None: ``lr``, a choice, not a measured optimum; 0 leaves the offset at zero); ``feature_reg`` = lambda >= 0 adds
        lambda * mean delta^2 per image (``last_loss_terms['feature']``, None when off).  The final OOD forward runs with the fitted offset;
        ``self.last_feature_offset`` / ``self.last_feature_layer`` hold it (None without the option) and
        ``model(x, lats=lats, feature_offset=self.last_feature_offset, feature_layer=self.last_feature_layer)`` reproduces the output.
        ``edit`` keeps its meaning.  Another index, a layer the generator's size lacks, ``feature_lr`` / ``feature_reg`` without a layer, or
        latent_space 's' raise ValueError; ``use_graph`` with it and a zero-padded (narrow) generator NotImplementedError.
        P_N+ prior (II2S, Zhu et al.: "Improved StyleGAN Embedding: Where are the Good Latents?"), off by default.  ``pn_reg`` =
        lambda >= 0 adds lambda * mean_{l,d} q^T M q per image, q = l5(w) - mu per latent row: l5(t) = t if t > 0 else 5 t undoes the mapping
        network's last LeakyReLU, and (mu, M) whiten it with the PCA of the mapping network's own outputs — the Mahalanobis distance to the
        latents the generator was trained on, the control for a fit that reconstructs well and edits badly, where ``latent_reg`` charges every
        direction of W the same.  The statistics come from ``generator.pn_stats(pn_samples, pn_seed, pn_floor)`` (cached per mapping
        weights; ``pn_floor``: the relative floor of the variances) unless ``pn_stats``, an ``oodgan.pn.PNStats``, is given: it wins over
        the three.  ``last_loss_terms['pn']`` is the term's table (None when off), ``self.last_pn_stats`` the statistics used.  A negative or
        non-finite value, latent_space 's', or statistics of another width, dtype or device raise ValueError; ``use_graph`` with it
        NotImplementedError.
        ``pixel_filter``: the filter of the ``pixel_size`` view.  None or 'box' (default): the area pool above, unchanged.
        'bilinear', 'bicubic' (Keys, a = -0.5) or 'lanczos3': the antialiased resize D that ``F.interpolate(antialias=True)``, PIL and the
        thumbnailers apply, the operator a real low-resolution photograph was made with; the term is the mean of rho over D(G) - D(x) and its
        gradient the true adjoint, two HIP kernels, one launch more per step.  ``pixel_target``: a float32 (B,3,n,n) image in [-1, 1] on the
        model's device, the low-resolution photograph at its own size: it replaces D(x) (with 'box': the pooled target) and fixes
        ``pixel_size`` = n.  ``x`` stays the full-size input of the encoder, the OOD forward and the blend, and LPIPS and SSIM, if on, keep
        comparing with ``x``.  A filter without a ``pixel_size`` below the image size, an unknown filter, a ``pixel_size`` that differs from
        the target's size, a size / n outside {2, 4, 8, 16}, or either option with ``loss_region`` other than 'full' raise ValueError;
        ``use_graph`` with them NotImplementedError.
        ``loss_region='fit'`` (the reference's MaskLoss, src/losses/mask_loss.py, is the anchor): the loop itself decides which
        region it stops fitting.  Beside the latents it fits the logits of a mask a = sigmoid(l), (B,1,m,m) with m = ``mask_size`` in
        {16, 32, 64, 128, 256} (S / m an integer >= 2); the loss is taken on the composite x + beta*(G(w) - x) with beta = the bilinear
        enlargement of a (``F.interpolate(align_corners=False)``, what ``blending_mask`` applies), refreshed every step, plus per image
        ``mask_area_weight`` * max(0, mean(1 - a) - ``mask_area``) + ``mask_binary_weight`` * mean(min(a, 1 - a)) — MaskLoss with target 1 on
        alpha = 1 - a; the defaults 0.30 / 5.0 / 0.2 are the shipped YAML's area, loss_weight and binary_weight * loss_weight.  The logits
        take Adam steps of their own at ``mask_lr`` (default 0.1) under the loop's betas, eps and ramps.  ``mask_init``: the start of a — a float
        in (0, 1) (default 0.88), 'blend' (the beta of ``loss_region='blend'`` area-pooled to m x m; needs the modulation, as 'blend' does) or
        a float32 (B,1,m,m) tensor in [0, 1] on the model's device; values are clipped to [1e-3, 1 - 1e-3] before the logit.  Afterwards
        ``self.last_fitted_mask`` is a (B,1,m,m), ``self.last_loss_weight`` its enlargement beta (B,1,S,S), and
        ``last_loss_terms['mask_area']`` / ``['mask_binary']`` the hinge and the binarisation mean per step and image (None when off).
        ``fit_blend=True`` returns ``blend(x, G(w), alpha_scale=1 - beta)`` in place of the SAMM blend — the one OOD blend a model built with
        ``enable_modulation=False`` has; False (default) leaves the returned image what it is without the option.  On a random-weight
        generator the mask goes where an occluder is (tests/test_hip_mask_fit.py); quality on real faces is unpinned for lack of
        checkpoints.  Goes with 'w+' / 'w', layer_lr, delta_reg, the schedule, pn_reg, edit, streams, the robust pixel terms, LPIPS and
        SSIM.  ``use_graph``, pixel_size, pixel_filter / pixel_target, latent_space 's', feature_layer and a zero-padded (narrow) generator
        raise NotImplementedError; a size outside the list or one that does not divide S, a negative or non-finite weight, a ``mask_lr``
        that is not a finite number > 0, an area outside [0, 1], an init outside (0, 1) or of the wrong shape, dtype or device, and
        ``fit_blend`` without 'fit' raise ValueError.
        ``align='similarity'``: the loop fits, beside the latents, a similarity theta = (log-scale, rotation in radians, tx, ty
        in units of half the image side) per image and compares G(w) with x warped by it — a photograph a few pixels or a degree off the
        generator's canonical frame is registered instead of costing the latents.  Adam with ``align_lr`` (0.001: about half a pixel per
        step at 1024²; nobody has measured it as an optimum) under the loop's betas, eps and ramps; ``align_reg`` = mu >= 0 adds
        mu * sum_k theta_k^2 per image (``last_loss_terms['align']``); ``align_init``: a float32 (B,4) start on the device, None = the
        identity.  After the loop x_a = ``ops.similarity_warp(x, theta)``: the encoder features of the final OOD forward are taken from x_a
        (on a model with modulation blocks: by the attached encoder, or by ``enc_feats`` given as a callable x_a -> features; ``enc_feats``
        given as tensors, the features of x, or neither, raises ValueError before the loop starts)
        and the forward and the blend run on x_a, so THE OUTPUT IS IN THE ALIGNED FRAME (``ops.similarity_warp(out,
        ops.similarity_inverse(theta))`` maps it back); ``self.last_alignment`` is theta (B,4), ``self.last_aligned_input`` x_a (both None
        without the option).  Goes with 'w+' / 'w', layer_lr, delta_reg, the schedule, pn_reg, edit, streams, the four pixel kinds and box
        ``pixel_size``.  ``use_graph``, LPIPS, SSIM, a ``loss_region`` other than 'full', a non-box ``pixel_filter``, ``pixel_target``,
        latent_space 's', feature_layer and a zero-padded (narrow) generator raise NotImplementedError (``engine.refuse_align``); a bad name,
        rate, weight or start raises ValueError.
        ``color='gain'`` or ``'affine'``: the loop fits, beside the latents, a colour map theta = (M row-major 3x3, b) per image
        and takes the pixel term on C(G) = M G + b — a colour cast, another exposure, faded or sepia film is explained by twelve numbers
        ('gain': six, per-channel gain and offset: white balance and exposure) instead of costing the latents identity and editability.
        Adam with ``color_lr`` (0.002: at most 0.2 of gain, or 25 grey levels of offset, over 100 steps; a choice, nobody has measured it
        as an optimum) under the loop's betas, eps and ramps; ``color_reg`` = mu >= 0 adds mu * sum_k (theta_k - id_k)^2 per image
        (``last_loss_terms['color']``); ``color_init``: a float32 (B,12) start on the device, None = the identity.  The final OOD forward maps
        the generator image once before the blend: the output is alpha x + (1 - alpha) C(G), in the photograph's colours (C(G) without
        modulation); ``self.last_color`` is theta (None without the option) and ``model(x, lats=lats, color=self.last_color)`` reproduces the
        output.  THE COLOUR-CORRECTED PICTURE is ``ops.color_apply(out, ops.color_inverse(theta))``: an affine map commutes with the blend, so
        this is the blend of C^-1(x) with G.  With ``loss_region='blend'`` alpha_0 comes from the unmapped pass at w0, as without the option.
        Goes with 'w+' / 'w', layer_lr, delta_reg, the schedule, pn_reg, edit, streams, the four pixel kinds and ``loss_region`` 'blend' or a
        tensor.  ``use_graph``, LPIPS, SSIM, ``loss_region='fit'``, align, pixel_size, pixel_filter, pixel_target, latent_space 's',
        feature_layer and a zero-padded (narrow) generator raise NotImplementedError (``engine.refuse_color``); a bad name, rate, weight or
        start raises ValueError."""
        color, color_lr, color_reg = check_color(color, color_lr, color_reg)
        if color is not None:       # every check of the option before any device work; the refusals in one place (engine.refuse_color)
            refuse_color(use_graph, bool(lpips_weight), ssim_weight != 0.0, loss_region if isinstance(loss_region, str) else 'a loss-weight tensor',
                         align, None if pixel_size == int(x.shape[-1]) else pixel_size, pixel_filter, pixel_target, latent_space, feature_layer)
            refuse_color(padded=self.generator.engine().padded)
            check_color_init(color_init, x.shape[0], x.device)
        elif color_init is not None:
            raise ValueError('color_init without color: there is no colour map it could start')
        align, align_lr, align_reg = check_align(align, align_lr, align_reg)
        feats_of = None
        if align is not None:       # every check of the option before any device work; the refusals in one place (engine.refuse_align)
            region = loss_region if isinstance(loss_region, str) else 'a loss-weight tensor'
            refuse_align(use_graph, bool(lpips_weight), ssim_weight != 0.0, region, pixel_filter, pixel_target, latent_space, feature_layer)
            refuse_align(padded=self.generator.engine().padded)
            check_align_init(align_init, x.shape[0], x.device)
            # the final OOD forward needs the encoder features of x_a, which does not exist before the loop: an attached encoder delivers
            # them, or the caller's ``enc_feats`` is a callable x_a -> features; features handed in as tensors are those of x
            if self.modulation is not None:
                ef = kwargs.get('enc_feats')
                if callable(ef):
                    feats_of = ef
                elif ef is not None:
                    raise ValueError('align with enc_feats given as tensors: they are the features of x, and the final OOD forward needs those of '
                                     'the aligned input x_a; pass enc_feats=<callable x_a -> features> or attach an encoder')
                elif isinstance(self.encoder, _MissingEncoder):
                    raise ValueError('align on a model with modulation blocks needs the encoder features of the aligned input: attach an encoder '
                                     'or pass enc_feats=<callable x_a -> features>')
        elif align_init is not None:
            raise ValueError('align_init without align: there is no alignment it could start')
        fit = isinstance(loss_region, str) and loss_region == 'fit'
        if fit:     # every check of the option before any device work; the refusals in one place (engine.refuse_mask_fit)
            mask_size, mask_lr, mask_area, mask_area_weight, mask_binary_weight = check_mask_fit(
                mask_size, mask_lr, mask_area, mask_area_weight, mask_binary_weight, int(x.shape[-1]))
            mask_init = check_mask_init(mask_init, x.shape[0], mask_size, x.device)
            if isinstance(mask_init, str) and (self.modulation is None or not self.blend_with_gen):
                raise ValueError("mask_init='blend' needs enable_modulation=True and blend_with_gen=True: without them there is no blend")
            refuse_mask_fit(use_graph, None if pixel_size == int(x.shape[-1]) else pixel_size, pixel_filter, pixel_target, latent_space,
                            feature_layer)
            refuse_mask_fit(padded=self.generator.engine().padded)
        elif fit_blend:
            raise ValueError("fit_blend needs loss_region='fit': there is no fitted mask to blend with")
        ssim_weight = check_nonneg(ssim_weight, 'ssim_weight')
        lr_rampup, lr_rampdown = check_nonneg(lr_rampup, 'lr_rampup'), check_nonneg(lr_rampdown, 'lr_rampdown')
        latent_noise, noise_ramp = check_nonneg(latent_noise, 'latent_noise'), check_nonneg(noise_ramp, 'noise_ramp')
        noise_seed, latent_reg = check_noise_seed(noise_seed), check_nonneg(latent_reg, 'latent_reg')
        pixel_loss, pixel_scale = check_pixel_loss(pixel_loss, pixel_scale)
        lpips_size = check_lpips_size(lpips_size, int(x.shape[-1]))
        pixel_size = check_pixel_size(pixel_size, int(x.shape[-1]))
        pixel_filter = check_pixel_filter(pixel_filter)
        pixel_target, pixel_size = check_pixel_target(pixel_target, x, pixel_size)
        pixel_size = check_pixel_size(pixel_size, int(x.shape[-1]), 'pixel_size' if pixel_target is None else 'the size of pixel_target')
        if pixel_filter is not None and pixel_size is None:
            raise ValueError(f'pixel_filter {pixel_filter!r} needs pixel_size (or pixel_target) below the image size')
        if (pixel_filter is not None or pixel_target is not None) and not (isinstance(loss_region, str) and loss_region == 'full'):
            raise ValueError("pixel_filter / pixel_target take loss_region='full' only: the masked objective is taken on the area-pooled view of x")
        if not isinstance(latent_anchor, torch.Tensor) and latent_anchor not in ('start', 'mean'):
            raise ValueError(f"latent_anchor must be 'start', 'mean' or a tensor, got {latent_anchor!r}")
        latent_space, layer_lr, delta_reg = check_latent_controls(latent_space, layer_lr, delta_reg, self.generator.n_latent)
        style_reg = check_style_space(latent_space, style_reg, delta_reg, latent_noise, latent_reg)
        feature_layer, feature_lr, feature_reg = check_feature_offset(feature_layer, feature_lr, feature_reg, lr, latent_space)
        check_feature_layer(feature_layer, self.generator.n_latent)
        pn_reg, pn_samples, pn_seed, pn_floor = check_pn_options(pn_reg, pn_samples, pn_seed, pn_floor, latent_space)
        sspace = latent_space == 's'
        lats0, enc_feats = self.encode(x, **kwargs)
        B = x.shape[0]
        edit = self._check_style_edit(edit, B, self.generator.engine().R, lats0.device) if sspace else self._check_edit(edit, lats0)
        if noise is None:
            noise = [n.expand(B, -1, -1, -1).contiguous() for n in self.generator.make_noise()]
        ml0 = None
        if fit:     # the start logits (set-up, not the step); the loop owns beta from here on
            if isinstance(mask_init, torch.Tensor):
                a0 = mask_init
            elif isinstance(mask_init, str):
                a0, f = self._loss_weight('blend', x, lats0, enc_feats, noise), int(x.shape[-1]) // mask_size
                while f > 1:            # the area pool takes factors up to 16: a larger one in two passes, the same means
                    a0, f = ops.area_pool(a0, min(f, 16)), f // min(f, 16)
            else:
                a0 = torch.full((B, 1, mask_size, mask_size), mask_init, device=x.device, dtype=torch.float32)
            ml0 = mask_logits(a0)
        beta = None if fit else self._loss_weight(loss_region, x, lats0, enc_feats, noise)
        self.last_loss_weight = beta
        lp = None
        if lpips_weight:
            # loss = MSE + lpips_weight * LPIPS(alex) (reference loss class: src/losses/lpips_loss.py:13-34, min_max = the generator's (-1, 1)).
            # ``lpips_state``: the lpips package's state dict; None = the seeded stand-in (weights absent here: parity unpinned)
            from .lpips import LPIPSAlex
            from .synth import lpips_state as _seeded
            key = id(lpips_state)
            if getattr(self, '_lpips_key', None) != key:
                st = lpips_state if lpips_state is not None else _seeded(0)
                self._lpips_net, self._lpips_key = LPIPSAlex({k: v.to(x.device) for k, v in st.items()}, min_max=(-1.0, 1.0)), key
            lp = self._lpips_net
        anchor = None
        if latent_reg > 0.0:
            anchor = latent_anchor
            if not isinstance(anchor, torch.Tensor):
                anchor = lats0 if anchor == 'start' else (self.avg_latent.reshape(1, -1, self.style_dim) + self.delta_latent)[0].expand(lats0.shape[1:])
            anchor = anchor.detach().float().contiguous()
        sigma0 = latent_noise * self.generator.latent_std() if latent_noise > 0.0 else 0.0
        if pn_reg > 0.0 and pn_stats is None:
            pn_stats = self.generator.pn_stats(pn_samples, pn_seed, pn_floor)
        self.last_pn_stats = pn_stats if pn_reg > 0.0 else None
        inv = WPlusInverter(self.generator.engine(), lr=lr, lpips=lp, lpips_weight=lpips_weight, ssim_weight=ssim_weight, lr_rampup=lr_rampup,
                            lr_rampdown=lr_rampdown, latent_noise=sigma0, noise_ramp=noise_ramp, noise_seed=noise_seed, latent_reg=latent_reg,
                            pixel_loss=pixel_loss, pixel_scale=pixel_scale, lpips_size=lpips_size, latent_space=latent_space, layer_lr=layer_lr,
                            delta_reg=delta_reg, style_reg=style_reg, pixel_size=pixel_size, feature_layer=feature_layer, feature_lr=feature_lr,
                            feature_reg=feature_reg, pn_reg=pn_reg, pixel_filter=pixel_filter, mask_size=mask_size if fit else None,
                            mask_lr=mask_lr, mask_area=mask_area, mask_area_weight=mask_area_weight, mask_binary_weight=mask_binary_weight, align=align, align_lr=align_lr, align_reg=align_reg,
                            color=color, color_lr=color_lr, color_reg=color_reg)
        w, losses = inv.invert(x, lats0, noise, steps=steps, streams=streams, use_graph=use_graph, loss_weight=beta, noise_ids=noise_ids,
                               latent_anchor=anchor, pn_stats=pn_stats, pixel_target=pixel_target, mask_logits=ml0, align_init=align_init, color_init=color_init)
        self.last_fitted_mask = inv.last_fitted_mask
        self.last_alignment, self.last_aligned_input = inv.last_alignment, inv.last_aligned_target
        self.last_color = inv.last_color
        if align is not None:       # the output is made in the aligned frame: the encoder features, the forward and the blend see x_a
            x = self.last_aligned_input
            if feats_of is not None:
                enc_feats = feats_of(x)
            elif self.modulation is not None:
                _, enc_feats = self.encode(x, **{k: v for k, v in kwargs.items() if k not in ('enc_lats', 'enc_feats')})
        if fit:
            self.last_loss_weight = inv.last_loss_weight
        self.last_loss_terms, self.last_invert_stats, self.last_invert_plan = inv.last_terms, inv.last_stats, inv.last_plan
        kw = {k: v for k, v in kwargs.items() if k not in ('noise_passes', 'truncation', 'enc_lats', 'enc_feats', 'lats', 'noise', 'style_offsets',
                                                           'feature_offset', 'color')}
        if self.last_color is not None:
            kw.update(color=self.last_color)
        self.last_feature_offset, self.last_feature_layer = inv.last_feature_offset, (feature_layer if inv.last_feature_offset is not None else None)
        if self.last_feature_offset is not None:
            kw.update(feature_offset=self.last_feature_offset, feature_layer=feature_layer)
        if sspace:          # w is the offset on the styles; the latents are the start's
            self.last_refined_lats, self.last_style_offsets = lats0, w
            out, lats = self._ood_forward(x, lats0, enc_feats, noise=noise, style_offsets=w if edit is None else (w + edit).contiguous(), **kw)
        elif fit and fit_blend:     # the fitted mask's own blend in place of the SAMM blend: no hooks, so also without the modulation
            self.last_refined_lats, self.last_style_offsets = w, None
            lats = w if edit is None else (w + edit).contiguous()
            self.ori_lats = lats
            gen, _ = self.generator(lats, input_is_tensor=True, input_is_latent=True, noise=noise)
            out = self.blend(x, gen, alpha_scale=1.0 - self.last_loss_weight)
        else:
            self.last_refined_lats, self.last_style_offsets = w, None
            out, lats = self._ood_forward(x, w if edit is None else (w + edit).contiguous(), enc_feats, noise=noise, **kw)
        # An inversion returns finished results.  Without this the host runs ahead into the next inversion's set-up while the device still works
        # on this one: blocks this inversion's side streams freed are then not yet reusable, the caching allocator goes to the driver for new ones
        # and every inversion pays ~20 ms (measured, bench.py back-to-back inversions on one box: 1054-1061 ms without, 1036-1047 ms with it —
        # profiles/r6_invert_sync_ab.txt; until round 6 a host read of the
        # carried-scale flag in Generator.forward happened to provide this synchronisation)
        torch.cuda.current_stream().synchronize()
        return out, lats, losses

    @staticmethod
    def _check_edit(edit, lats0):
        """``invert(edit=...)``: None, or a float32 (L,512) / (1,L,512) / (B,L,512) tensor on the latents' device (ValueError otherwise)."""
        if edit is None:
            return None
        B, L, D = lats0.shape
        if (not isinstance(edit, torch.Tensor) or tuple(edit.shape) not in ((L, D), (1, L, D), (B, L, D)) or edit.dtype != torch.float32
                or edit.device != lats0.device):
            got = f'{edit.dtype} {tuple(edit.shape)} on {edit.device}' if isinstance(edit, torch.Tensor) else repr(edit)
            raise ValueError(f'edit must be a float32 {(L, D)}, {(1, L, D)} or {(B, L, D)} tensor on {lats0.device}, got {got}')
        return edit.detach()

    @staticmethod
    def _check_style_edit(edit, B, R, device):
        """``invert(latent_space='s', edit=...)``: None, or a float32 (R,) / (1,R) / (B,R) StyleSpace direction on the device (ValueError otherwise)."""
        if edit is None:
            return None
        if (not isinstance(edit, torch.Tensor) or tuple(edit.shape) not in ((R,), (1, R), (B, R)) or edit.dtype != torch.float32
                or edit.device != device):
            got = f'{edit.dtype} {tuple(edit.shape)} on {edit.device}' if isinstance(edit, torch.Tensor) else repr(edit)
            raise ValueError(f"edit with latent_space 's' must be a float32 {(R,)}, {(1, R)} or {(B, R)} StyleSpace direction on {device}, got {got}")
        return edit.detach()

    def _loss_weight(self, loss_region, x, lats0, enc_feats, noise):
        """beta of ``invert(loss_region=...)``: None for 'full'; for 'blend' the mask of one hooked generator pass at the start latents
        (blending_mask, then oodgan_loss_weight_from_alpha); a tensor is checked and returned."""
        S = self.generator.size
        if isinstance(loss_region, torch.Tensor):
            beta = loss_region
            if tuple(beta.shape) != (x.shape[0], 1, S, S) or beta.dtype != torch.float32 or beta.device != x.device:
                raise ValueError(f'loss_region tensor must be float32 of shape {(x.shape[0], 1, S, S)} on {x.device}, got '
                                 f'{beta.dtype} {tuple(beta.shape)} on {beta.device}')
            lo, hi = torch.aminmax(beta)
            if not (lo.item() >= 0.0 and hi.item() <= 1.0):         # NaN fails both
                raise ValueError(f'loss_region tensor values must lie in [0, 1], got [{lo.item()}, {hi.item()}]')
            return beta.contiguous()
        if loss_region == 'full':
            return None
        if loss_region != 'blend':
            raise ValueError(f"loss_region must be 'full', 'blend' or a (B,1,S,S) tensor, got {loss_region!r}")
        if self.modulation is None or not self.blend_with_gen:
            raise ValueError("loss_region='blend' needs enable_modulation=True and blend_with_gen=True: without them there is no blend")
        # alpha0 is frozen for the run: refreshing it would need the OOD forward (which shares the engine's carried range state) between
        # recorded steps.  The W+ loop resets that state before its first step, so this pass leaves nothing behind for it
        self._hooked_generate(lats0, enc_feats, noise)
        alpha = self.blending_mask()
        return ops.loss_weight_from_alpha(alpha, self.blend_cnt)


class GraphedForward:
    """``model(x)`` replayed from a captured hipGraph — for the single-image latency the reference's CLI reports ("Average process
    time", run_ood_faceGAN_inversion.py:167-172,187): at B = 1 the forward is ~800 launches of 5-250 us and the host call overhead and
    the gaps between dependent launches are ~6 % of the 15 ms (at B = 8 nothing).  One graph per input shape, captured on first use
    after two eager warm-up calls; ``noise=`` (the 17 generator maps) is copied into static buffers, otherwise every replay draws
    fresh noise (PyTorch registers its generator with the graph).  Returned tensors and ``model.aligns`` are the graph's static
    buffers: they are overwritten by the next call.  Call ``reset()`` after changing any weight (packed copies are part of the graph).
    Works for the three variants (their forwards make no host-side decisions on tensor values)."""

    def __init__(self, model):
        self.model, self._cache, self._side = model, {}, None

    def reset(self):
        """Drop the captured graphs (and, with them, their private pools); the scratch buffers the library-side pools keep per
        stream handle (ops.sform_scratch / conv_workspace) are released too — they were created for this object's side stream."""
        self._cache = {}
        if self._side is not None:
            from . import ops
            ops.drop_stream_scratch(self._side.cuda_stream)

    @torch.no_grad()
    def __call__(self, x, noise=None):
        key = (tuple(x.shape), noise is not None)
        ent = self._cache.get(key)
        if ent is None:
            sx = x.clone()
            sn = None if noise is None else [n.clone() for n in noise]
            # ONE side stream per object, used for the warm-up AND the capture: the S-form scratch buffers and conv workspaces are
            # keyed by the stream handle (ops.sform_scratch), so the buffers the warm-up creates are the ones the captured launches
            # use — nothing is allocated (or zero-filled) inside the graph, and nothing is left behind under another handle
            if self._side is None:
                self._side = torch.cuda.Stream(device=x.device)
            side = self._side
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                for _ in range(2):                  # packs weights, fills the memo caches, grows the allocator pools
                    self.model(sx, noise=sn) if sn is not None else self.model(sx)
            torch.cuda.current_stream().wait_stream(side)
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, stream=side):
                out, lats = self.model(sx, noise=sn) if sn is not None else self.model(sx)
            gen = getattr(self.model, 'generator', None)
            eng = getattr(gen, '_engine_obj', None) if gen is not None else None
            # the range state THIS graph's launches read and write (one per batch size, engine._range): the check after a replay must look
            # at this object, not at whatever batch size ran last
            ent = self._cache[key] = dict(graph=graph, x=sx, noise=sn, out=out, lats=lats, aligns=dict(self.model.aligns),
                                          rng=getattr(eng, 'fwd_range', None))
        ent['x'].copy_(x)
        if noise is not None:
            for d, n in zip(ent['noise'], noise):
                d.copy_(n)
        ent['graph'].replay()
        # the captured forward runs on carried range scales (modules.Generator.forward) and cannot read their check flag inside the graph:
        # read it here (one small device-to-host copy) and repeat the call eagerly with measured scales if it is set
        gen = getattr(self.model, 'generator', None)
        eng = gen._engine_obj if gen is not None and getattr(gen, '_engine_obj', None) is not None else None
        rng = ent.get('rng')
        if eng is not None and rng is not None and rng.violated():
            eng.reset_fwd_state(rng.B)
            out, lats = self.model(x, noise=noise) if noise is not None else self.model(x)
            return out, lats
        self.model.aligns = dict(ent['aligns'])
        return ent['out'], ent['lats']


@ARCH_REGISTRY.register()
class ood_faceGAN_restyle(ood_faceGAN_e4e):
    """The ReStyle variant (reference src/archs/OOD_faceGAN_restyle_arch.py:29-375): the latent code is
    predicted iteratively — ``enc_cycle`` passes of a 6-channel encoder over [pool256(x), pool256(current reconstruction)],
    starting from the average image — and the OOD forward (SAMM hooks, mask, blend) then runs exactly as in
    ``ood_faceGAN_e4e``.  Same constructor surface, ``forward(x, **kw) -> (out, lats)`` and side channels.

    ``ReStyle_pth``: a checkpoint with ``state_dict`` (``encoder.*`` keys), ``latent_avg`` (style_cnt, style_dim) and
    ``opts`` (``encoder_type``, ``input_nc``), as the reference loads it (:67-83).  Only ``ProgressiveBackboneEncoder``
    is supported (the ResNet-34 variant needs torchvision).

    The reference draws fresh noise in every generator pass (it never forwards ``noise=``).  For reproducible runs
    ``forward`` takes ``noise_passes=[avg-image pass (batch 1), cycle pass 1, ..., final pass]``, each a list of the 17
    per-layer maps; ``noise=`` sets the final pass only."""

    def __init__(self, out_size=1024, style_dim=512, encoder='ReStyle', ReStyle_pth=None, enc_cycle=2, avg_latent_pth=None, **kwargs):
        if encoder != 'ReStyle':
            raise NotImplementedError("ood_faceGAN_restyle: encoder must be 'ReStyle'")
        if ReStyle_pth is None:
            raise AssertionError('ReStyle_pth is required (reference :66)')
        stage = kwargs.pop('stage', 'Inference')
        kwargs.pop('build_encoder', None)
        kwargs.pop('E4E_pth', None)
        super().__init__(out_size=out_size, style_dim=style_dim, encoder='E4E', stage=stage, build_encoder=False, **kwargs)
        self.encoder_type = encoder
        from collections import OrderedDict
        from .encoder import ProgressiveStage
        enc_ckpt = torch.load(ReStyle_pth, map_location='cpu') if isinstance(ReStyle_pth, (str, bytes)) or hasattr(ReStyle_pth, '__fspath__') else ReStyle_pth
        opts = dict(enc_ckpt['opts'])
        if opts.get('encoder_type') != 'ProgressiveBackboneEncoder':
            raise NotImplementedError(f"ReStyle encoder_type {opts.get('encoder_type')!r}: only ProgressiveBackboneEncoder")
        from .encoder_hip import ProgressiveBackboneEncoderHIP as Enc
        self.encoder = Enc(num_layers=50, mode='ir_se', n_styles=self.style_cnt, opts=opts)
        enc_dict = OrderedDict((k[len('encoder.'):], v) for k, v in enc_ckpt['state_dict'].items() if k.startswith('encoder.'))
        self.encoder.load_state_dict(enc_dict, strict=True)
        self.encoder.progressive_stage = ProgressiveStage[stage]
        self.avg_latent = nn.Parameter(enc_ckpt['latent_avg'].detach().clone().float().reshape(self.style_cnt, style_dim), requires_grad=False)
        self.enc_cycle = enc_cycle
        self.avg_img = None

    def face_pool(self, x):
        return samm.avgpool(x, 256)

    def random_gen_center(self, scale=0.1, gen=True, noise=None):
        lats = (self.avg_latent + (torch.randn_like(self.avg_latent) * scale)).unsqueeze(0)
        out = self.generator(lats, input_is_tensor=True, input_is_latent=True, noise=noise)[0] if gen else None
        return out, lats

    def encode(self, x, **kwargs):
        """:288-318 — iterative latent prediction; returns (lats, encoder feats of the last cycle)."""
        passes = list(kwargs.get('noise_passes', None) or [])
        take = lambda: passes.pop(0) if passes else None          # noqa: E731
        with torch.no_grad():
            if self.avg_img is None:
                avg_img, _ = self.random_gen_center(scale=0, noise=take())
                self.avg_img = self.face_pool(avg_img)
            elif len(passes) > self.enc_cycle:                    # avg image cached: its noise entry is not needed
                passes.pop(0)
            if self.encoder.training:
                self.encoder.eval()
            x256 = self.face_pool(x)
            lats, feats = self.encoder(torch.cat([x256, self.avg_img.repeat(x.shape[0], 1, 1, 1)], dim=1), return_feats=True)
            lats = lats + self.avg_latent.unsqueeze(0)
            for _ in range(self.enc_cycle - 1):
                # both reference branches (:308-311) end in the plain, hook-free generator pass
                new_x = self.generator(lats.contiguous(), input_is_tensor=True, input_is_latent=True, noise=take())[0]
                delta, feats = self.encoder(torch.cat([x256, self.face_pool(new_x)], dim=1), return_feats=True)
                lats = lats + delta
        lats = lats + self.delta_latent
        truncation = kwargs.get('truncation', 1.0)
        if truncation < 1.0:
            lats = self.avg_latent.unsqueeze(0) * (1. - truncation) + (lats * truncation)
        self._final_noise = take()
        return lats.contiguous(), feats

    def forward(self, x, **kwargs):
        if kwargs.get('random_gen', False):
            return self.random_gen(batch_size=kwargs.get('batch_size', 1), gen=kwargs.get('gen', True))
        if kwargs.get('enc_lats', None) is not None:
            raise NotImplementedError('enc_lats= is the e4e entry; the ReStyle encoder is iterative')
        lats, feats = self.encode(x, **kwargs)
        kw = {k: v for k, v in kwargs.items() if k not in ('noise_passes', 'truncation')}
        if kw.get('noise', None) is None:
            kw['noise'] = self._final_noise
        return self._ood_forward(x, lats, feats, **kw)


@ARCH_REGISTRY.register()
class ood_faceGAN_FeatureStyle(ood_faceGAN_e4e):
    """The Feature-Style variant (reference src/archs/OOD_faceGAN_featureStyle_arch.py:28-334): latents from
    ``fs_encoder_v2`` (IResNet-50 trunk, pooled descriptors, 18 linear heads) on the 256² average-pooled input, SAMM taps
    = stem + first three stages, then the shared OOD forward.  ``FeatureStyle_pth`` is the encoder's state dict (loaded
    strictly, :74-79).  ``arcface_model_path`` is accepted and not read: the reference only uses it to initialise the trunk
    before ``FeatureStyle_pth`` overwrites every parameter.  Like the reference (:277-291) the encoder's ``content`` feature
    is computed and NOT injected — ``generate(lats, feats, x)`` leaves ``contents=None``."""

    def __init__(self, out_size=1024, style_dim=512, StyleGAN_pth_key='g_ema', encoder='FeatureStyle', FeatureStyle_pth=None,
                 arcface_model_path=None, avg_latent_pth=None, **kwargs):
        if encoder != 'FeatureStyle':
            raise NotImplementedError("ood_faceGAN_FeatureStyle: encoder must be 'FeatureStyle'")
        if FeatureStyle_pth is None:
            raise AssertionError('FeatureStyle_pth is required (reference :73)')
        kwargs.pop('build_encoder', None)
        kwargs.pop('E4E_pth', None)
        super().__init__(out_size=out_size, style_dim=style_dim, StyleGAN_pth_key=StyleGAN_pth_key, encoder='E4E', build_encoder=False, **kwargs)
        self.encoder_type = encoder
        from .encoder_hip import fs_encoder_v2HIP as Enc
        self.encoder = Enc(n_styles=self.style_cnt, stride=(2, 2))
        enc_ckpt = torch.load(FeatureStyle_pth, map_location='cpu') if isinstance(FeatureStyle_pth, (str, bytes)) or hasattr(FeatureStyle_pth, '__fspath__') else FeatureStyle_pth
        self.encoder.load_state_dict(enc_ckpt, strict=True)
        self.avg_latent = nn.Parameter(torch.zeros((self.style_cnt, style_dim)), requires_grad=False)
        if avg_latent_pth is not None:
            self.avg_latent.data = torch.load(avg_latent_pth, map_location='cpu')

    def face_pool(self, x):
        return samm.avgpool(x, 256)

    def encode(self, x, **kwargs):
        """:268-285"""
        with torch.no_grad():
            if self.encoder.training:
                self.encoder.eval()
            lats, self.content, feats = self.encoder(self.face_pool(x), return_feats=True)
        lats = lats + self.avg_latent.unsqueeze(0) + self.delta_latent
        truncation = kwargs.get('truncation', 1.0)
        if truncation < 1.0:
            lats = self.avg_latent.unsqueeze(0) * (1. - truncation) + (lats * truncation)
        return lats.contiguous(), feats

    def forward(self, x, **kwargs):
        if kwargs.get('random_gen', False):
            return self.random_gen(batch_size=kwargs.get('batch_size', 1), gen=kwargs.get('gen', True))
        if kwargs.get('enc_lats', None) is not None:
            raise NotImplementedError('enc_lats= is the e4e entry')
        lats, feats = self.encode(x, **kwargs)
        return self._ood_forward(x, lats, feats, **{k: v for k, v in kwargs.items() if k != 'truncation'})
