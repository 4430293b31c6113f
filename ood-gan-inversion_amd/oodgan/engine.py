"""Generator schedule on the HIP ops: forward (with optional SAMM hooks), backward w.r.t. the W+
latents, and the W+ Adam inversion loop.

``GeneratorEngine`` owns the *prepared* form of the frozen generator weights:
  * every 3x3 weight packed K-major for the MFMA implicit-GEMM kernels (forward and input-gradient
    layouts), scaled by 1/sqrt(fan_in) once;
  * per-(co,ci) squared tap sums for the factorised demodulation;
  * all 26 modulation matrices concatenated (rows grouped by latent index) so that the style affine
    of a whole forward is one MFMA contraction and its backward one kernel.
Layer order / latent indexing follow reference src/ops/StyleGAN/model.py:548-576."""
import math
import numbers
import re

import os

import torch

from . import ops
from ._lib import ACT_LRELU, ACT_NONE, CONV_S1, CONV_S2, CONV_T2
from .synth import generator_channels, make_kernel


_Cols = ops.Cols


class _Layer:
    __slots__ = ('name', 'kind', 'cin', 'cout', 'res', 'lat', 'row', 'drow', 'wpk', 'wpk_bwd', 'wsq', 'w_rgb',
                 'bias', 'noise_w', 'scale', 'noise_idx', 'src', 'sidx', 'wpk_vb')


def _pad_channels_to_16(state, prefix, log_size, ch):
    """The matrix kernels take 16-channel blocks.  A generator with other channel counts (``StyleGAN2Generator(narrow=...)``, stylegan2_arch.py:422,
    435-443: 8 channels at 1024² for narrow = 0.25) runs as the SAME function on zero-padded tensors: padded input channels get zero conv / ToRGB
    weights and a zero modulation row and bias (style 0), padded output channels zero weights and bias — they only ever hold lrelu(noise), which
    every reader multiplies by zero, and no gradient reaches the latents through them.  ToRGB weights of a padded layer carry sqrt(padded / real):
    the ops compute 1/sqrt(C) from the count they see.  Returns (state with the padded tensors, {res: padded count})."""
    up16 = lambda c: (c + 15) // 16 * 16
    chp = {r: up16(c) for r, c in ch.items()}
    out = dict(state)

    def pad(key, sizes):            # sizes: {dim: new size}
        t = state[prefix + key]
        shape = list(t.shape)
        for d, n in sizes.items():
            shape[d] = n
        if shape == list(t.shape):
            return
        new = torch.zeros(shape, dtype=t.dtype, device=t.device)
        new[tuple(slice(0, n) for n in t.shape)] = t
        out[prefix + key] = new

    def styled(name, cin, cout):
        pad(f'{name}.conv.weight', {1: up16(cout), 2: up16(cin)})
        pad(f'{name}.conv.modulation.weight', {0: up16(cin)})
        pad(f'{name}.conv.modulation.bias', {0: up16(cin)})
        pad(f'{name}.activate.bias', {0: up16(cout)})

    def rgb(name, cin):
        pad(f'{name}.conv.weight', {2: up16(cin)})
        # every ToRGB op derives its fan-in scale 1/sqrt(C) from the channel count it is handed (the padded one): fold the ratio into the weights
        if up16(cin) != cin:
            out[prefix + f'{name}.conv.weight'] = out[prefix + f'{name}.conv.weight'] * math.sqrt(up16(cin) / cin)
        pad(f'{name}.conv.modulation.weight', {0: up16(cin)})
        pad(f'{name}.conv.modulation.bias', {0: up16(cin)})

    pad('input.input', {1: up16(ch[4])})
    styled('conv1', ch[4], ch[4])
    rgb('to_rgb1', ch[4])
    cin = ch[4]
    for j in range(log_size - 2):
        cout = ch[2 ** (j + 3)]
        styled(f'convs.{2 * j}', cin, cout)
        styled(f'convs.{2 * j + 1}', cout, cout)
        rgb(f'to_rgbs.{j}', cout)
        cin = cout
    return out, chp


def style_layout(log_size, channels_of):
    """[(module name, latent index, row offset, channels)] of the (B, R) style tensor, in the generator's execution order (model.py:548-576):
    conv1, to_rgb1, then convs.2j, convs.2j+1, to_rgbs.j per level; ``channels_of(name)``: the input channels of that modulated conv.  The one
    definition of the order, for ``GeneratorEngine.style_layout`` and ``Generator.style_layout``.  Channel counts that are not multiples of 16
    run zero-padded in the engine (its rows are then not the generator's): NotImplementedError."""
    names = [('conv1', 0), ('to_rgb1', 1)]
    for j in range(log_size - 2):
        names += [(f'convs.{2 * j}', 2 * j + 1), (f'convs.{2 * j + 1}', 2 * j + 2), (f'to_rgbs.{j}', 2 * j + 3)]
    out, row = [], 0
    for name, lat in names:
        n = int(channels_of(name))
        if n % 16:
            raise NotImplementedError(f'style_layout() of a generator whose channel counts are zero-padded to multiples of 16 ({name}: {n})')
        out.append((name, lat, row, n))
        row += n
    return out


class GeneratorEngine:
    def __init__(self, state, size, style_dim=512, channel_multiplier=2, prefix='', with_backward=True, precision=None, narrow=1,
                 blur_kernel=(1, 3, 3, 1), upsample_kernel=(1, 3, 3, 1)):
        self.size, self.style_dim = size, style_dim
        self.precision = precision or ops.PRECISION
        # 'f16s-g2' (round 6): the split-f16 arithmetic with the BACK-PROPAGATED gradient rounded to f16 before each contraction —
        # g_hi * (w_hi + w_lo), two matrix instructions per product in the input-gradient convs; the forward is unchanged
        self.grad_hi_only = self.precision == 'f16s-g2'
        if self.grad_hi_only:
            self.precision = 'f16s'
        self.sform = (self.precision == 'f16s') and ops.USE_SFORM
        self.log_size = int(math.log2(size))
        self.n_latent = self.log_size * 2 - 2
        self.num_layers = (self.log_size - 2) * 2 + 1
        ch = generator_channels(channel_multiplier, narrow)
        used = [ch[2 ** i] for i in range(2, self.log_size + 1)]
        if any(c < 1 for c in used):
            raise ValueError(f'channel counts {used} (narrow={narrow}, channel_multiplier={channel_multiplier})')
        self.padded = any(c % 16 for c in used)
        self.real_channels = dict(ch)
        if self.padded:
            state, _ = _pad_channels_to_16(state, prefix, self.log_size, ch)
        g = lambda k: state[prefix + k].detach().float().contiguous()
        dev = g('input.input').device
        if dev.type != 'cuda':
            raise RuntimeError('GeneratorEngine needs its parameters on a ROCm device (no CPU fallback)')
        self.device = dev
        self.const_input = g('input.input')
        # The kernels of Blur(upsample_factor=2) in the up-convs (model.py:72-81,199-205) and of Upsample in ToRGB's skip path (model.py:30-48,
        # 353-372).  Both are registered buffers: what the state holds is what the reference runs (a loaded checkpoint overrides the constructor's
        # taps — and model.py:455 builds ToRGB WITHOUT the constructor's ``blur_kernel``, so the two families may differ); the keyword taps serve
        # states without these keys (BasicSR layout: stylegan2_arch.py:61,115 keeps them as plain attributes)
        def family(pattern, taps, what):
            pat = re.compile('^' + re.escape(prefix) + pattern + r'\.kernel$')
            held = [v.detach().float().cpu() for k, v in state.items() if pat.match(k)]
            k4 = held[0] if held else make_kernel(tuple(taps)) * 4.0
            if tuple(k4.shape) != (4, 4):
                raise NotImplementedError(f'{what} kernel of shape {tuple(k4.shape)}: the fused producers are built for four taps (every shipped config: [1,3,3,1])')
            if any(h.shape != k4.shape or not torch.equal(h, k4) for h in held):
                raise NotImplementedError(f'the {what} kernels of the state differ between layers')
            return k4.contiguous()

        k4 = family(r'convs\.\d+\.conv\.blur', blur_kernel, 'Blur')
        self.k4x4 = k4.to(dev)
        self.k4x4_flip = torch.flip(self.k4x4, [0, 1]).contiguous()
        self.k4x4_rank1 = bool(torch.linalg.matrix_rank(k4.double()) == 1)
        self.k_up = family(r'to_rgbs\.\d+\.upsample', upsample_kernel, 'Upsample').to(dev)
        self.k_up_flip = torch.flip(self.k_up, [0, 1]).contiguous()
        layers = []

        up16 = lambda c: (c + 15) // 16 * 16

        def styled(name, cin, cout, res, lat, up, nidx):        # cin / cout: the REAL counts (fan-in scale); the layer runs on the padded ones
            L = _Layer()
            L.name, L.kind, L.cin, L.cout, L.res, L.lat, L.noise_idx = name, ('up' if up else 'conv'), up16(cin), up16(cout), res, lat, nidx
            w = g(f'{name}.conv.weight')[0]                 # (Co,Ci,3,3)
            L.scale = 1.0 / math.sqrt(cin * 9)
            L.wpk = ops.pack_conv3x3(w, L.scale, transpose=False, flip=False, precision=self.precision)
            L.wpk_bwd = ops.pack_conv3x3(w, L.scale, transpose=True, flip=not up, precision=self.precision) if with_backward else None
            if L.wpk_bwd is not None:
                L.wpk_bwd.x_hi_only = self.grad_hi_only
            L.wsq = ops.weight_sqsum(w)
            L.wpk_vb = None
            L.bias = g(f'{name}.activate.bias')
            L.noise_w = g(f'{name}.noise.weight')
            layers.append(L)
            return L

        def rgb(name, cin, res, lat):
            L = _Layer()
            L.name, L.kind, L.cin, L.cout, L.res, L.lat = name, 'rgb', up16(cin), 3, res, lat
            L.w_rgb = g(f'{name}.conv.weight').reshape(3, up16(cin)).contiguous()
            L.bias = g(f'{name}.bias').reshape(3).contiguous()
            L.scale = 1.0 / math.sqrt(up16(cin))    # with the weights of a padded layer x sqrt(padded / real) (_pad_channels_to_16)
            layers.append(L)
            return L

        styled('conv1', ch[4], ch[4], 4, 0, False, 0)
        rgb('to_rgb1', ch[4], 4, 1)
        cin, i = ch[4], 1
        for j in range(self.log_size - 2):
            res = 2 ** (j + 3)
            cout = ch[res]
            styled(f'convs.{2 * j}', cin, cout, res, i, True, 2 * j + 1)
            styled(f'convs.{2 * j + 1}', cout, cout, res, i + 1, False, 2 * j + 2)
            rgb(f'to_rgbs.{j}', cout, res, i + 2)
            cin, i = cout, i + 2
        self.layers = layers
        # fused backward producers (csrc/bwd_producers.hip): per-layer range scale carried from one W+ step to the next (_new_run_state);
        # the flags below exist for the exact-scale fallback and for A/B tests (tests flip them on the instance)
        self.fused_bwd = True
        styled = [L for L in layers if L.kind != 'rgb']
        self.layers_styled_last = styled[-1]
        self.fused_fwd = True
        self.next_conv = {a.name: b for a, b in zip(styled[:-1], styled[1:]) if a.kind == 'up' and b.kind == 'conv'}
        # ToRGB layer -> the up-sampling conv that reads the same feature map next (its S-form input is written by ToRGB)
        self.rgb_next_up = {a.name: b for a, b in zip(layers[:-1], layers[1:]) if a.kind == 'rgb' and b.kind == 'up'}
        self.conv_next_rgb = {a.name: b for a, b in zip(layers[:-1], layers[1:]) if a.kind == 'conv' and b.kind == 'rgb'}
        self.by_name = {L.name: L for L in layers}
        self.fuse_act_bwd = True     # activation backward of the conv layers inside the stride-2 conv's epilogue (carried scales)
        self.hi_records = os.environ.get('OODGAN_HI_RECORDS', '1') != '0'    # f16s-g2: 32-byte hi-only gradient records between the blur^T producer and the stride-2 conv
        self.fused_rgb = True
        self.fuse_x = True           # 1024² level: F-form activations, the strip convs convert their input themselves (conv_f16s_stripx.hip)
        # the up-conv of that level in ONE pass (transposed conv + blur + noise + bias + activation -> F-form, csrc/conv_f16s_upvb.hip):
        # the blur's vertical pass folded into two 3x3 weight sets — prepared here, once, for the layer in front of the last conv
        self.fuse_up = True
        self.save_sform_only = os.environ.get('OODGAN_SAVE_SFORM_ONLY', '1') != '0'    # W+ loop: those layers' saved activation only as that S-form
        self.fuse_conv_rgb_64 = True     # ... from the 64² level on (the separate ToRGB pass started at 128²)
        self.sform_only_max_res = None   # A/B: largest resolution whose conv activation is saved only as the S-form (None: all eligible levels)
        self.fuse_conv_rgb = os.environ.get('OODGAN_FUSE_CONV_RGB', '1') != '0'    # ToRGB sums + the next up-conv's S-form from the 8-wave conv's epilogue (128² ... 512² levels, carried scales)
        self.plain_one_pass = os.environ.get('OODGAN_PLAIN_ONE_PASS', '1') != '0'     # the plain forward's last level through the one-pass up-conv + in-kernel conversion too (A/B flag)
        Lup = next((a for a, b in zip(styled[:-1], styled[1:]) if a.kind == 'up' and b is styled[-1]), None)
        if (Lup is not None and self.precision == 'f16s' and self.sform and with_backward and Lup.cout % 32 == 0 and Lup.cin % 16 == 0
                and Lup.cout <= 32 and size >= 64):
            Lup.wpk_vb = ops.pack_upconv_vblur(g(f'{Lup.name}.conv.weight')[0], Lup.scale, self.k4x4)
        ops.xf_supported(1, 32, 32, 8, 32)      # first call initialises that path (allocations must not fall into a stream capture)
        self.batched_tail = True
        src = 'input'
        for L in layers:            # producer of every layer's input feature
            L.src = src
            if L.kind != 'rgb':
                src = L.name
        # concatenated modulation matrix, rows grouped by latent index (execution order already is)
        rows, drows, wl, bl, rl = 0, 0, [], [], []
        lat_start = [0] * (self.n_latent + 1)
        row_layer, drow_layer, sidx = [], [], 0
        for L in layers:
            L.row = rows
            wl.append(g(f'{L.name}.conv.modulation.weight'))
            bl.append(g(f'{L.name}.conv.modulation.bias'))
            rl += [L.lat] * L.cin
            rows += L.cin
            lat_start[L.lat + 1] = rows
            if L.kind != 'rgb':
                L.drow = drows
                drows += L.cout
                L.sidx = sidx                       # index of the styled conv: row of the forward range-scale table
                row_layer += [sidx] * L.cin
                drow_layer += [sidx] * L.cout
                sidx += 1
            else:
                L.sidx = -1
                row_layer += [-1] * L.cin           # ToRGB colour weights use the true style
        for l in range(1, self.n_latent + 1):
            lat_start[l] = max(lat_start[l], lat_start[l - 1])
        self.R, self.DR = rows, drows
        self.wcat = torch.cat(wl, 0).contiguous()
        self.bcat = torch.cat(bl, 0).contiguous()
        self.row_lat = torch.tensor(rl, dtype=torch.int32, device=dev)
        self.lat_start = torch.tensor(lat_start, dtype=torch.int32, device=dev)
        self.row_layer = torch.tensor(row_layer, dtype=torch.int32, device=dev)
        self.drow_layer = torch.tensor(drow_layer, dtype=torch.int32, device=dev)
        self.n_styled = sidx
        self.carry_range = True      # False: every forward measures its scales exactly (the fallback after a violation)
        self.stored_noises = [g(f'noises.noise_{k}') for k in range(self.num_layers)] if (prefix + 'noises.noise_0') in state else None
        # ConstantInput broadcast over the batch, one copy per (batch size, stream): prepared data like the weights, shared between clones
        # (clones are made per inversion and must not make the copies again)
        self._const_b = {}
        self._new_run_state()

    def _new_run_state(self):
        """Everything a run of this engine writes, in one place: what ``clone_shared`` must not share.  A state attribute created anywhere
        else would silently be shared between the sub-batches of two HIP streams."""
        self.saved = None                           # forward(save=True) -> backward: activations, styles, demodulation factors
        self._fwd_serial = 0                        # forwards counted: backward() refuses activations a later forward may have overwritten
        self.bwd_state, self.bwd_flag = {}, None    # backward range scale per layer, carried from one W+ step to the next; their sticky flag
        # forward range control of the split-f16 path (ops.FwdRange): one state per batch size, ``fwd_range`` the one in use
        self.fwd_range, self._ranges = None, {}
        self.last_gs = None                         # dL/dstyles of the last backward, kept for inspection

    def clone_shared(self):
        """A second engine over the SAME prepared weights (read-only) with its own per-run state."""
        import copy
        e = copy.copy(self)
        e._new_run_state()
        return e

    def reset_fwd_state(self, B=None):
        """Forget the carried forward range scales (new images / new batch): the next forward measures them exactly.
        Every batch size's state is reset (``B``: only that one) — a state left `valid` with another image set's scales would
        make the first forward at that batch size run in carry mode and the result depend on the call history."""
        todo = list(self._ranges.values()) if B is None else [r for r in (self._ranges.get(B),) if r is not None]
        if self.fwd_range is not None and (B is None or self.fwd_range.B == B) and not any(r is self.fwd_range for r in todo):
            todo.append(self.fwd_range)
        for r in todo:
            r.valid = False
            r.flag.zero_()
            r.vm.zero_()       # maxima an aborted carry pass left behind must not enter the next measurement

    def fwd_range_violated(self):
        """True if a carried forward scale left the exact window in any forward since reset_fwd_state() (host sync)."""
        return self.fwd_range is not None and self.fwd_range.violated()

    def _range(self, B):
        if self.fwd_range is None or self.fwd_range.B != B:
            # one state per batch size (an inversion alternates between the sub-batch of the W+ loop and the full batch of the OOD forward:
            # the latter's carried scales survive the former)
            r = self._ranges.get(B)
            if r is None:
                # never evicted: captured hipGraphs (arch.GraphedForward, the W+ step graphs) hold raw pointers to a state's
                # q / vm / flag / s_sc / d_sc — a state is ~100 KB per batch size
                r = self._ranges[B] = ops.FwdRange(self.n_styled, B, self.R, self.DR, self.row_layer, self.drow_layer, self.device)
            self.fwd_range = r
        return self.fwd_range

    def reset_bwd_state(self):
        """Forget the carried range scales (new images / new batch): the next backward measures them exactly."""
        self.bwd_state = {}
        if self.bwd_flag is not None:
            self.bwd_flag.zero_()

    def bwd_scale_violated(self):
        """True if a carried range scale left the exact window in any step since reset_bwd_state() (host sync)."""
        return self.bwd_flag is not None and int(self.bwd_flag.item()) != 0

    # ------------------------------------------------------------------ forward
    def styles(self, latent, offsets=None):
        """(B, n_latent, S) -> all style vectors (B, R) in one contraction; ``offsets`` (B, R): StyleSpace offsets added to them."""
        return ops.style_affine(latent, self.wcat, self.bcat, self.row_lat, offset=offsets)

    def style_layout(self):
        """[(layer name, latent index, first row, channels)] in row order: the meaning of a column of the (B, R) style tensor."""
        if self.padded:
            raise NotImplementedError('style_layout() of a generator whose channel counts are zero-padded to multiples of 16')
        lay = style_layout(self.log_size, lambda name: self.by_name[name].cin)
        assert lay == [(L.name, L.lat, L.row, L.cin) for L in self.layers]      # the rows the kernels use
        return lay

    def feature_shape(self, l):
        """(C, h, h) of the feature offset on the input of the styled up-conv that reads latent ``l``; ValueError for a
        latent outside FEATURE_LAYERS or one this generator's size does not have, NotImplementedError on a zero-padded generator."""
        l = check_feature_layer(l, self.n_latent)
        if self.padded:
            raise NotImplementedError('feature_layer on a generator whose channel counts are zero-padded to multiples of 16')
        L = next(L for L in self.layers if L.kind == 'up' and L.lat == l)
        return (L.cin, L.res // 2, L.res // 2)

    def forward(self, latent, noises, save=False, cond_hook=None, cond_layers=None, return_features=False, features_in=None,
                feature_scale=1.0, range_mode='exact', post_hook=None, style_offsets=None, feature_offset=None, feature_out=None):
        """latent (B,n_latent,S); noises list[num_layers] of (B|1,1,r,r).
        cond_hook(k, raw, latent_i, noise, noise_w) -> cond tensor replacing the raw up-conv output
        (the algebra of OOD_faceGAN_e4e_arch.py:239-242 + model.py:292: layer = cond + w*noise).
        features_in[i] (or None), feature_scale: `insert_feature` of the Feature-Style variant (model.py:541-546,557,572):
        the input of the styled conv that reads latent i becomes (1-fs)*x + fs*features_in[i].
        post_hook(k, out) -> tensor replacing the ACTIVATED output of the up-conv reading latent cond_layers[k]
        (feature_modulation for cond_type 'SFT' / 'ADD' / 'FUSE', model.py:558-566).
        range_mode (split-f16 only, ops.FwdRange): 'exact' measures max|x*s| of every conv input before converting it;
        'carry' (the W+ loop) uses the scales of the previous forward with the fused producers and verifies them.
        style_offsets: float32 (B, R) added to the styles, s = style_affine(latent) + style_offsets (StyleSpace; the columns
        are those of ``style_layout()``).  Everything downstream reads the sum; the hooks still receive the latent of their layer.
        feature_offset: (l, delta) — float32 (B, C, h, h) added to the input of the styled up-conv that reads latent l, x' = x + delta
        (F/W+; l in FEATURE_LAYERS, the shape: ``feature_shape(l)``).  ToRGB of the level below and the backward of the conv
        below keep reading x; with ``save`` both tensors are kept.  Unlike ``features_in`` it leaves carry mode on.  ``feature_out``: the
        buffer x' is written to (the W+ loop's persistent one); None: a new tensor."""
        if self.padded and (cond_hook is not None or features_in is not None or post_hook is not None):
            raise NotImplementedError('conditioning hooks / feature injection on a generator whose channel counts are zero-padded to multiples of 16')
        if save and (features_in is not None or post_hook is not None):
            raise NotImplementedError('backward through an injected feature / feature modulation is not part of the path')
        if self.padded and style_offsets is not None:
            raise NotImplementedError('style offsets on a generator whose channel counts are zero-padded to multiples of 16')
        B = latent.shape[0]
        f_lat, f_delta, f_in = None, None, None
        if feature_offset is not None:
            f_lat, f_delta = feature_offset
            if tuple(f_delta.shape) != (B,) + self.feature_shape(f_lat):        # checks the layer too
                raise ValueError(f'feature_offset for latent {f_lat} must be {(B,) + self.feature_shape(f_lat)}, got {tuple(f_delta.shape)}')
        # forwards are counted: the activations saved for backward() live in pooled scratch buffers (ops.sform_scratch: keyed by shape and
        # stream) and their S-form scales alias the range state — ANY later forward of this engine on the same stream may overwrite them
        self._fwd_serial += 1
        s_all = self.styles(latent, style_offsets)
        d_all = torch.empty(B, self.DR, device=self.device, dtype=torch.float32)
        if self.batched_tail:       # the demodulation factors of all styled convs in one launch
            from ._lib import DemodFwdJob, lib, check
            import ctypes
            styled = [L for L in self.layers if L.kind != 'rgb']
            arr = (DemodFwdJob * len(styled))(*[DemodFwdJob(ctypes.c_void_p(s_all.data_ptr() + 4 * L.row), ctypes.c_void_p(L.wsq.data_ptr()),
                                                            ctypes.c_void_p(d_all.data_ptr() + 4 * L.drow), self.R, self.DR, B, L.cin, L.cout,
                                                            float(L.scale)) for L in styled])
            check(lib().oodgan_demod_fwd_batch(arr, len(styled), ops._stream()), 'demod_fwd_batch')
        else:
            for L in self.layers:
                if L.kind != 'rgb':
                    self._demod(L, s_all, d_all)
        rng, carry = None, False
        s_use, d_use = s_all, d_all
        if self.sform:
            rng = self._range(B)
            # cond_hook (the SAMM hook of the OOD forward) does not stand in the way: a hooked layer's output is converted by to_s(),
            # which takes the carried scale and records the maximum like any fused producer
            carry = range_mode == 'carry' and rng.valid and self.carry_range and features_in is None and post_hook is None
            if carry:
                rng.plan(s_all, d_all)
            s_use, d_use = rng.s_sc, rng.d_sc

        def to_s(L, t):
            # S-form input of styled conv L from the fp32 tensor t (x its style x the layer's range scale)
            if not carry:
                rng.measure(L.sidx, t, _Cols(s_all, L.row, L.cin))
                rng.plan(s_all, d_all, L.row, L.cin, L.drow, L.cout)
            return ops.to_sform(t, _Cols(s_use, L.row, L.cin), out=ops.sform_scratch(B, L.cin, t.shape[2], t.shape[3], self.device),
                                vmax=rng.vm[L.sidx] if carry else None)

        acts = {}
        # ConstantInput broadcast over the batch (model.py:296-305): read-only, one copy per batch size — not a torch copy kernel per forward
        # (a launch plan, oodgan_plan_*, replays this library's launches only)
        ck = (B, ops._stream_handle())      # per stream: the copy is enqueued on the stream that first needs it
        x = self._const_b.get(ck)
        if x is None:
            x = self._const_b[ck] = self.const_input.expand(B, -1, -1, -1).contiguous()
        acts['input'] = x
        skip, out = None, x
        pending = None
        rgb_partial = None
        i = 1
        for L in self.layers:
            s = _Cols(s_all, L.row, L.cin)
            if L.kind == 'rgb' and rgb_partial is not None:
                skip = ops.rgb_finish(rgb_partial, L.bias, skip, self.k_up if skip is not None else None)
                rgb_partial = None
                continue
            if L.kind == 'rgb':
                Lu = self.rgb_next_up.get(L.name) if (carry and self.fused_rgb) else None
                if (Lu is not None and pending is None and out.shape[2] * out.shape[3] > 4096 and L.cin % 16 == 0
                        and out.shape[3] % 4 == 0):
                    # one pass over the feature map: RGB contribution AND the next up-conv's S-form input (x its style)
                    pending = ops.sform_scratch(B, L.cin, out.shape[2], out.shape[3], self.device)
                    skip = ops.torgb(out, L.w_rgb, s, L.bias, skip, self.k_up if skip is not None else None, ys=pending,
                                     ys_scale=_Cols(s_use, Lu.row, Lu.cin), vmax=rng.vm[Lu.sidx])
                else:
                    skip = ops.torgb(out, L.w_rgb, s, L.bias, skip, self.k_up if skip is not None else None)
                continue
            d = _Cols(d_use, L.drow, L.cout)
            nz = noises[L.noise_idx]
            if features_in is not None and L.lat >= 1 and L.lat < len(features_in) and features_in[L.lat] is not None:
                from . import samm as _samm
                f = features_in[L.lat].to(out.dtype).contiguous()
                C = out.shape[1]
                ones = torch.ones(B, C, device=self.device)
                zeros = torch.zeros(B, C, device=self.device)
                t = _samm.affine_apply(f, ones * float(feature_scale), zeros)
                out = _samm.affine_apply(out, ones * float(1.0 - feature_scale), zeros, res=t)
                pending = None              # an S-form written for the un-mixed tensor is stale
            if L.lat == f_lat:
                # the offset layer reads x' = out + delta; ``acts`` keeps the un-offset tensor under the name of the conv that made it.  No
                # producer below 64² writes an S-form ahead of its reader: what to_s() converts next is x'
                assert L.kind == 'up' and pending is None and isinstance(out, torch.Tensor), (L.name, pending is not None, type(out))
                out = f_in = ops.feature_add(out, f_delta, out=feature_out)
            if L.kind == 'conv':
                if self.sform:
                    # S-form hand-off: style folded in while splitting, the conv then streams its tiles by LDS-DMA
                    xf_in = isinstance(out, ops.FForm)      # the up-conv tail left its activation in F-form: converted inside the conv
                    if xf_in:
                        xs = out
                    elif pending is not None:     # written by the up-conv tail that produced `out`
                        xs, pending = pending, None
                    else:
                        xs = to_s(L, out)
                    Lr = self.conv_next_rgb.get(L.name) if self.fused_rgb else None
                    if Lr is not None and 16 < L.cin <= 32 and 16 < L.cout <= 32:
                        # 32-channel 1024² layer (strip kernel): the ToRGB colour sums come out of the same epilogue.
                        # Inside the W+ loop the activation of the LAST styled conv is read back by nothing but its own activation
                        # backward: once that runs as the fused producer (a carried scale exists) it is kept in F-form — both
                        # sides then move 16 bytes per lane on contiguous runs
                        ff = (save and carry and self.fused_bwd and L is self.layers_styled_last and L.cout == 32
                              and self.bwd_state.get(L.name) is not None and not return_features)
                        out, rgb_partial = ops.conv3x3(xs, L.wpk, L.cout, CONV_S1, out_scale=d, bias=L.bias, noise=nz,
                                                       noise_weight=L.noise_w, act=ACT_LRELU, rgb=(Lr.w_rgb, _Cols(s_all, Lr.row, Lr.cin)),
                                                       y_fform=ff or xf_in, in_scale=_Cols(s_use, L.row, L.cin) if xf_in else None)
                    else:
                        Lu = self.rgb_next_up.get(Lr.name) if (Lr is not None and carry) else None
                        Hc, Wc = xs.shape[2], xs.shape[3]
                        if (Lu is not None and self.fuse_conv_rgb and not xf_in and L.cout % 16 == 0 and Hc * Wc > (4095 if self.fuse_conv_rgb_64 else 4096) and Wc % 4 == 0
                                and ops.s1_ys_supported(B, L.cin, L.cout, Hc, Wc)):
                            # round 4: the 8-wave conv hands BOTH consumers of its output their input from its registers — the ToRGB colour
                            # sums (one partial per 64-channel block, finished by rgb_finish) and the S-form of out x style x range scale of
                            # the next up-conv, with the maximum for its range control: the torgb_fwd_sform pass (a read of the feature
                            # map at 128² ... 512²) disappears from the step
                            pending = ops.sform_scratch(B, L.cout, Hc, Wc, self.device, tag=4)
                            # both readers of the activation are served from the epilogue: without a backward pass to save it for, the fp32
                            # tensor is not written at all (the epilogue's stores are what these launches wait for, LABNOTES.md §13.9)
                            # ... and inside the W+ loop the saved activation exists ONCE: the only reader of this layer's output in the
                            # backward pass is the fused epilogue of the stride-2 conv above (style-gradient dot + this layer's
                            # activation backward), which decodes it from the same S-form (oodgan_conv_args.dotx_sform)
                            sform_only = (save and self.save_sform_only and self.fused_bwd and self.fuse_act_bwd
                                          and (self.sform_only_max_res is None or Hc <= self.sform_only_max_res)
                                          and self.bwd_state.get(L.name) is not None and self.bwd_state.get(Lu.name) is not None
                                          and ops.s2_fuse_supported(B, Lu.cout, Lu.cin, 2 * Hc + 1, 2 * Wc + 1))
                            keep = (save and not sform_only) or return_features or post_hook is not None
                            out, rgb_partial = ops.conv3x3(xs, L.wpk, L.cout, CONV_S1, out_scale=d, bias=L.bias, noise=nz, noise_weight=L.noise_w,
                                                           act=ACT_LRELU, rgb=(Lr.w_rgb, _Cols(s_all, Lr.row, Lr.cin)), ys=pending,
                                                           ys_scale=_Cols(s_use, Lu.row, Lu.cin), vmax=rng.vm[Lu.sidx], want_y=keep)
                            if not keep:
                                out = ops.SFormSaved(pending, _Cols(s_use, Lu.row, Lu.cin))
                        else:
                            out = ops.conv3x3(xs, L.wpk, L.cout, CONV_S1, out_scale=d, bias=L.bias, noise=nz,
                                              noise_weight=L.noise_w, act=ACT_LRELU)
                    del xs
                else:
                    out = ops.conv3x3(out, L.wpk, L.cout, CONV_S1, in_scale=s, out_scale=d, bias=L.bias, noise=nz,
                                      noise_weight=L.noise_w, act=ACT_LRELU)
            else:
                Hi = out.shape[2]
                Ln = self.next_conv.get(L.name)
                # last level inside the W+ loop: the activation stays in F-form and the conv converts it itself — no S-form copy of
                # the largest tensor of the step is written or read
                ff_tail = (self.sform and carry and self.fused_fwd and Ln is not None and save and self.fuse_x and self.fused_bwd and self.fused_rgb
                           and Ln is self.layers_styled_last and not return_features
                           and self.bwd_state.get(Ln.name) is not None and self.bwd_state.get(L.name) is not None
                           and ops.xf_supported(B, Ln.cin, Ln.cout, 2 * Hi, 2 * Hi))
                one_pass = ff_tail and self.fuse_up and L.wpk_vb is not None and ops.upconv_vblur_supported(B, L.cin, L.cout, Hi, Hi)
                # the plain forward (model(x), exact ranges) takes the same two kernels: the up-conv kernel records max|y * style| of the
                # F-form activation it writes, the range scale of the last conv is set from it on the device — no (2H+1)² intermediate,
                # no blur pass, no measurement pass and no S-form copy of the 1024² tensor
                plain_tail = (self.sform and not save and not one_pass and self.plain_one_pass and self.fuse_up and self.fuse_x
                              and self.fused_rgb and Ln is not None and Ln is self.layers_styled_last and L.wpk_vb is not None
                              and Ln.name in self.conv_next_rgb and 16 < Ln.cin <= 32 and 16 < Ln.cout <= 32
                              and not (cond_layers is not None and L.lat in cond_layers)
                              and not (features_in is not None and Ln.lat < len(features_in) and features_in[Ln.lat] is not None)
                              and ops.upconv_vblur_supported(B, L.cin, L.cout, Hi, Hi) and ops.xf_supported(B, Ln.cin, Ln.cout, 2 * Hi, 2 * Hi))
                z = None
                if self.sform:
                    if pending is not None:
                        xs, pending = pending, None
                    else:
                        xs = to_s(L, out)
                    if one_pass:
                        # ... and the (2H+1)² transposed-conv result is not written either: conv + blur + noise + bias + activation in ONE kernel
                        out = ops.upconv_vblur_fform(xs, L.wpk_vb, out_scale=d, bias=L.bias, noise=nz, noise_weight=L.noise_w, act=True,
                                                     ys_scale=_Cols(s_use, Ln.row, Ln.cin), vmax=rng.vm[Ln.sidx])
                    elif plain_tail:
                        out = ops.upconv_vblur_fform(xs, L.wpk_vb, out_scale=d, bias=L.bias, noise=nz, noise_weight=L.noise_w, act=True,
                                                     ys_scale=_Cols(s_use if carry else s_all, Ln.row, Ln.cin), vmax=rng.vm[Ln.sidx])
                        if not carry:       # exact ranges: the scale of the last conv from the maximum just recorded
                            rng.update_exact(Ln.sidx)
                            rng.plan(s_all, d_all, Ln.row, Ln.cin, Ln.drow, Ln.cout)
                        one_pass = True
                    else:
                        z = ops.conv3x3(xs, L.wpk, L.cout, CONV_T2, out_scale=d)
                    del xs
                else:
                    z = ops.conv3x3(out, L.wpk, L.cout, CONV_T2, in_scale=s, out_scale=d)
                H2 = 2 * Hi + 1
                lat_idx = L.lat
                if one_pass:
                    pass
                elif cond_hook is not None and cond_layers is not None and lat_idx in cond_layers:
                    raw = ops.blur_bias_act(z, self.k4x4, (1, 1), act=False, in_hw=(H2, H2), in_pitch=z.shape[3])
                    cond = cond_hook(cond_layers.index(lat_idx), raw, latent[:, lat_idx], nz, L.noise_w)
                    out = ops.bias_noise_act(cond, L.bias, nz, L.noise_w)
                elif carry and self.fused_fwd and L.name in self.next_conv:
                    # blur + noise + bias + activation, and the following conv's S-form input (x its style), in one pass
                    if ff_tail:
                        out = ops.blur_act_fform(z, self.k4x4, Hi, Hi, L.bias, nz, L.noise_w, act=True,
                                                 ys_scale=_Cols(s_use, Ln.row, Ln.cin), vmax=rng.vm[Ln.sidx], rank_one=self.k4x4_rank1)
                    else:
                        pending = ops.sform_scratch(B, L.cout, 2 * Hi, 2 * Hi, self.device, tag=2)
                        out = ops.blur_act_sform(z, self.k4x4, Hi, Hi, L.bias, nz, L.noise_w, act=True, ys=pending,
                                                 ys_scale=_Cols(s_use, Ln.row, Ln.cin), vmax=rng.vm[Ln.sidx], rank_one=self.k4x4_rank1)
                else:
                    out = ops.blur_bias_act(z, self.k4x4, (1, 1), L.bias, nz, L.noise_w, act=True, in_hw=(H2, H2),
                                            in_pitch=z.shape[3])
                del z
                if post_hook is not None and cond_layers is not None and lat_idx in cond_layers:
                    out = post_hook(cond_layers.index(lat_idx), out)
                    pending = None
            acts[L.name] = out
        if rng is not None:
            if carry:
                rng.finish()            # verify the carried scales, publish the next ones
            else:
                rng.valid = True
        if save:
            self.saved = dict(acts=acts, s_all=s_all, d_all=d_all, noises=noises, B=B, serial=self._fwd_serial, f_lat=f_lat, f_in=f_in)
        if return_features:
            feat = out.to_nchw() if isinstance(out, ops.FForm) else out
            return skip, (feat[:, :self.real_channels[self.size]].contiguous() if self.padded else feat)
        return skip

    def _demod(self, L, s_all, d_all):
        from ._lib import lib, check
        import ctypes
        B = s_all.shape[0]
        check(lib().oodgan_demod_fwd(ctypes.c_void_p(s_all.data_ptr() + 4 * L.row), self.R, ctypes.c_void_p(L.wsq.data_ptr()),
                                     ctypes.c_void_p(d_all.data_ptr() + 4 * L.drow), self.DR, B, L.cin, L.cout, L.scale,
                                     ops._stream()), 'demod_fwd')

    def _hi_records(self, B, L, Hd, Rg):
        """precision 'f16s-g2': the gradient of an up-conv layer goes to its stride-2 input-gradient conv as 32-byte hi-only records when that
        conv is the two-instruction 8-wave kernel (which never reads a lo half) and the producer is the strip walk (oodgan_act_bwd_blurT_sform_phases_hi):
        half the bytes written by the one and read by the other."""
        return bool(self.grad_hi_only and self.hi_records and Rg is None and ops.blurT_hi_supported(Hd, Hd)
                    and ops.s2_fuse_supported(B, L.cout, L.cin, 2 * Hd + 1, 2 * Hd + 1))

    # ------------------------------------------------------------------ backward (w.r.t. latents only)
    def backward(self, gimg, grad_scale=1.0, carry_scale=False, wrt='latent', feature_grad=None):
        """gimg (B,3,size,size), already multiplied by ``grad_scale`` -> dL/dlatent (B,n_latent,S).
        ``wrt='styles'``: dL/dstyles (B,R) instead — also the gradient of ``style_offsets`` — still multiplied by ``grad_scale``; the
        contraction with the modulation matrices does not run.
        Needs forward(..., save=True).  Every step is linear in the gradient, so a power-of-two
        grad_scale is undone exactly at the end.
        ``carry_scale`` (set by the W+ loop): from the second call on, the activation gradients are produced directly
        in the matrix kernels' input layout with the range scale measured on the previous call (fused producers);
        the caller must start a new sequence with reset_bwd_state() and check bwd_scale_violated() at its end.
        ``feature_grad``: after forward(feature_offset=, save=True), the contiguous float32 buffer of the offset's shape that receives
        dL/ddelta = dL/dx', still multiplied by ``grad_scale``: the fp32 result of the offset layer's input-gradient conv, which therefore
        runs without the fused epilogue at that one layer; the gradient continues downward unchanged."""
        from ._lib import lib, check
        import ctypes
        if wrt not in ('latent', 'styles'):
            raise ValueError(f"wrt must be 'latent' or 'styles', got {wrt!r}")
        sv = self.saved
        if sv is None:
            raise RuntimeError('backward() without forward(save=True)')
        if sv['serial'] != self._fwd_serial:
            raise RuntimeError('backward(): another forward of this engine ran after forward(save=True) — the saved activations (pooled S-form / F-form '
                               'buffers, scales of the range state) may have been overwritten; call backward() right after the forward it belongs to')
        acts, s_all, d_all, noises, B = sv['acts'], sv['s_all'], sv['d_all'], sv['noises'], sv['B']
        f_lat, f_in = sv['f_lat'], sv['f_in']
        if (feature_grad is not None) != (f_lat is not None):
            raise RuntimeError('backward(feature_grad=) goes with forward(feature_offset=, save=True), and one needs the other')
        if feature_grad is not None and not (tuple(feature_grad.shape) == tuple(f_in.shape) and feature_grad.dtype == torch.float32
                                             and feature_grad.is_contiguous() and feature_grad.device == f_in.device):
            raise ValueError(f'feature_grad must be a contiguous float32 {tuple(f_in.shape)} tensor on {f_in.device}')
        gs_all = ops.zeros(B, self.R, device=self.device)
        # gradient of the skip chain: gskip[res] for every ToRGB level
        gskip = {self.size: gimg.contiguous()}
        r = self.size
        while r > 4:
            gskip[r // 2] = ops.upfirdn2d(gskip[r], self.k_up_flip, up=1, down=2, pad=(1, 1))
            r //= 2
        g_feat = None
        prev_rgb = None
        fused_in = None         # ops.ActBwdFusion produced by the stride-2 conv of the layer above
        fused_pre = None        # ops.DotActGrad: the stride-1 conv above already applied this up-conv layer's act'
        jobs = ops.BwdJobs() if (carry_scale and self.fused_bwd and self.sform and self.batched_tail) else None
        for L in reversed(self.layers):
            if L.kind == 'rgb':          # fused into the backward of the styled conv that feeds it
                prev_rgb = L
                continue
            out, x_in, nz = acts[L.name], acts[L.src], noises[L.noise_idx]
            # the offset layer: its input was x' = x + delta — the style-gradient dot reads x', the conv writes dL/dx' in fp32 into the
            # caller's buffer, and the activation backward of the layer below (which reads acts[L.src], the un-offset x) runs unfused
            at_f = L.lat == f_lat
            if at_f:
                x_in = f_in
            dx_out = feature_grad if at_f else None
            fused_ok = carry_scale and self.fused_bwd and self.bwd_state.get(L.name) is not None
            # last level: out and x_in in F-form -> the activation backward runs inside the input-gradient conv (ops.ActBwdX)
            xf_bwd = (fused_ok and g_feat is None and L.kind == 'conv' and isinstance(out, ops.FForm) and isinstance(x_in, ops.FForm)
                      and prev_rgb is not None and self.fuse_x)
            if isinstance(out, ops.FForm) and not (fused_ok and (g_feat is None or fused_pre is not None)):
                out = out.to_nchw()         # the two-pass path reads NCHW
            if isinstance(out, ops.SFormSaved) and fused_in is None:
                out = out.to_nchw()         # saved only as its consumer's S-form, but this layer's activation backward did not run fused
            if isinstance(x_in, ops.FForm) and not xf_bwd:
                x_in = x_in.to_nchw()
            s = _Cols(s_all, L.row, L.cin)
            d = _Cols(d_all, L.drow, L.cout)
            Hd = x_in.shape[2]
            carry = carry_scale and self.fused_bwd and self.sform and (L.kind == 'conv' or Hd >= 4)
            st = self.bwd_state.get(L.name) if carry else None
            Rg, prev_rgb = prev_rgb, None
            rgb_kw = {} if Rg is None else dict(g_rgb=gskip[L.res], w_rgb=Rg.w_rgb, s_rgb=_Cols(s_all, Rg.row, Rg.cin))
            if st is not None and fused_in is not None:
                # this layer's activation backward already ran in the epilogue of the stride-2 conv above (its S-form
                # gradient, partial sums and maxima come from there; g_feat never went to HBM)
                gin, rsum, tsum, part_m = fused_in.dst, fused_in.r, None, fused_in.part_m
                fused_in = None
                mul2, g_pre = st, None
            elif st is not None and xf_bwd:
                gin, rsum, tsum, part_m = None, None, None, None        # produced by the conv below (ops.ActBwdX)
                mul2, g_pre = st, None
            elif st is not None:
                # fused producer: g_pre goes straight into the next matrix kernel's input layout, scaled with the
                # range scale measured on the previous step (verified below, after the conv has consumed it)
                t_into = None if Rg is None else _Cols(gs_all, Rg.row, Rg.cin)
                if L.kind == 'conv':
                    gin = ops.sform_scratch(B, L.cout, out.shape[2], out.shape[3], self.device)
                    rsum, tsum, part_m = ops.act_bwd_producer(out, g_feat, nz, L.noise_w, L.bias, d, st, gin, t_into=t_into, jobs=jobs, **rgb_kw)
                elif fused_pre is not None:
                    # g_feat already is g_pre: blur^T + phase split of one tensor; r = noise / bias term + s * dot of that conv
                    gin = ops.sform_phases_scratch(B, L.cout, Hd, Hd, self.device)
                    rsum, tsum, part_m = ops.act_bwd_producer(None, g_feat, nz, L.noise_w, L.bias, d, st, gin, blur_kernel=self.k4x4_flip,
                                                              jobs=jobs, dot_of=fused_pre, hi_only=self._hi_records(B, L, Hd, Rg))
                    fused_pre = None
                else:
                    gin = ops.sform_phases_scratch(B, L.cout, Hd, Hd, self.device)
                    rsum, tsum, part_m = ops.act_bwd_producer(out, g_feat, nz, L.noise_w, L.bias, d, st, gin,
                                                              blur_kernel=self.k4x4_flip, t_into=t_into, jobs=jobs,
                                                              hi_only=self._hi_records(B, L, Hd, Rg), **rgb_kw)
                mul2, g_pre = st, None
            else:
                if Rg is not None:
                    g_pre, rsum, tsum, mul2 = ops.act_bwd_fused(out, g_feat, nz, L.noise_w, L.bias, gskip[L.res], Rg.w_rgb,
                                                                _Cols(s_all, Rg.row, Rg.cin), want_scale=True, dscale=d)
                else:
                    g_pre, rsum, tsum, mul2 = ops.act_bwd_fused(out, g_feat, nz, L.noise_w, L.bias, want_scale=True, dscale=d)
                if carry:
                    self.bwd_state[L.name] = mul2            # exact this step; carried to the next one
                    if self.bwd_flag is None:
                        self.bwd_flag = torch.zeros(1, dtype=torch.int32, device=self.device)
            if Rg is not None and tsum is not None:
                gs_all[:, Rg.row:Rg.row + Rg.cin] = tsum
            # demodulation gradient
            deferred = st is not None and jobs is not None
            xa = None
            if st is not None and xf_bwd:
                xa = ops.ActBwdX(nz, L.noise_w, L.bias, d, st, gskip[L.res], Rg.w_rgb, _Cols(s_all, Rg.row, Rg.cin),
                                 t_into=_Cols(gs_all, Rg.row, Rg.cin))
                pre = None
                Lp = self.by_name.get(L.src)
                if (Lp is not None and Lp.kind == 'up' and self.fuse_act_bwd and self.bwd_state.get(L.src) is not None
                        and ops.s1_actgrad_supported(B, L.cout, L.cin, out.shape[2], out.shape[3])):
                    pre = ops.DotActGrad()
                dx, dot = ops.conv3x3(out, L.wpk_bwd, L.cin, CONV_S1, out_scale=s, dotx=x_in, in_mul2=mul2,
                                      dot_into=_Cols(gs_all, L.row, L.cin), jobs=jobs, dot_actgrad=pre, xf_act=xa)
                rsum, part_m = xa.r, xa.part_m
                fused_in, fused_pre = None, pre
            if deferred:        # rsum is filled by the batched reduction at the end of the pass; so is this job's input
                jobs.add_demod(_Cols(s_all, L.row, L.cin), L.wsq, _Cols(d_all, L.drow, L.cout), rsum, _Cols(gs_all, L.row, L.cin), B, L.cin,
                               L.cout, L.scale)
            else:
                check(lib().oodgan_demod_bwd(ctypes.c_void_p(s_all.data_ptr() + 4 * L.row), self.R, ctypes.c_void_p(L.wsq.data_ptr()),
                                             ctypes.c_void_p(d_all.data_ptr() + 4 * L.drow), self.DR, ctypes.c_void_p(rsum.data_ptr()),
                                             ctypes.c_void_p(gs_all.data_ptr() + 4 * L.row), self.R, B, L.cin, L.cout, L.scale,
                                             ops._stream()), 'demod_bwd')
            if xa is not None:
                if deferred:
                    jobs.add_check(part_m, st)
                else:
                    ops.absmax_scale_check(part_m, st, self.bwd_flag)
            elif st is not None:
                fz = None
                Lp = self.by_name.get(L.src)
                stp = self.bwd_state.get(L.src) if (L.kind == 'up' and Lp is not None and self.fuse_act_bwd) else None
                if stp is not None and not at_f and ops.s2_fuse_supported(B, L.cout, L.cin, 2 * Hd + 1, 2 * Hd + 1):
                    # the stride-2 conv's result is the gradient w.r.t. the output of the conv layer below (x_in): its
                    # epilogue continues with that layer's activation backward (+ ToRGB branch) and writes the S-form
                    Rp = self.conv_next_rgb[Lp.name]
                    # f16s-g2: that S-form as 32-byte hi-only records when the conv that reads it is the two-instruction 8-wave stride-1 kernel
                    hi = bool(self.grad_hi_only and self.hi_records and ops.s1_xh_supported(B, Lp.cout, Lp.cin, Hd, Hd))
                    fz = ops.ActBwdFusion((ops.sform_hi_scratch if hi else ops.sform_scratch)(B, Lp.cout, Hd, Hd, self.device), noises[Lp.noise_idx],
                                          Lp.noise_w, Lp.bias, _Cols(d_all, Lp.drow, Lp.cout), stp, g_rgb=gskip[Lp.res], w_rgb=Rp.w_rgb,
                                          s_rgb=_Cols(s_all, Rp.row, Rp.cin), t_into=_Cols(gs_all, Rp.row, Rp.cin), hi_only=hi)
                pre = None
                if (L.kind == 'conv' and Lp is not None and Lp.kind == 'up' and self.fuse_act_bwd and self.bwd_state.get(L.src) is not None
                        and ops.s1_actgrad_supported(B, L.cout, L.cin, out.shape[2], out.shape[3])):
                    # x_in is the output of the up-sampling layer below: this conv's epilogue applies that layer's act',
                    # the blur^T producer then reads one tensor
                    pre = ops.DotActGrad()
                dx, dot = ops.conv3x3(gin, L.wpk_bwd, L.cin, CONV_S1 if L.kind == 'conv' else CONV_S2, out_scale=s, dotx=x_in,
                                      in_mul2=mul2, dot_into=_Cols(gs_all, L.row, L.cin), jobs=jobs, fuse=fz, want_y=fz is None,
                                      dot_actgrad=pre, out=dx_out)
                fused_in, fused_pre = fz, pre
                del gin
                if deferred:
                    jobs.add_check(part_m, st)
                else:
                    ops.absmax_scale_check(part_m, st, self.bwd_flag)
            elif L.kind == 'conv':
                if self.sform:
                    gs_ = ops.to_sform(g_pre, d, mul2, out=ops.sform_scratch(B, L.cout, g_pre.shape[2], g_pre.shape[3], self.device))
                    dx, dot = ops.conv3x3(gs_, L.wpk_bwd, L.cin, CONV_S1, out_scale=s, dotx=x_in, in_mul2=mul2)
                    del gs_
                else:
                    dx, dot = ops.conv3x3(g_pre, L.wpk_bwd, L.cin, CONV_S1, in_scale=d, out_scale=s, dotx=x_in, in_mul2=mul2)
            else:
                if self.sform and Hd >= 4:
                    # blur^T, demodulation scale, range scale, phase split and f16 split in one pass, then the
                    # stride-2 conv as stride-1 taps on the four parity images
                    gp = ops.blurT_to_sform_phases(g_pre, self.k4x4_flip, d, mul2,
                                                   out=ops.sform_phases_scratch(B, L.cout, Hd, Hd, self.device))
                    dx, dot = ops.conv3x3(gp, L.wpk_bwd, L.cin, CONV_S2, out_scale=s, dotx=x_in, in_mul2=mul2, out=dx_out)
                else:
                    H2 = 2 * Hd + 1
                    P2 = (H2 + 3) // 4 * 4
                    g2 = ops.upfirdn2d(g_pre, self.k4x4_flip, pad=(2, 2), out_pitch=P2)
                    dx, dot = ops.conv3x3(g2, L.wpk_bwd, L.cin, CONV_S2, in_scale=d, out_scale=s, dotx=x_in, in_hw=(H2, H2),
                                          in_pitch=P2, in_mul2=mul2, out=dx_out)
                    del g2
            if dot is not None:
                gs_all[:, L.row:L.row + L.cin] += dot
            g_feat = dx
            del g_pre
        if jobs is not None:
            jobs.run(self.bwd_flag)         # four launches: partial sums, demodulation gradient, dot products, scale checks
        self.last_gs = gs_all
        if wrt == 'styles':
            return gs_all
        return ops.style_affine_backward(gs_all, self.wcat, self.lat_start, self.n_latent, grad_div=grad_scale)


_SIDE = {}


def _side_streams(device, n):
    """The same n side streams on every call: the caching allocator's pools and the S-form scratch buffers are keyed by
    stream, so fresh streams per inversion would mean fresh (synchronising) device allocations inside every inversion."""
    pool = _SIDE.setdefault(str(device), [])
    while len(pool) < n:
        pool.append(torch.cuda.Stream(device=device))
    return pool[:n]


# Concurrent sub-batches (streams > 1): the 8-wave stride-1 kernel from 64 work items instead of 128.  A sub-batch of four images brings 64 items
# to the 32² layers; on the 8-wave kernel they occupy 64 CUs for a short time and leave the rest of the chip to the other stream's launch, the
# 4-wave ring kernel it replaces spreads 256 small workgroups over every CU.  Measured (bench.py, 2 streams, three boxes): 6.97-6.99 -> 7.10-7.16
# img/s; on ONE stream (batch 8) the lower threshold moves the 16² layers and costs 1.3 % — hence only here (LABNOTES.md §14.6).
MULTI_STREAM_S1_BIG_MIN_ITEMS = int(os.environ.get('OODGAN_MULTI_STREAM_S1_BIG_MIN_ITEMS', '64'))
_S1_BIG_DEFAULT = 128

_FLAG = {}
_PLAN_POOLS = {}


def _plan_pool(device, batch):
    """The private allocator pool a launch plan is recorded under, ONE per (device, stream, batch size) for the life of the process: the buffers a
    recorded step touched keep their addresses while the plan lives, and the next inversion's recording reuses the same blocks (a fresh pool per
    inversion hands ~5 GB back to the driver and takes it again: 35 ms per inversion of 8, measured).  Per batch size: a step of ONE image recorded
    into blocks a batch of 8 left behind ran 2.6x slower (724 against 274 ms per inversion, tools/plan_pool_probe.py) — its tensors are then carved out
    of a few multi-GB segments instead of sized segments."""
    if os.environ.get('OODGAN_PLAN_POOL_CACHE', '1') == '0':
        return torch.cuda.MemPool()
    key = (str(device), ops._stream_handle(), int(batch))
    pool = _PLAN_POOLS.get(key)
    if pool is None:
        pool = _PLAN_POOLS[key] = torch.cuda.MemPool()
    return pool


def _flag_stream(device):
    """The stream the range flags are read on (one per device): a 4-byte device-to-host copy behind an event of the compute stream."""
    st = _FLAG.get(str(device))
    if st is None:
        st = _FLAG[str(device)] = torch.cuda.Stream(device=device)
    return st


class _WRun:
    """One (sub-)batch of the W+ loop on one HIP stream, advanced one step per ``advance()``.  A step is forward, ``_loss_grad`` (the one
    place that knows the loss terms), backward, Adam; its step index lives on the device (``dev_t``), so every step is the same launch
    list, ``_eager_step``, however it is run.  ``replay`` says how: None — every step from Python; 'plan' — recorded into a launch plan
    (oodgan_plan_*) while it runs, then one oodgan_plan_run call per step; 'graph' — captured into a hipGraph and replayed (``_record``).

    Range guard (round 6): the carried forward / backward range scales raise sticky device flags when a tensor's range
    moved by more than the format's head-room within one step (range control).  Until round 5 the flags were read after the last
    step and the WHOLE inversion repeated with exact per-step scales.  Now, every ``check_every`` steps, (w, m, v, t) is snapshotted and the
    two flags are copied to pinned host memory on a side stream behind an event of the compute stream — no synchronisation of the compute
    stream; ``check_lag`` steps later (the copy has long finished: the host runs ahead of the GPU) the host looks at them.  Clear: the
    snapshot becomes the last clean state.  Set: the run goes back to the last clean state, repeats that window (<= check_every steps)
    with exact scales, and continues in carry mode from freshly measured scales.  A captured step cannot change its arithmetic mid-run: a
    graph run has no guard, ``WPlusInverter._invert_runs`` reads the flags once at its end and repeats a flagged inversion through the guard.

    Projector schedule: the learning-rate factor, the latent noise and its strength are functions of ``dev_t`` (and of the
    run's constants: seed, image ids, ``steps``) evaluated inside the kernels — a rollback, which restores (w, m, v, t), needs nothing new: a
    repeated window draws the same noise and takes the same learning rates."""

    def __init__(self, inv, eng, target, w0, noises, steps, stream, keep_traj, replay, beta=None, ids=None, anchor=None, f0=None, pn=None,
                 px=None, ml0=None, th0=None, c0=None):
        self.inv, self.eng, self.stream, self.steps = inv, eng, stream, steps
        self.target, self.noises = target, noises
        # colour map: a leaf beside the latents — theta (B,12) = (M, b) from ``c0``, its moments, the gradient Adam consumed,
        # the float and double partial sums of the fused term and the buffer it writes M^T g into.  All persistent and born here, never
        # inside a recorded step (see ``replay`` below); ``color_reg`` brings a loss table
        self.ct = self.ctm = self.ctv = self.ctg = self.cparts = self.cgimg = self.co_table = None
        if c0 is not None:
            self.ct = c0.detach().clone().contiguous()
            self.ctm, self.ctv, self.ctg = (torch.zeros_like(self.ct) for _ in range(3))
            self.cparts = ops.color_parts(self.ct.shape[0], target.shape[-2], target.shape[-1], target.device)
            self.cgimg = torch.empty_like(target, memory_format=torch.contiguous_format)
            if inv.color_reg != 0.0:
                self.co_table = torch.zeros(steps, self.ct.shape[0], device=self.ct.device, dtype=torch.float32)
        # similarity alignment: a leaf beside the latents — theta (B,4) from ``th0``, its moments and the gradient Adam consumed.
        # ``src`` keeps the photograph; ``target`` becomes the buffer x_theta the warp rewrites in front of every forward, so that
        # ``_loss_grad`` reads it where it read the photograph (with ``pixel_size`` the pooled target below is re-made from it every step as
        # well).  All persistent and born here, never inside a recorded step (see ``replay`` below); ``align_reg`` brings a loss table
        self.src = self.th = self.thm = self.thv = self.thg = self.apart = self.al_table = None
        if th0 is not None:
            self.src = target.contiguous()
            self.target = target = torch.empty_like(self.src)
            self.th = th0.detach().clone().contiguous()
            self.thm, self.thv, self.thg = (torch.zeros_like(self.th) for _ in range(3))
            self.apart = ops.align_grad_parts(self.th.shape[0], self.src.shape[-2], self.src.shape[-1], self.src.device)
            ops.similarity_warp(self.src, self.th, out=self.target)       # what the set-up below pools: every step warps again
            if inv.align_reg != 0.0:
                self.al_table = torch.zeros(steps, self.th.shape[0], device=self.th.device, dtype=torch.float32)
        # masked objective: the per-image loss weight plane (B,1,S,S), a persistent input like ``target`` (a recorded step
        # replays it unchanged; a rollback needs nothing new: it is constant for the run); None = the plain per-image MSE
        self.beta = beta
        # StyleSpace: the latents stay at their start, a persistent input like ``target``; the optimised state is the offset
        # on the styles, (B, R), from 0.  It keeps the name ``w``: snapshots, rollback, trajectory and gathering work on it unchanged
        self.sspace = inv.latent_space == 's'
        self.w0 = w0.detach().clone().contiguous() if self.sspace else None
        self.w = torch.zeros(w0.shape[0], eng.R, device=w0.device, dtype=torch.float32) if self.sspace else w0.detach().clone().contiguous()
        self.m, self.v = torch.zeros_like(self.w), torch.zeros_like(self.w)
        self.gmul = ops.loss_scale_for(target.numel() // target.shape[0])
        # the step index twice: ``t`` for the host's control flow, ``dev_t`` on the device for the step's kernels — the row of the loss tables
        # and Adam's bias corrections — so that a step is the same launch list for every t, recorded or driven from Python
        self.t = 0
        self.dev_t = torch.zeros(1, dtype=torch.int32, device=self.w.device)
        self.lbuf = torch.empty(steps, self.w.shape[0], device=self.w.device, dtype=torch.float32)
        # optional LPIPS(alex) term (oodgan/lpips.py): the target's normalised taps once, a second loss table
        self.lp = inv.lpips if (inv.lpips is not None and inv.lpips_weight != 0.0) else None
        # ``lpips_size``: the term on the area-pooled view, factor ``lp_f``; the pooled target's taps once, outside the step
        self.lp_f = inv._lpips_f if self.lp is not None else 1
        self.lp_target = self.lp.target_taps(target if self.lp_f == 1 else ops.area_pool(target.contiguous(), self.lp_f)) if self.lp is not None else None
        self.lp_table = torch.zeros(steps, self.w.shape[0], device=self.w.device, dtype=torch.float32) if self.lp is not None else None
        # ``pixel_size``: the pixel term on the area-pooled view, factor ``px_f``.  The pooled target is a persistent input like
        # ``target`` and ``lp_target``, made here, once: never born inside a recorded step (see ``replay`` below), and the step reads it
        # instead of the full target — with a loss weight the kernel pools beta*(G - x) from the full target and this stays None
        self.px_f = inv._pixel_f
        self.px_target = ops.area_pool(target.contiguous(), self.px_f) if (self.px_f > 1 and beta is None and px is None) else px
        # ``pixel_filter``: the view is the antialiased resize Ay · G · Ax^T instead of the area pool.  The two tap tables and
        # the target's view — the resized target, or the caller's own low-resolution ``pixel_target`` (``px``) — are persistent inputs too
        self.px_tables = None
        if inv.pixel_filter is not None:
            H, W = int(target.shape[-2]), int(target.shape[-1])
            self.px_tables = (ops.resample_tables(inv.pixel_filter, H, self.px_f).to(target.device),
                              ops.resample_tables(inv.pixel_filter, W, self.px_f).to(target.device))
            self.px_target = px if px is not None else ops.resample_view(target.contiguous(), *self.px_tables, self.px_f)
        # optional SSIM term (csrc/loss_ssim.hip): a third loss table, 1 - SSIM per step and image
        self.ss_table = torch.zeros(steps, self.w.shape[0], device=self.w.device, dtype=torch.float32) if inv.ssim_weight != 0.0 else None
        # projector schedule (csrc/wplus_sched.hip).  ``w_in``, the perturbed latent the generator reads, is a persistent
        # buffer like ``w``: born inside a recorded step it would be carved out of blocks the step's temporaries held (see ``replay`` below)
        self.ids = ids
        self.w_in = torch.empty_like(self.w) if inv.latent_noise != 0.0 else None
        # latent prior: latent_reg * mean (w - anchor)^2 per image, a fourth loss table; the anchor is constant for the run
        self.anchor = anchor
        self.lat_table = torch.zeros(steps, self.w.shape[0], device=self.w.device, dtype=torch.float32) if inv.latent_reg != 0.0 else None
        # latent controls: with any of them on, ops.latent_step takes the place of the Adam call.  The per-layer factors are a
        # persistent device buffer like ``w_in``, for the same reason: it must never be born inside a recorded step.  ``delta_reg`` brings a
        # fifth loss table, the squared spread of the layers about their mean per step and image
        self.tied = inv.latent_space == 'w'
        self.layer_lr = None if inv.layer_lr is None else torch.tensor(inv.layer_lr, dtype=torch.float32, device=self.w.device)
        self.dl_table = torch.zeros(steps, self.w.shape[0], device=self.w.device, dtype=torch.float32) if inv.delta_reg != 0.0 else None
        self.controls = self.tied or self.layer_lr is not None or self.dl_table is not None
        # ``style_reg`` brings a sixth loss table, mean_r delta_r^2 per step and image
        self.st_table = torch.zeros(steps, self.w.shape[0], device=self.w.device, dtype=torch.float32) if (self.sspace and inv.style_reg != 0.0) else None
        # feature offset: a second optimised state beside ``w`` — the offset ``f`` (B, C, h, h) from ``f0`` (zeros), its moments, the
        # buffer the backward writes dL/dx' into, the buffer x' = x + f is written to and the partial sums of the regulariser, all persistent
        # and born here, never inside a recorded step (see ``replay`` below); ``feature_reg`` brings a seventh loss table, mean f^2
        self.f = self.fm = self.fv = self.fg = self.fx = self.fpart = self.ft_table = None
        if inv.feature_layer is not None:
            self.f = f0.detach().clone().contiguous()
            self.fm, self.fv, self.fg, self.fx = (torch.zeros_like(self.f) for _ in range(4))
            if inv.feature_reg != 0.0:
                self.ft_table = torch.zeros(steps, self.w.shape[0], device=self.w.device, dtype=torch.float32)
                self.fpart = ops.feature_step_parts(self.f.shape[0], self.f.numel() // self.f.shape[0], self.f.device)
        # P_N+ prior: pn_reg * mean_{l,d} q^T M q per image, q = l5(w) - mu, an eighth loss table; the statistics are constant for
        # the run and shared by the sub-batches, the per-row partial sums a persistent buffer born here, never inside a recorded step
        self.pn = pn
        self.pn_table = torch.zeros(steps, self.w.shape[0], device=self.w.device, dtype=torch.float32) if inv.pn_reg != 0.0 else None
        self.pn_part = ops.pn_prior_parts(self.w.shape[0], self.w.shape[1], self.w.device) if self.pn_table is not None else None
        # fitted mask: a third optimised state — the logits ``ml`` (B,1,m,m) from ``ml0``, their moments, the gradient Adam
        # consumed, the mask a = sigmoid(ml), its enlargement ``beta`` (the loss weight of this run, rewritten by every step), the plane
        # e = dL/dbeta, the per-image means and the two tables of the regulariser: all persistent and born here, never inside a recorded step
        self.ml = self.mm = self.mv = self.mg = self.ma = self.me = self.mstat = self.ma_table = self.mb_table = None
        if ml0 is not None:
            Bm, S = self.w.shape[0], int(target.shape[-1])
            self.ml = ml0.detach().clone().contiguous()
            self.mm, self.mv, self.mg, self.ma = (torch.zeros_like(self.ml) for _ in range(4))
            self.beta, self.me = (torch.empty(Bm, 1, S, S, device=self.w.device, dtype=torch.float32) for _ in range(2))
            self.mstat = ops.maskfit_stat(Bm, self.w.device)
            self.ma_table, self.mb_table = (torch.zeros(steps, Bm, device=self.w.device, dtype=torch.float32) for _ in range(2))
        self.traj = [None] * steps if keep_traj else None
        self.mode0 = (eng.fused_bwd, eng.carry_range)            # what the caller asked for (tests run the exact loop on purpose)
        self.guard = (eng.fused_bwd or eng.carry_range) and inv.check_every > 0 and replay != 'graph'
        self.clean = (0, self.w.clone(), None, None, self._fsnap(), self._msnap(), self._asnap(), self._csnap()) if self.guard else None     # m = v = 0 at t = 0
        self.pending, self.exact_until = None, 0
        self.steps_run = 0                                       # forward/backward pairs enqueued, repeated windows included
        self.rollbacks = 0
        self.host = inv._pinned(len(inv._runs)) if self.guard else None
        inv._runs.append(self)
        # launch plan (round 6): the first step measures exact scales (its own launch sequence); the second — the first
        # steady-state step — runs from Python as well: it CREATES the persistent scratch buffers only the carried-scale path uses (pooled
        # S-forms with a zero border, hi-only record buffers, max slots).  Created inside the recording they would be carved out of blocks
        # that temporaries of the same step held earlier, and on every replay those temporaries' kernels would write over them — borders
        # included (seen as NaN from the second replay on).  The third step is RECORDED while it runs (oodgan_plan_*, under a private
        # allocator pool so that every buffer it touched keeps its address); every later step is one oodgan_plan_run call instead of ~100
        # ctypes calls and the Python between them.  A hipGraph is captured under a pool of its own, which no step before it has touched:
        # there the second step is the captured one
        if replay == 'plan' and (keep_traj or not eng.sform):       # the trajectory's per-step w.clone() is a torch kernel outside the plan
            replay = None
        self.replay, self.warmup = replay, 1 if replay == 'graph' else 2
        self.plan, self.pool, self.eager_left, self.plan_steps, self.plan_size = None, None, self.warmup, 0, 0

    # ---- one W+ step on the current stream
    def _eager_step(self):
        eng, inv = self.eng, self.inv
        if self.sspace:
            # forward at style_affine(w0) + delta, the loss as ever, backward down to the styles — the contraction to dL/dW+ does not run, the
            # step is one launch shorter than the W+ step — and the division by the loss scale, the regulariser and Adam in one kernel
            img = eng.forward(self.w0, self.noises, save=True, range_mode='carry', style_offsets=self.w)
            gimg = self._loss_grad(img)
            gs = eng.backward(gimg, self.gmul, carry_scale=True, wrt='styles')
            ops.style_step(self.w, gs, self.m, self.v, self.dev_t, self.steps, inv.lr_rampup, inv.lr_rampdown, inv.lr, inv.betas, inv.eps,
                           grad_div=self.gmul, row_lat=eng.row_lat if self.layer_lr is not None else None, layer_lr=self.layer_lr,
                           style_reg=inv.style_reg, table=self.st_table)
            return
        w_in = self.w
        if self.w_in is not None:
            # W: one vector of noise per image, repeated over the layers — the rows of w_in stay identical
            w_in = ops.latent_noise(self.w, self.dev_t, self.ids, self.steps, inv.latent_noise, inv.noise_ramp, inv.noise_seed, out=self.w_in,
                                    period=self.w.shape[-1] if self.tied else None)
        if self.ml is not None:
            # the fitted mask as a third leaf: a = sigmoid(ml) and beta = U(a) once per step, in front of the forward; ``_loss_grad`` leaves
            # dL/dbeta in ``me``; the mask's side of the step stands BEFORE the latent-side call, which increments the counter both read
            ops.maskfit_expand(self.ml, int(self.target.shape[-1]), a=self.ma, beta=self.beta)
            img = eng.forward(w_in, self.noises, save=True, range_mode='carry')
            gimg = self._loss_grad(img)
            g = eng.backward(gimg, self.gmul, carry_scale=True)
            ops.maskfit_step(self.ml, self.mg, self.mm, self.mv, self.ma, self.me, self.dev_t, self.steps, inv.lr_rampup, inv.lr_rampdown,
                             inv.mask_lr, inv.betas, inv.eps, grad_div=self.gmul, area=inv.mask_area, area_weight=inv.mask_area_weight,
                             binary_weight=inv.mask_binary_weight, area_table=self.ma_table, binary_table=self.mb_table, stat=self.mstat)
        elif self.th is not None:
            # the alignment as a second leaf: the photograph is warped by theta into ``target`` (and pooled into ``px_target``) in front of the
            # forward, the loss and the backward are the plain step's, and dL/dtheta is read off the image gradient the step computed
            # anyway; its side of the step stands BEFORE the latent-side call, which increments the counter both read
            ops.similarity_warp(self.src, self.th, out=self.target)
            if self.px_f > 1:
                ops.area_pool(self.target, self.px_f, out=self.px_target)
            img = eng.forward(w_in, self.noises, save=True, range_mode='carry')
            gimg = self._loss_grad(img)
            g = eng.backward(gimg, self.gmul, carry_scale=True)
            ops.align_grad_step(gimg, self.src, self.th, self.thg, self.thm, self.thv, self.dev_t, self.steps, inv.lr_rampup, inv.lr_rampdown,
                                inv.align_lr, inv.betas, inv.eps, grad_div=self.gmul, align_reg=inv.align_reg, table=self.al_table,
                                part=self.apart)
        elif self.ct is not None:
            # the colour map as a second leaf: forward and backward are the plain step's, ``_loss_grad`` takes the pixel term on M G + b in
            # one fused pass that hands M^T g to the backward and leaves the sums of dL/dtheta; its side of the step is one launch, placed
            # BEFORE the latent-side call, which increments the counter both read
            img = eng.forward(w_in, self.noises, save=True, range_mode='carry')
            gimg = self._loss_grad(img)
            g = eng.backward(gimg, self.gmul, carry_scale=True)
            ops.color_step(self.ct, self.ctg, self.ctm, self.ctv, self.cparts[1], self.dev_t, self.steps, inv.lr_rampup, inv.lr_rampdown,
                           inv.color_lr, inv.betas, inv.eps, grad_div=self.gmul, kind=inv.color, color_reg=inv.color_reg, table=self.co_table)
        elif self.f is None:
            img = eng.forward(w_in, self.noises, save=True, range_mode='carry')
            gimg = self._loss_grad(img)
            g = eng.backward(gimg, self.gmul, carry_scale=True)
        else:
            # the same step with the offset as a second leaf: its gradient is the dx the backward computes at that layer anyway, its side
            # of the step one call placed BEFORE the latent-side call, which increments the counter both read
            img = eng.forward(w_in, self.noises, save=True, range_mode='carry', feature_offset=(inv.feature_layer, self.f), feature_out=self.fx)
            gimg = self._loss_grad(img)
            g = eng.backward(gimg, self.gmul, carry_scale=True, feature_grad=self.fg)
            ops.feature_step(self.f, self.fg, self.fm, self.fv, self.dev_t, self.steps, inv.lr_rampup, inv.lr_rampdown, inv.feature_lr,
                             inv.betas, inv.eps, grad_div=self.gmul, feature_reg=inv.feature_reg, table=self.ft_table, part=self.fpart)
        if self.lat_table is not None:          # evaluated at w, not at the perturbed w_in
            ops.latent_prior_loss_grad(self.w, self.anchor, g, inv.latent_reg, table=self.lat_table, row_dev=self.dev_t)
        if self.pn_table is not None:           # at the unperturbed w as well; into the true gradient, before the W tie and the step
            ops.pn_prior_loss_grad(self.w, self.pn.mean, self.pn.matrix, g, inv.pn_reg, table=self.pn_table, row_dev=self.dev_t, part=self.pn_part)
        if self.controls:                       # spread term, W tie, per-layer step sizes and Adam: one kernel, the launch count of the Adam call
            ops.latent_step(self.w, g, self.m, self.v, self.dev_t, self.steps, inv.lr_rampup, inv.lr_rampdown, inv.lr, inv.betas, inv.eps,
                            layer_lr=self.layer_lr, delta_reg=inv.delta_reg, tied=self.tied, table=self.dl_table)
        elif inv.lr_rampup > 0.0 or inv.lr_rampdown > 0.0:
            ops.adam_step_dev_sched(self.w, g, self.m, self.v, self.dev_t, self.steps, inv.lr_rampup, inv.lr_rampdown, inv.lr, inv.betas, inv.eps)
        else:
            ops.adam_step_dev(self.w, g, self.m, self.v, self.dev_t, inv.lr, inv.betas, inv.eps)

    def _loss_grad(self, img):
        """The loss of the step, each term's values to row dev_t of its table, and gmul * d(sum_b loss_b)/d(img).  The terms in the order
        they accumulate into the gradient: the pixel term (the MSE, or the robust term ``pixel_loss`` names) writes it, LPIPS and 1 - SSIM add
        lambda * gmul * their part; with ``lpips_size`` LPIPS is taken on the area-pooled view of the same image.  With a loss weight beta
        the terms are taken on the composite c: alone, the composite MSE writes beta*dL/dc in one kernel; with LPIPS or
        SSIM it writes dL/dc and c, they add to it, and beta is applied once afterwards.  With ``pixel_size`` the pixel term is the fused
        kernel of the pooled view: the same call, the same number of launches, a full-resolution gradient and composite; with
        ``pixel_filter`` the kernel pair of the antialiased view: the same call again, one launch more.  With a fitted mask
         the pixel term always writes dL/dc (and c only if LPIPS or SSIM reads it), and ``maskfit_chain`` takes the place of
        ``scale_by_plane``: the same pass also leaves dL/dbeta = sum_c dL/dc_c (G_c - x_c) in ``me``, whatever terms added to dL/dc."""
        inv, gmul, row = self.inv, self.gmul, self.dev_t
        if self.ct is not None:                 # the fused term of the colour map in the pixel term's place (no other term goes with it)
            _, gimg, _ = ops.color_pixel_loss_grad(img, self.target, self.ct, inv.pixel_loss, inv.pixel_scale, self.beta, gmul, table=self.lbuf,
                                                   row_dev=row, parts=self.cparts, out=self.cgimg)
            return gimg
        fit = self.ml is not None
        on_c = self.beta is not None and (self.lp is not None or self.ss_table is not None)
        _, gimg, c = ops.pixel_loss_grad(img, self.target, inv.pixel_loss, inv.pixel_scale, self.beta, gmul, wrt='composite' if (on_c or fit) else 'gen',
                                         composite=on_c, table=self.lbuf, row_dev=row, pool=self.px_f, target_pooled=self.px_target,
                                         resample=self.px_tables)
        x = c if on_c else img
        if self.lp is not None and self.lp_f == 1:
            self.lp.loss_and_grad(x, gimg, inv.lpips_weight * gmul, table=self.lp_table, row_dev=row, target_taps=self.lp_target)
        elif self.lp is not None:               # on the pooled view: pool (and zero the small gradient), the term there, unpool-add
            xs, gs = ops.area_pool(x, self.lp_f, grad_buffer=True)
            self.lp.loss_and_grad(xs, gs, inv.lpips_weight * gmul, table=self.lp_table, row_dev=row, target_taps=self.lp_target)
            ops.area_pool_bwd_add(gs, gimg, self.lp_f)
        if self.ss_table is not None:
            ops.ssim_loss_grad(x, self.target, gimg, inv.ssim_weight * gmul, table=self.ss_table, row_dev=row)
        if fit:
            ops.maskfit_chain(gimg, img, self.target, self.beta, e=self.me)
        elif on_c:
            ops.scale_by_plane(gimg, self.beta)
        return gimg

    def _record(self):
        """Perform the step and keep it in ``self.plan``: a launch plan, recorded while the step runs, or a captured hipGraph."""
        if self.replay == 'graph':
            self.stream.synchronize()
            self.plan = torch.cuda.CUDAGraph()
            with torch.cuda.graph(self.plan, stream=self.stream):
                self._eager_step()
            self.inv._graphs.append(self.plan)      # replays are still in flight when ``invert`` returns
            self.plan.replay()                      # a capture only captures
        else:
            plan, pool = ops.LaunchPlan(), _plan_pool(self.w.device, self.w.shape[0])
            with torch.cuda.use_mem_pool(pool):
                with plan.recording():
                    self._eager_step()
            self.plan, self.pool, self.plan_size = plan, pool, plan.size

    def _step(self):
        eng = self.eng
        if self.plan is not None:
            self.plan.replay() if self.replay == 'graph' else self.plan.run()
            self.plan_steps += 1
        elif self.replay and self.eager_left == 0 and (self.replay == 'graph' or (
                not self.exact_until and eng.fused_bwd and eng.carry_range and self.steps - self.t >= 3)):
            self._record()
        else:
            self._eager_step()
            self.eager_left = max(0, self.eager_left - 1)
        self.t += 1
        self.steps_run += 1
        if self.traj is not None:
            self.traj[self.t - 1] = self.w.clone()
        if self.inv.on_step is not None:
            self.inv.on_step(self)

    def _fsnap(self):
        """(f, fm, fv) as they stand, for a snapshot; None without a feature offset."""
        return None if self.f is None else (self.f.clone(), self.fm.clone(), self.fv.clone())

    def _msnap(self):
        """(ml, mm, mv) as they stand, for a snapshot; None without a fitted mask."""
        return None if self.ml is None else (self.ml.clone(), self.mm.clone(), self.mv.clone())

    def _asnap(self):
        """(th, thm, thv) as they stand, for a snapshot; None without an alignment."""
        return None if self.th is None else (self.th.clone(), self.thm.clone(), self.thv.clone())

    def _csnap(self):
        """(ct, ctm, ctv) as they stand, for a snapshot; None without a colour map."""
        return None if self.ct is None else (self.ct.clone(), self.ctm.clone(), self.ctv.clone())

    def _post_check(self):
        eng = self.eng
        snap = (self.t, self.w.clone(), self.m.clone(), self.v.clone(), self._fsnap(), self._msnap(), self._asnap(), self._csnap())
        ev = torch.cuda.Event()
        ev.record()
        side, done = _flag_stream(self.w.device), torch.cuda.Event()
        self.host.zero_()
        with torch.cuda.stream(side):
            side.wait_event(ev)
            if eng.bwd_flag is not None:
                self.host[0:1].copy_(eng.bwd_flag, non_blocking=True)
            if eng.fwd_range is not None:
                self.host[1:2].copy_(eng.fwd_range.flag, non_blocking=True)
            done.record(side)
        self.pending = (snap, done)

    def _resolve(self):
        """Look at the flags of the pending check; True if the run was rolled back."""
        snap, done = self.pending
        self.pending = None
        done.synchronize()
        if int(self.host[0]) == 0 and int(self.host[1]) == 0:
            self.clean = snap
            return False
        eng = self.eng
        t0, w, m, v, fs, ms, als, cs = self.clean
        self.w.copy_(w)
        if m is None:
            self.m.zero_()
            self.v.zero_()
        else:
            self.m.copy_(m)
            self.v.copy_(v)
        if fs is not None:                                       # the offset and its moments go back with the latents'
            for dst, src in zip((self.f, self.fm, self.fv), fs):
                dst.copy_(src)
        if ms is not None:                                       # ... and the mask's logits and theirs
            for dst, src in zip((self.ml, self.mm, self.mv), ms):
                dst.copy_(src)
        if als is not None:                                      # ... and the alignment and its moments
            for dst, src in zip((self.th, self.thm, self.thv), als):
                dst.copy_(src)
        if cs is not None:                                       # ... and the colour map and its moments
            for dst, src in zip((self.ct, self.ctm, self.ctv), cs):
                dst.copy_(src)
        self.t = t0
        self.dev_t.fill_(t0)
        self.rollbacks += 1
        self.plan = None                                         # the carried state it points to is rebuilt: recorded again after the window
        eng.fused_bwd = eng.carry_range = False                  # exact per-step scales, both directions, for the flagged window
        eng.reset_bwd_state()
        eng.reset_fwd_state()
        self.exact_until = snap[0]
        return True

    def _leave_exact(self):
        eng = self.eng
        eng.fused_bwd, eng.carry_range = self.mode0
        eng.reset_bwd_state()                                    # the next step measures its scales exactly, like the first of a run
        eng.reset_fwd_state()
        self.exact_until = 0
        self.eager_left = self.warmup
        self.clean = (self.t, self.w.clone(), self.m.clone(), self.v.clone(), self._fsnap(), self._msnap(), self._asnap(), self._csnap())

    def _advance(self):
        if self.t < self.steps:
            self._step()
            if self.exact_until:
                if self.t == self.exact_until:
                    self._leave_exact()
            elif self.guard and (self.t % self.inv.check_every == 0 or self.t == self.steps):
                if self.pending is not None and self._resolve():     # (only when the last step follows a check within the lag)
                    return
                self._post_check()
        if self.pending is not None and (self.t >= self.pending[0][0] + self.inv.check_lag or self.t >= self.steps):
            self._resolve()

    def advance(self):
        """Enqueue the next step (or resolve a check / roll back); False once the run is complete and verified."""
        if self.done():
            return False
        with torch.cuda.stream(self.stream):        # None: the caller's stream
            self._advance()
        return not self.done()

    def done(self):
        return self.t >= self.steps and self.pending is None

    def close(self):
        self.eng.fused_bwd, self.eng.carry_range = self.mode0
        self.eng.saved = None
        self.plan = None            # before the pool it points into
        self.pool = None


def check_nonneg(value, name='ssim_weight'):
    """The option ``name`` (a loss weight, a ramp fraction, a noise strength) as a float; ValueError unless it is a finite number >= 0."""
    try:
        w = float(value)
    except (TypeError, ValueError):
        raise ValueError(f'{name} must be a finite number >= 0, got {value!r}') from None
    if not (math.isfinite(w) and w >= 0.0):
        raise ValueError(f'{name} must be a finite number >= 0, got {value!r}')
    return w


check_ssim_weight = check_nonneg       # the name it had while the SSIM weight was its only caller


LPIPS_POOL_FACTORS = (1, 2, 4, 8, 16)      # 1: full resolution; the others: the factors of csrc/loss_pool.hip
LPIPS_MIN_SIZE = 64                         # the smallest size the HIP AlexNet stack is pinned at (tests/test_hip_lpips.py)


def check_lpips_size(value, image_size=None, name='lpips_size'):
    """The size LPIPS is taken at (None: the image's own): ValueError unless it is None or an int (not a bool) >= LPIPS_MIN_SIZE and, once the
    image size is known, <= it, a divisor of it, with a quotient in LPIPS_POOL_FACTORS.  Returns the value."""
    if value is None:
        return None
    if isinstance(value, bool) or not isinstance(value, int):
        raise ValueError(f'{name} must be None or an int, got {value!r}')
    if value < LPIPS_MIN_SIZE:
        raise ValueError(f'{name} must be >= {LPIPS_MIN_SIZE} (the smallest size the LPIPS stack is checked at), got {value!r}')
    if image_size is not None and (value > image_size or image_size % value != 0 or image_size // value not in LPIPS_POOL_FACTORS):
        raise ValueError(f'{name} must divide the image size {image_size} by one of {list(LPIPS_POOL_FACTORS)}, got {value!r}')
    return value


PIXEL_POOL_FACTORS = (1, 2, 4, 8, 16)      # 1: full resolution; the others: the factors of the pooled pixel kernel (csrc/loss_pixel.hip)


def check_pixel_size(value, image_size=None, name='pixel_size'):
    """The size the pixel term is taken at (None: the image's own): ValueError unless it is None or a positive int (not a bool) and, once the
    image size is known, a divisor of it with a quotient in PIXEL_POOL_FACTORS — the only lower bound.  Returns the value, None for the
    image's own size (factor 1: today's path)."""
    if value is None:
        return None
    if isinstance(value, bool) or not isinstance(value, int):
        raise ValueError(f'{name} must be None or an int, got {value!r}')
    if value < 1:
        raise ValueError(f'{name} must be positive, got {value!r}')
    if image_size is not None:
        if value > image_size or image_size % value != 0 or image_size // value not in PIXEL_POOL_FACTORS:
            raise ValueError(f'{name} must divide the image size {image_size} by one of {list(PIXEL_POOL_FACTORS)}, got {value!r}')
        if value == image_size:
            return None
    return value


PIXEL_FILTERS = ('box',) + tuple(ops.RESAMPLE_FILTERS)


def check_pixel_filter(value, name='pixel_filter'):
    """The filter of the view the pixel term is taken on with ``pixel_size``: ValueError unless it is None or one of
    PIXEL_FILTERS.  Returns None for None and 'box' (the area pool of §20: today's path), else the name."""
    if value is None or (isinstance(value, str) and value == 'box'):
        return None
    if not isinstance(value, str) or value not in PIXEL_FILTERS:
        raise ValueError(f'{name} must be None or one of {list(PIXEL_FILTERS)}, got {value!r}')
    return value


def check_pixel_target(value, target, pixel_size, name='pixel_target'):
    """``pixel_target``, the caller's own low-resolution target of the pixel term: ValueError unless it is None or a float32 (B,C,n,n*W/H)
    tensor on the target's device with H / n in PIXEL_POOL_FACTORS above 1; it fixes ``pixel_size`` = n, so a ``pixel_size`` that differs is
    an error.  Returns (the tensor, contiguous, or None; the pixel_size in force)."""
    if value is None:
        return None, pixel_size
    B, C, H, W = target.shape
    if not isinstance(value, torch.Tensor) or value.dtype != torch.float32 or value.dim() != 4 or value.device != target.device:
        raise ValueError(f'{name} must be a float32 (B,C,n,n) tensor on {target.device}')
    n, m = int(value.shape[-2]), int(value.shape[-1])
    if tuple(value.shape[:2]) != (B, C) or n < 1 or H % n != 0 or H // n not in PIXEL_POOL_FACTORS[1:] or m * (H // n) != W:
        raise ValueError(f'{name} must have shape ({B}, {C}, n, n) with {H} / n in {list(PIXEL_POOL_FACTORS[1:])}, got {tuple(value.shape)}')
    if pixel_size is not None and pixel_size != m:
        raise ValueError(f'{name} of size {m} fixes pixel_size = {m}, got pixel_size {pixel_size!r}')
    return value.contiguous(), m


PIXEL_LOSSES = ('mse',) + tuple(ops.ROBUST_KINDS)


def check_pixel_loss(pixel_loss, pixel_scale, name='pixel_loss', scale_name='pixel_scale'):
    """The pixel term of the W+ loss and its scale as (name, s): ValueError unless the name is one of PIXEL_LOSSES and the scale a finite real
    number > 0 (not a string, not a bool).  s is the scale rounded to float32, the value the kernel uses; its float32 square must be a normal
    number (about 1.1e-19 < s < 1.8e19), or d^2 + s^2 could be 0 or inf."""
    if not isinstance(pixel_loss, str) or pixel_loss not in PIXEL_LOSSES:
        raise ValueError(f'{name} must be one of {list(PIXEL_LOSSES)}, got {pixel_loss!r}')
    if isinstance(pixel_scale, bool) or not isinstance(pixel_scale, numbers.Real) or not (math.isfinite(pixel_scale) and pixel_scale > 0):
        raise ValueError(f'{scale_name} must be a finite number > 0, got {pixel_scale!r}')
    s = torch.tensor(float(pixel_scale), dtype=torch.float32)
    s2 = (s * s).item()
    if not (math.isfinite(s2) and s2 >= torch.finfo(torch.float32).tiny):
        raise ValueError(f'{scale_name} must have a normal float32 square (about 1.1e-19 < s < 1.8e19), got {pixel_scale!r}')
    return pixel_loss, s.item()


LATENT_SPACES = ('w+', 'w', 's')


def check_latent_space(value, name='latent_space'):
    """Where the W+ loop moves: 'w+' (default: every layer its own vector), 'w' (one vector per image) or 's' (StyleSpace: an offset on the
    per-channel styles, the latents fixed); anything else raises ValueError."""
    if not isinstance(value, str) or value not in LATENT_SPACES:
        raise ValueError(f'{name} must be one of {list(LATENT_SPACES)}, got {value!r}')
    return value


def check_layer_lr(value, n_layers=None, name='layer_lr'):
    """The per-layer factors of the learning rate as a tuple of floats (None stays None): ValueError unless it is a list / tuple of finite real
    numbers >= 0 (no bools, no strings) and, once the number of layers is known, of that length."""
    if value is None:
        return None
    if not isinstance(value, (list, tuple)) or len(value) == 0:
        raise ValueError(f'{name} must be None or a list of finite numbers >= 0, one per layer, got {value!r}')
    for f in value:
        if isinstance(f, bool) or not isinstance(f, numbers.Real) or not (math.isfinite(f) and f >= 0):
            raise ValueError(f'{name} must hold finite numbers >= 0, got {f!r} in {list(value)!r}')
    if n_layers is not None and len(value) != n_layers:
        raise ValueError(f'{name} must have one entry per layer ({n_layers}), got {len(value)}')
    return tuple(float(f) for f in value)


def check_latent_controls(latent_space, layer_lr, delta_reg, n_layers=None, prefix=''):
    """(latent_space, layer_lr, delta_reg) checked one by one and together: in W there is one vector per image, so per-layer rates mean
    nothing and the spread of the layers is identically zero — both raise ValueError there."""
    space = check_latent_space(latent_space, prefix + 'latent_space')
    rates = check_layer_lr(layer_lr, n_layers, prefix + 'layer_lr')
    reg = check_nonneg(delta_reg, prefix + 'delta_reg')
    if space == 'w' and rates is not None:
        raise ValueError(f"{prefix}layer_lr with {prefix}latent_space 'w': there is only one vector per image")
    if space == 'w' and reg != 0.0:
        raise ValueError(f"{prefix}delta_reg with {prefix}latent_space 'w': the layers are identical there, the term is zero")
    return space, rates, reg


def check_style_space(latent_space, style_reg, delta_reg=0.0, latent_noise=0.0, latent_reg=0.0, prefix=''):
    """``style_reg`` as a float, checked against the latent space: in 's' the latents do not move, so the terms and the noise that act on them
    (delta_reg, latent_noise, latent_reg) raise ValueError there, and ``style_reg`` raises it anywhere else."""
    reg = check_nonneg(style_reg, prefix + 'style_reg')
    if latent_space == 's':
        for value, name in ((delta_reg, 'delta_reg'), (latent_noise, 'latent_noise'), (latent_reg, 'latent_reg')):
            if check_nonneg(value, prefix + name) != 0.0:
                raise ValueError(f"{prefix}{name} with {prefix}latent_space 's': the latents stay at their start there, only the style offsets move")
    elif reg != 0.0:
        raise ValueError(f"{prefix}style_reg with {prefix}latent_space {latent_space!r}: the term acts on the style offsets of latent_space 's'")
    return reg


FEATURE_LAYERS = (3, 5, 7)       # the latents whose styled up-conv reads an 8², 16², 32² map (convs.2, convs.4, convs.6); 5: Feature-Style's index


def check_feature_layer(value, n_latent=None, name='feature_layer'):
    """The latent index whose styled up-conv receives the feature offset (None: no offset): ValueError unless it is None or an int (not a
    bool) in FEATURE_LAYERS and, once the generator is known, one of its ``n_latent`` latents.  From latent 9 on the conv below hands its
    output to the up-conv only as a fused S-form: there is no fp32 tensor to add to."""
    if value is None:
        return None
    if isinstance(value, bool) or not isinstance(value, int) or value not in FEATURE_LAYERS:
        raise ValueError(f'{name} must be None or one of {list(FEATURE_LAYERS)}, got {value!r}')
    if n_latent is not None and value > n_latent - 3:       # the up-convs read latents 1, 3, ..., n_latent - 3; the last latent only a ToRGB
        raise ValueError(f'{name} {value}: a generator with {n_latent} latents has no styled up-conv that reads it (its image is too small)')
    return value


def check_feature_offset(feature_layer, feature_lr, feature_reg, lr=None, latent_space='w+', prefix=''):
    """(feature_layer, feature_lr, feature_reg) checked one by one and together.  ``feature_lr`` None: ``lr`` (a choice, not a measured
    optimum); 0 is allowed and leaves the offset at zero.  Without a layer the other two must be off; latent_space 's' moves the styles of a
    fixed latent and does not take an offset."""
    layer = check_feature_layer(feature_layer, None, prefix + 'feature_layer')
    rate = None if feature_lr is None else check_nonneg(feature_lr, prefix + 'feature_lr')
    reg = check_nonneg(feature_reg, prefix + 'feature_reg')
    if layer is None:
        if rate is not None or reg != 0.0:
            raise ValueError(f'{prefix}feature_lr / {prefix}feature_reg without {prefix}feature_layer: there is no offset they could act on')
        return None, None, 0.0
    if latent_space == 's':
        raise ValueError(f"{prefix}feature_layer with {prefix}latent_space 's': the feature offset is optimised beside the latents of 'w+' or 'w'")
    if rate is None:
        rate = None if lr is None else float(lr)
    return layer, rate, reg


def check_pn(pn_reg, latent_space='w+', pn_stats=None, dim=None, device=None, need_stats=False, prefix=''):
    """``pn_reg`` as a float, checked against the latent space and, with ``need_stats`` (the call that runs the loop), against the statistics
    it reads.  ValueError, one place per refusal, naming the option: ``pn_reg`` not a finite number >= 0; ``pn_reg`` > 0 with latent_space 's'
    (the latents do not move there); ``pn_reg`` > 0 without ``pn_stats``; ``pn_stats`` that is not an ``oodgan.pn.PNStats`` whose ``mean``
    (dim,) and ``matrix`` (dim, dim) are float32 on ``device``.  With ``pn_reg`` 0 the statistics are not looked at."""
    reg = check_nonneg(pn_reg, prefix + 'pn_reg')
    if reg == 0.0:
        return reg
    if latent_space == 's':
        raise ValueError(f"{prefix}pn_reg with {prefix}latent_space 's': the latents stay at their start there, only the style offsets move")
    if not need_stats:
        return reg
    from .pn import PNStats
    if pn_stats is None:
        raise ValueError(f'{prefix}pn_reg > 0 needs {prefix}pn_stats: the statistics of the mapping network (Generator.pn_stats)')
    if not isinstance(pn_stats, PNStats):
        raise ValueError(f'{prefix}pn_stats must be an oodgan.pn.PNStats, got {type(pn_stats).__name__}')
    mean, matrix = pn_stats.mean, pn_stats.matrix
    d = int(mean.numel()) if dim is None else int(dim)
    if tuple(mean.shape) != (d,) or tuple(matrix.shape) != (d, d):
        raise ValueError(f'{prefix}pn_stats must hold a ({d},) mean and a ({d}, {d}) matrix for latents of {d} columns, got '
                         f'{tuple(mean.shape)} and {tuple(matrix.shape)}')
    if mean.dtype != torch.float32 or matrix.dtype != torch.float32:
        raise ValueError(f'{prefix}pn_stats must hold float32 tensors, got {mean.dtype} and {matrix.dtype}')
    if device is not None and (mean.device != torch.device(device) or matrix.device != torch.device(device)):
        raise ValueError(f'{prefix}pn_stats must be on {device} (PNStats.to), got {mean.device}')
    return reg


def check_pn_options(pn_reg, pn_samples=100000, pn_seed=0, pn_floor=0.0, latent_space='w+', prefix=''):
    """(pn_reg, pn_samples, pn_seed, pn_floor) checked one by one and against the latent space (``check_pn``): the sample count an int (not a
    bool) >= 2, the seed an integer in [0, 2^63), the relative floor of the variances a finite number >= 0.  ValueError names the option."""
    reg = check_pn(pn_reg, latent_space, prefix=prefix)
    if isinstance(pn_samples, bool) or not isinstance(pn_samples, int) or pn_samples < 2:
        raise ValueError(f'{prefix}pn_samples must be an int >= 2, got {pn_samples!r}')
    return reg, pn_samples, check_noise_seed(pn_seed, prefix + 'pn_seed'), check_nonneg(pn_floor, prefix + 'pn_floor')


MASK_SIZES = (16, 32, 64, 128, 256)          # the sizes m of the fitted mask


def _finite_real(value, name, what):
    if isinstance(value, bool) or not isinstance(value, numbers.Real) or not math.isfinite(value):
        raise ValueError(f'{name} must be {what}, got {value!r}')
    return float(value)


def check_mask_fit(mask_size=64, mask_lr=0.1, mask_area=0.30, mask_area_weight=5.0, mask_binary_weight=0.2, image_size=None, prefix=''):
    """The options of the fitted mask (loss_region='fit') as (m, lr, A, lambda_a, lambda_b): ValueError, naming the option,
    unless ``mask_size`` is an int (not a bool) in MASK_SIZES and, once the image size S is known, S / m is an integer >= 2; ``mask_lr`` a
    finite number > 0; ``mask_area`` a finite number in [0, 1]; the two weights finite numbers >= 0."""
    if isinstance(mask_size, bool) or not isinstance(mask_size, int) or mask_size not in MASK_SIZES:
        raise ValueError(f'{prefix}mask_size must be one of {list(MASK_SIZES)}, got {mask_size!r}')
    if image_size is not None and (image_size % mask_size != 0 or image_size // mask_size < 2):
        raise ValueError(f'{prefix}mask_size {mask_size} must divide the image size {image_size} by an integer >= 2')
    rate = _finite_real(mask_lr, prefix + 'mask_lr', 'a finite number > 0')
    if not rate > 0.0:
        raise ValueError(f'{prefix}mask_lr must be a finite number > 0, got {mask_lr!r}')
    area = _finite_real(mask_area, prefix + 'mask_area', 'a finite number in [0, 1]')
    if not 0.0 <= area <= 1.0:
        raise ValueError(f'{prefix}mask_area must be a finite number in [0, 1], got {mask_area!r}')
    wa = _finite_real(mask_area_weight, prefix + 'mask_area_weight', 'a finite number >= 0')
    wb = _finite_real(mask_binary_weight, prefix + 'mask_binary_weight', 'a finite number >= 0')
    if wa < 0.0 or wb < 0.0:
        raise ValueError(f'{prefix}mask_area_weight / {prefix}mask_binary_weight must be finite numbers >= 0, got {mask_area_weight!r}, {mask_binary_weight!r}')
    return mask_size, rate, area, wa, wb


def check_mask_init(value, B=None, m=None, device=None, name='mask_init'):
    """``mask_init``, the start of beta: a float in (0, 1) (not a bool), the string 'blend', or a float32 (B,1,m,m) tensor on ``device``
    (shape and device are checked once they are known; its values, which must lie in [0, 1], by ``mask_logits``).  ValueError otherwise."""
    if isinstance(value, torch.Tensor):
        if value.dtype != torch.float32 or value.dim() != 4:
            raise ValueError(f'{name} tensor must be a float32 (B,1,m,m) tensor, got {value.dtype} {tuple(value.shape)}')
        if B is not None and (tuple(value.shape) != (B, 1, m, m) or value.device != torch.device(device)):
            raise ValueError(f'{name} tensor must be float32 of shape {(B, 1, m, m)} on {device}, got {tuple(value.shape)} on {value.device}')
        return value
    if isinstance(value, str):
        if value != 'blend':
            raise ValueError(f"{name} must be a float in (0, 1), 'blend' or a (B,1,m,m) tensor, got {value!r}")
        return value
    v = _finite_real(value, name, "a float in (0, 1), 'blend' or a (B,1,m,m) tensor")
    if not 0.0 < v < 1.0:
        raise ValueError(f'{name} must lie in (0, 1), got {value!r}')
    return v


MASK_INIT_CLIP = 1e-3


def mask_logits(a0, name='mask_init'):
    """The start logits of the fitted mask from a start mask a0 (B,1,m,m) with values in [0, 1] (ValueError otherwise; NaN fails): clipped
    to [MASK_INIT_CLIP, 1 - MASK_INIT_CLIP], then log(a / (1 - a)).  Set-up, not the step."""
    lo, hi = torch.aminmax(a0)
    if not (lo.item() >= 0.0 and hi.item() <= 1.0):
        raise ValueError(f'{name} values must lie in [0, 1], got [{lo.item()}, {hi.item()}]')
    a = a0.detach().clamp(MASK_INIT_CLIP, 1.0 - MASK_INIT_CLIP)
    return torch.log(a / (1.0 - a)).contiguous()


def refuse_mask_fit(use_graph=False, pixel_size=None, pixel_filter=None, pixel_target=None, latent_space='w+', feature_layer=None, padded=False):
    """What the fitted mask (loss_region='fit') does not go with, refused in this one place before anything is launched."""
    for on, what in ((use_graph, 'use_graph'), (pixel_size is not None, 'pixel_size'), (pixel_filter is not None, 'pixel_filter'),
                     (pixel_target is not None, 'pixel_target'), (latent_space == 's', "latent_space 's'"),
                     (feature_layer is not None, 'feature_layer'),
                     (padded, 'a generator whose channel counts are zero-padded to multiples of 16')):
        if on:
            raise NotImplementedError(f"loss_region='fit' with {what}: the fitted mask is built for the full-resolution pixel term of the 'w+' / 'w' loop under launch plans")


ALIGN_KINDS = ('similarity',)        # the alignments the W+ loop fits beside the latents


def check_align(align=None, align_lr=0.001, align_reg=0.0, prefix=''):
    """The options of the fitted alignment as (align, align_lr, align_reg): ValueError, naming the option, unless ``align`` is
    None or one of ALIGN_KINDS, ``align_lr`` a finite number >= 0 (0 keeps theta at its start: the run then is the plain run on the target
    warped once) and ``align_reg`` a finite number >= 0.  Without ``align`` the other two are not looked at."""
    if align is None:
        return None, 0.001, 0.0
    if not isinstance(align, str) or align not in ALIGN_KINDS:
        raise ValueError(f'{prefix}align must be None or one of {list(ALIGN_KINDS)}, got {align!r}')
    rate = _finite_real(align_lr, prefix + 'align_lr', 'a finite number >= 0')
    reg = _finite_real(align_reg, prefix + 'align_reg', 'a finite number >= 0')
    if rate < 0.0 or reg < 0.0:
        raise ValueError(f'{prefix}align_lr / {prefix}align_reg must be finite numbers >= 0, got {align_lr!r}, {align_reg!r}')
    return align, rate, reg


def check_align_init(value, B=None, device=None, name='align_init'):
    """``align_init``, the start of theta: None (the identity) or a float32 (B, 4) tensor of finite values — (log-scale, rotation in radians,
    tx, ty) per image — on ``device`` (batch and device are checked once they are known).  ValueError otherwise."""
    if value is None:
        return None
    if not isinstance(value, torch.Tensor) or value.dtype != torch.float32 or value.dim() != 2 or value.shape[1] != 4:
        raise ValueError(f'{name} must be None or a float32 (B, 4) tensor (log-scale, rotation, tx, ty), got '
                         f'{getattr(value, "dtype", type(value).__name__)} {tuple(getattr(value, "shape", ()))}')
    if B is not None and (value.shape[0] != B or value.device != torch.device(device)):
        raise ValueError(f'{name} must be a float32 {(B, 4)} tensor on {device}, got {tuple(value.shape)} on {value.device}')
    if not bool(torch.isfinite(value).all()):
        raise ValueError(f'{name} must hold finite values')
    return value


def refuse_align(use_graph=False, lpips=False, ssim=False, loss_region='full', pixel_filter=None, pixel_target=None, latent_space='w+',
                 feature_layer=None, padded=False):
    """What the fitted alignment does not go with, refused in this one place before anything is launched.  Two of the
    reasons: LPIPS caches the target's taps, and a loss weight or a fitted mask lives in the photograph's frame, not in the warped one."""
    for on, what in ((use_graph, 'use_graph'), (lpips, 'the LPIPS term'), (ssim, 'the SSIM term'),
                     (loss_region != 'full', f'loss_region {loss_region!r} (a loss weight or a fitted mask)'),
                     (pixel_filter not in (None, 'box'), f'pixel_filter {pixel_filter!r}'), (pixel_target is not None, 'pixel_target'),
                     (latent_space == 's', "latent_space 's'"), (feature_layer is not None, 'feature_layer'),
                     (padded, 'a generator whose channel counts are zero-padded to multiples of 16')):
        if on:
            raise NotImplementedError(f"align with {what}: the alignment is built for the pixel term (every kind, full resolution or box "
                                      f"pixel_size) of the 'w+' / 'w' loop under launch plans")


COLOR_KINDS = ('gain', 'affine')      # the colour maps the W+ loop fits beside the latents


def check_color(color=None, color_lr=0.002, color_reg=0.0, prefix=''):
    """The options of the fitted colour map as (color, color_lr, color_reg): ValueError, naming the option, unless ``color`` is
    None or one of COLOR_KINDS, ``color_lr`` a finite number >= 0 (0 keeps theta at its start) and ``color_reg`` a finite number >= 0.
    Without ``color`` the other two are not looked at.  The default rate 0.002 is a choice — at most 0.2 of gain, or 25 grey levels of
    offset, over 100 steps — and not a measured optimum."""
    if color is None:
        return None, 0.002, 0.0
    if not isinstance(color, str) or color not in COLOR_KINDS:
        raise ValueError(f'{prefix}color must be None or one of {list(COLOR_KINDS)}, got {color!r}')
    rate = _finite_real(color_lr, prefix + 'color_lr', 'a finite number >= 0')
    reg = _finite_real(color_reg, prefix + 'color_reg', 'a finite number >= 0')
    if rate < 0.0 or reg < 0.0:
        raise ValueError(f'{prefix}color_lr / {prefix}color_reg must be finite numbers >= 0, got {color_lr!r}, {color_reg!r}')
    return color, rate, reg


def check_color_init(value, B=None, device=None, name='color_init'):
    """``color_init``, the start of theta: None (the identity) or a float32 (B, 12) tensor of finite values — (M row-major 3x3, b) per image —
    on ``device`` (batch and device are checked once they are known).  ValueError otherwise."""
    if value is None:
        return None
    if not isinstance(value, torch.Tensor) or value.dtype != torch.float32 or value.dim() != 2 or value.shape[1] != 12:
        raise ValueError(f'{name} must be None or a float32 (B, 12) tensor (M row-major 3x3, then b), got '
                         f'{getattr(value, "dtype", type(value).__name__)} {tuple(getattr(value, "shape", ()))}')
    if B is not None and (value.shape[0] != B or value.device != torch.device(device)):
        raise ValueError(f'{name} must be a float32 {(B, 12)} tensor on {device}, got {tuple(value.shape)} on {value.device}')
    if not bool(torch.isfinite(value).all()):
        raise ValueError(f'{name} must hold finite values')
    return value


def refuse_color(use_graph=False, lpips=False, ssim=False, loss_region='full', align=None, pixel_size=None, pixel_filter=None, pixel_target=None,
                 latent_space='w+', feature_layer=None, padded=False):
    """What the fitted colour map does not go with, refused in this one place before anything is launched: its fused kernel
    is the full-resolution pixel term, and LPIPS and SSIM would have to see the mapped image.  ``loss_region``: 'full', 'blend' and a loss
    weight go with it, 'fit' does not."""
    for on, what in ((use_graph, 'use_graph'), (lpips, 'the LPIPS term'), (ssim, 'the SSIM term'),
                     (loss_region == 'fit', "loss_region 'fit' (a fitted mask)"), (align is not None, f'align {align!r}'),
                     (pixel_size is not None, 'pixel_size'), (pixel_filter is not None, f'pixel_filter {pixel_filter!r}'),
                     (pixel_target is not None, 'pixel_target'), (latent_space == 's', "latent_space 's'"),
                     (feature_layer is not None, 'feature_layer'),
                     (padded, 'a generator whose channel counts are zero-padded to multiples of 16')):
        if on:
            raise NotImplementedError(f"color with {what}: the colour map is built for the full-resolution pixel term (every kind, with or "
                                      f"without a loss weight) of the 'w+' / 'w' loop under launch plans")


def check_noise_seed(value, name='noise_seed'):
    """The seed of the latent noise as an int; ValueError unless it is an integer in [0, 2^63)."""
    if isinstance(value, bool) or not isinstance(value, int) or not 0 <= value < 2 ** 63:
        raise ValueError(f'{name} must be an integer in [0, 2^63), got {value!r}')
    return value


class WPlusInverter:
    """Build-defined W+ optimisation loop: ``steps`` x {G(w) with fixed noise,
    per-image MSE, backward to w, Adam(lr, betas, eps)} — anchors: reference Generator.forward with
    ``noise=<list>`` (model.py:483-585), torch.optim.Adam as built by get_optimizer
    (src/models/OOD_faceGAN_model.py:398-400), basicsr MSELoss (losses.py:58-83).

    The loss of a step is defined once, in ``_WRun._loss_grad``: the pixel term — MSE, or the robust ``pixel_loss`` (on the composite with a loss weight; with ``pixel_size`` on the view area-pooled to that size or, with ``pixel_filter``, resized to it by that antialiased filter) — + lpips_weight * LPIPS
    (with ``lpips_size`` on the image and the target area-pooled to that size) + ssim_weight * (1 - SSIM); the step index is a device counter in every mode.
    The step itself is defined once too, ``_WRun._eager_step``: run from Python, replayed from a launch plan (default) or, with
    ``invert(use_graph=True)``, from a captured hipGraph, with a trajectory or without, on any number of streams.

    Projector schedule (rosinality's projector.py), every part off by default — the step is then the launch list above:
    ``lr_rampup`` / ``lr_rampdown``: fractions of the run over which the learning rate ramps up linearly / follows a cosine down
    (``ops.lr_multiplier``); ``latent_noise``: sigma_0, in latent units, of Gaussian noise added to the latent the generator reads, decaying as
    max(0, 1 - (t / steps) / noise_ramp)^2 (``noise_ramp`` <= 0: constant), a function of (``noise_seed``, the image's id, step, element);
    ``latent_reg``: adds latent_reg * mean (w - latent_anchor)^2 per image, evaluated at the unperturbed w (``last_terms['latent']``).

    Latent controls, off by default as well.  ``latent_space='w'``: one 512-vector per image — the latent stays (B,L,512) with
    identical rows, started at the layer mean of ``w0``; every layer receives the sum over the layers of the gradient and the latent noise is
    one vector repeated.  ``layer_lr``: L finite factors >= 0 of ``lr``, one per layer (of the step size: Adam does not see a gradient's scale);
    0 freezes a layer.  ``delta_reg``: adds delta_reg * mean_le (w_le - mean_l w_le)^2 per image, the squared spread of the layers about their
    mean, at the unperturbed w (``last_terms['delta']``); W is its limit.  'w' with either of the other two raises ValueError.

    StyleSpace (Wu et al., CVPR 2021).  ``latent_space='s'``: the latents stay at ``w0`` and the loop optimises an offset delta
    (B, R) on the per-channel styles, s = style_affine(w0) + delta, from 0 (the columns: ``GeneratorEngine.style_layout()``); ``invert`` then
    returns delta in the latents' place.  ``style_reg`` = lambda >= 0 adds lambda * mean_r delta_r^2 per image (``last_terms['style']``), a
    build-defined pull towards styles some w can produce.  ``layer_lr`` applies to the style rows of each layer; the lr ramps apply;
    delta_reg, latent_noise and latent_reg act on latents that do not move and raise ValueError, as ``style_reg`` does outside 's'.

    Feature offset (the F/W+ family: BDInvert, Feature-Style).  ``feature_layer`` = l in FEATURE_LAYERS: beside the latents the
    loop fits an offset delta (B, C, h, h), from 0, on the input of the styled up-conv that reads latent l, x' = x(w) + delta — at delta = 0
    the W+ run, and dL/ddelta is the input gradient the backward computes at that layer anyway.  Adam with ``feature_lr`` (None: ``lr``; 0
    leaves it at zero); ``feature_reg`` = lambda >= 0 adds lambda * mean delta^2 per image (``last_terms['feature']``).  The result is
    ``last_feature_offset``; the trajectory stays the latents'.  Goes with 'w+' and 'w', every loss term, layer_lr (all zeros: the offset
    alone is fitted), delta_reg, the schedule and streams; refused with ``use_graph``, latent_space 's' and a zero-padded generator.

    P_N+ prior (II2S, Zhu et al.).  ``pn_reg`` = lambda >= 0 adds lambda * mean_{l,d} q^T M q per image, q = l5(w) - mu per latent
    row, l5 the inverse of the mapping network's last LeakyReLU and (mu, M) the ``oodgan.pn.PNStats`` passed as ``invert(pn_stats=)``
    (``Generator.pn_stats``): the Mahalanobis distance to the latents the generator was trained on, where ``latent_reg`` charges every
    direction of W the same.  Evaluated at the unperturbed w, added to the gradient ``backward`` returned (``last_terms['pn']``); goes with
    'w+' and 'w', every other option and streams; refused with ``use_graph`` (NotImplementedError) and latent_space 's' (ValueError).

    Fitted mask (the reference's MaskLoss, src/losses/mask_loss.py, is the anchor).  ``mask_size`` = m in MASK_SIZES: beside
    the latents the loop fits the logits l (B,1,m,m) of a mask a = sigmoid(l), from ``invert(mask_logits=)``; the loss weight of the
    composite objective is beta = U(a), U the bilinear enlargement of ``F.interpolate(align_corners=False)``, rewritten every step, and per
    image the loss gains ``mask_area_weight`` * max(0, mean(1 - a) - ``mask_area``) + ``mask_binary_weight`` * mean(min(a, 1 - a)): the loop
    decides which region, up to an area budget, it stops fitting.  Adam with ``mask_lr`` and the loop's betas, eps and ramps.  Results:
    ``last_fitted_mask`` (a_T), ``last_mask_logits``, ``last_loss_weight`` (beta_T = U(a_T)), ``last_terms['mask_area']`` /
    ``['mask_binary']`` (the hinge and the binarisation mean per step and image).  Goes with 'w+' and 'w', layer_lr, delta_reg, the schedule,
    pn_reg, streams, the robust pixel terms, LPIPS (+ lpips_size) and SSIM; refused (``refuse_mask_fit``, NotImplementedError) with
    ``use_graph``, pixel_size, pixel_filter / pixel_target, latent_space 's', feature_layer and a zero-padded generator; a caller's
    ``loss_weight`` beside it raises ValueError.

    Fitted alignment.  ``align='similarity'``: beside the latents the loop fits theta = (log-scale, rotation in radians, tx, ty
    in units of half the image side) per image, from ``invert(align_init=)`` (None: the identity), and every step compares G(w) with the
    target warped by theta (bicubic, border padding; ``ops.similarity_warp``) — a photograph a few pixels or a degree off the generator's
    canonical frame is registered instead of being explained by the latents.  The target is warped, not the generator image: forward,
    backward and the pixel-term kernels are the plain step's, and dL/dtheta is read off the image gradient.  Adam with ``align_lr`` (0.001:
    about half a pixel per step at 1024²; not a measured optimum) and the loop's betas, eps and ramps; ``align_reg`` = mu >= 0 adds
    mu * sum_k theta_k^2 per image (``last_terms['align']``).  Results: ``last_alignment`` (B,4), ``last_aligned_target``.  Goes with 'w+' and
    'w', layer_lr, delta_reg, the schedule, pn_reg, the four pixel kinds, box ``pixel_size`` and streams; refused (``refuse_align``,
    NotImplementedError) with ``use_graph``, LPIPS, SSIM, a loss weight or a fitted mask, pixel_filter / pixel_target, latent_space 's',
    feature_layer and a zero-padded generator.

    Fitted colour map.  ``color='gain'`` or ``'affine'``: beside the latents the loop fits theta = (M row-major 3x3, b) per image,
    from ``invert(color_init=)`` (None: the identity), and takes the pixel term on C(G) = M G + b — a colour cast, an exposure or faded film
    is explained by twelve numbers ('gain': six, the diagonal of M and b — white balance and exposure) instead of by the latents.  The
    generator image is mapped, not the photograph: with the map on the target (M, b) -> (0, const) would shrink any residual.  One fused
    pass (``ops.color_pixel_loss_grad``) gives the term, M^T g for the backward and the sums of dL/dtheta; ``ops.color_step`` is Adam with
    ``color_lr`` (0.002: at most 0.2 of gain or 25 grey levels of offset over 100 steps; a choice, not a measured optimum) and the loop's
    betas, eps and ramps: one launch more per step.  ``color_reg`` = mu >= 0 adds mu * sum_k (theta_k - id_k)^2 per image
    (``last_terms['color']``).  Result: ``last_color`` (B,12); ``ops.color_apply(G, last_color)`` is the mapped image.  Goes with 'w+' and 'w',
    layer_lr, delta_reg, the schedule, pn_reg, the four pixel kinds, a loss weight and streams; refused (``refuse_color``, NotImplementedError)
    with ``use_graph``, LPIPS, SSIM, a fitted mask, align, pixel_size, pixel_filter / pixel_target, latent_space 's', feature_layer and a
    zero-padded generator.

    ``check_every`` / ``check_lag``: the range guard of ``_WRun`` (0 = flags read only by the caller).  ``last_stats`` after a call:
    {'steps_run': forward/backward pairs enqueued per (sub-)batch, 'rollbacks': windows repeated with exact scales}; ``last_plan``:
    {'steps': steps replayed per (sub-)batch, from the plan or the graph, 'launches': launches of the recorded plan (0: none, or a graph)}."""

    def __init__(self, engine, lr=0.01, betas=(0.9, 0.999), eps=1e-8, check_every=10, check_lag=2, use_plan=None, lpips=None, lpips_weight=0.0,
                 ssim_weight=0.0, lr_rampup=0.0, lr_rampdown=0.0, latent_noise=0.0, noise_ramp=0.75, noise_seed=0, latent_reg=0.0,
                 pixel_loss='mse', pixel_scale=0.1, lpips_size=None, latent_space='w+', layer_lr=None, delta_reg=0.0, style_reg=0.0,
                 pixel_size=None, feature_layer=None, feature_lr=None, feature_reg=0.0, pn_reg=0.0, pixel_filter=None, mask_size=None,
                 mask_lr=0.1, mask_area=0.30, mask_area_weight=5.0, mask_binary_weight=0.2, align=None, align_lr=0.001, align_reg=0.0,
                 color=None, color_lr=0.002, color_reg=0.0):
        self.engine, self.lr, self.betas, self.eps = engine, lr, betas, eps
        # fitted colour map, off by default (``color`` None): the step is then the launch list above.  'gain' / 'affine': beside
        # the latents the loop fits theta = (M, b) per image and takes the pixel term on M G + b.  The default rate 0.002 allows at most 0.2
        # of gain, or 25 grey levels of offset, over 100 steps: a choice, nobody has measured it as an optimum
        self.color, self.color_lr, self.color_reg = check_color(color, color_lr, color_reg)
        self.last_color = None
        # fitted alignment, off by default (``align`` None): the step is then the launch list above.  'similarity': beside the
        # latents the loop fits theta = (log-scale, rotation, tx, ty) per image and compares G(w) with the target warped by it.  The default
        # rate 0.001 moves a translation by about half a pixel per step at 1024² (tx is in units of half the image side); nobody has
        # measured it as an optimum
        self.align, self.align_lr, self.align_reg = check_align(align, align_lr, align_reg)
        self.last_alignment = self.last_aligned_target = None
        # fitted mask, off by default (``mask_size`` None): the step is then the launch list above.  With a size m the loop
        # fits the logits of an m x m mask beside the latents, under the reference's mask objective; the image size is known in ``invert``
        self.mask_size = None
        self.mask_lr, self.mask_area, self.mask_area_weight, self.mask_binary_weight = 0.1, 0.30, 5.0, 0.2
        if mask_size is not None:
            (self.mask_size, self.mask_lr, self.mask_area, self.mask_area_weight,
             self.mask_binary_weight) = check_mask_fit(mask_size, mask_lr, mask_area, mask_area_weight, mask_binary_weight)
        self.last_fitted_mask = self.last_mask_logits = self.last_loss_weight = None
        # the filter of the ``pixel_size`` view: None or 'box' = the area pool of §20, today's kernels; 'bilinear', 'bicubic'
        # or 'lanczos3': the antialiased resize the usual resizers apply (two kernels, one launch more per step).  It needs ``pixel_size``
        # (or ``invert(pixel_target=)``) and takes neither a loss weight nor the hipGraph option
        self.pixel_filter = check_pixel_filter(pixel_filter)
        # the size the pixel term is taken at: None = the image's own, today's kernels and launch list; an int: the term is the
        # mean of rho over the area-pooled residual (one fused kernel; with ``lpips_size`` of the same value both terms see one view).  A
        # low-resolution photograph enters nearest-upsampled: its area pool is the photograph.  Checked against the image size in ``invert``
        self.pixel_size, self._pixel_f = check_pixel_size(pixel_size), 1
        # the size the LPIPS term is taken at: None = the image's own, today's path; an int: the image and the target are
        # area-pooled to it first (the projectors' value is 256).  The image size is known in ``invert``: the part of the check that needs it runs there
        self.lpips_size, self._lpips_f = check_lpips_size(lpips_size), 1
        # the pixel term: 'mse' (default: today's kernels and launch list) or a robust rho of the residual with scale ``pixel_scale`` in image
        # units — 'charbonnier', 'huber' (a very large scale: half the MSE), 'geman_mcclure' (DESIGN.md §5).  The default scale 0.1, a tenth of
        # the image half-range (about 13 grey levels), is a choice, not a measured optimum
        self.pixel_loss, self.pixel_scale = check_pixel_loss(pixel_loss, pixel_scale)
        # loss = per-image MSE + lpips_weight * LPIPS(alex) (north_star: "W+ Adam steps against LPIPS/L2"); ``lpips``: an oodgan.lpips.LPIPSAlex
        # (min_max = the generator's output range).  Off by default: the `lpips` weights are third-party and absent here (parity unpinned).
        # ``invert`` then returns the TOTAL loss per step and image; ``last_terms`` = {'pixel', 'mse', 'lpips', 'ssim', 'latent', 'delta'} tables (None: term off;
        # 'pixel' is the pixel term's table whatever its kind, 'mse' the same tensor when ``pixel_loss`` is 'mse' and None otherwise).
        self.lpips, self.lpips_weight = lpips, float(lpips_weight)
        # + ssim_weight * (1 - SSIM): the metric the CLI reports, on the unrounded images; 0 (default) = the term, its
        # kernel launches and its table do not exist
        self.ssim_weight = check_nonneg(ssim_weight, 'ssim_weight')
        self.lr_rampup, self.lr_rampdown = check_nonneg(lr_rampup, 'lr_rampup'), check_nonneg(lr_rampdown, 'lr_rampdown')
        self.latent_noise, self.noise_ramp = check_nonneg(latent_noise, 'latent_noise'), check_nonneg(noise_ramp, 'noise_ramp')
        self.noise_seed, self.latent_reg = check_noise_seed(noise_seed), check_nonneg(latent_reg, 'latent_reg')
        # latent controls, all off by default: the step is then the launch list above.  The number of layers is known in ``invert``
        self.latent_space, self.layer_lr, self.delta_reg = check_latent_controls(latent_space, layer_lr, delta_reg)
        # StyleSpace: ``latent_space='s'`` optimises an offset on the styles; ``style_reg`` * mean_r delta_r^2 per image pulls it
        # back towards styles some w can produce — a term of this build, as delta_reg is
        self.style_reg = check_style_space(self.latent_space, style_reg, self.delta_reg, self.latent_noise, self.latent_reg)
        # feature offset, off by default: the step is then the launch list above.  ``feature_layer`` in FEATURE_LAYERS: an offset
        # on the input of that latent's up-conv is fitted beside the latents, by Adam with ``feature_lr`` (None: ``lr`` — a choice, not a
        # measured optimum; 0 leaves the offset at zero); ``feature_reg`` * mean delta^2 per image keeps it small (``last_terms['feature']``).
        # After a call ``last_feature_offset`` holds it, (B, C, h, h), None without the option
        self.feature_layer, self.feature_lr, self.feature_reg = check_feature_offset(feature_layer, feature_lr, feature_reg, lr, self.latent_space)
        self.last_feature_offset = None
        # P_N+ prior, off by default: the step is then the launch list above.  ``pn_reg`` = lambda >= 0 adds lambda * the squared
        # length of l5(w) - mu in the whitened space of the mapping network's outputs, per image; ``invert(pn_stats=)`` brings the statistics
        self.pn_reg = check_pn(pn_reg, self.latent_space)
        self.last_terms = None
        # launch plans (oodgan_plan_*): on unless OODGAN_USE_PLAN=0; off for a run that returns its trajectory
        self.use_plan = (os.environ.get('OODGAN_USE_PLAN', '1') != '0') if use_plan is None else bool(use_plan)
        self.check_every, self.check_lag = int(check_every), max(0, int(check_lag))
        self._runs, self._pins, self._graphs = [], [], []
        self.last_stats = self.last_plan = None
        self.on_step = None         # optional callable(run) after every enqueued step (progress reporting; tests inject faults with it)

    def _pinned(self, i):
        while len(self._pins) <= i:
            self._pins.append(torch.zeros(2, dtype=torch.int32).pin_memory())
        return self._pins[i]

    def invert(self, target, w0, noises, steps=100, return_trajectory=False, streams=1, use_graph=False, loss_weight=None, noise_ids=None,
               latent_anchor=None, pn_stats=None, pixel_target=None, mask_logits=None, align_init=None, color_init=None):
        """``streams`` > 1 splits the batch into that many independent sub-batches, each advanced on its own HIP
        stream (images are independent): the HBM-bound layout/activation kernels of one sub-batch
        then share the GPU with the matrix kernels of the other instead of running back to back.
        ``loss_weight``: None (the per-image MSE) or a float32 (B,1,S,S) plane beta in [0,1] on the device — the loss is then taken on the
        composite c = target + beta*(G(w) - target); a pixel with beta = 0 has no influence on the run.
        ``noise_ids``: int64 (B,), the id each image draws its latent noise under (default arange(B)); it travels with the image into the
        sub-batches, so an image sees the same noise on one stream or several and in any batch.  ``latent_anchor``: (L,512) or (B,L,512),
        what ``latent_reg`` pulls towards (required when latent_reg > 0).  ``pn_stats``: the ``oodgan.pn.PNStats`` of the mapping network on
        the latents' device (required when pn_reg > 0; not looked at otherwise).  ``pixel_target``: a float32 (B,C,n,n) image
        on the device, the low-resolution target of the pixel term given at its own size; it fixes ``pixel_size`` = n (a differing
        ``pixel_size`` is an error) and replaces the view of ``target`` made here — the pooled target with the box, the resized one with a
        ``pixel_filter``.  ``target`` stays the full-size image LPIPS and SSIM, if on, compare with.  Not with a loss weight.
        ``mask_logits``: with ``mask_size`` = m, the float32 (B,1,m,m) start logits of the fitted mask on the device
        (``mask_logits(a0)`` makes them from a start mask); required then, refused without it, and not beside a ``loss_weight``.
        ``align_init``: with ``align``, the float32 (B,4) start of theta on the device, None = the identity; refused without
        ``align``.  Afterwards ``last_alignment`` (B,4) is the fitted theta and ``last_aligned_target`` the target warped by it.
        ``color_init``: with ``color``, the float32 (B,12) start of theta = (M, b) on the device, None = the identity; refused
        without ``color``.  Afterwards ``last_color`` (B,12) is the fitted theta."""
        B = w0.shape[0]
        self.last_color = None
        if self.color is not None:
            refuse_color(use_graph, self.lpips is not None and self.lpips_weight != 0.0, self.ssim_weight != 0.0,
                         'fit' if self.mask_size is not None else 'full', self.align,
                         None if self.pixel_size == int(target.shape[-1]) else self.pixel_size, self.pixel_filter, pixel_target,
                         self.latent_space, self.feature_layer, self.engine.padded)
            if target.dim() != 4 or target.shape[1] != 3:
                raise ValueError(f'color: the target must be (B,3,H,W), got {tuple(target.shape)}')
            check_color_init(color_init, B, target.device)
            color_init = ops.color_identity(B, target.device) if color_init is None else color_init.detach().contiguous()
        elif color_init is not None:
            raise ValueError('color_init without color: there is no colour map it could start')
        self.last_alignment = self.last_aligned_target = None
        if self.align is not None:
            refuse_align(use_graph, self.lpips is not None and self.lpips_weight != 0.0, self.ssim_weight != 0.0,
                         'full' if (loss_weight is None and self.mask_size is None) else 'blend' if self.mask_size is None else 'fit',
                         self.pixel_filter, pixel_target, self.latent_space, self.feature_layer, self.engine.padded)
            if target.dim() != 4 or min(target.shape[-2:]) < 4:
                raise ValueError(f'align: the target must be (B,C,H,W) with H, W >= 4, got {tuple(target.shape)}')
            check_align_init(align_init, B, target.device)
            align_init = (torch.zeros(B, 4, device=target.device, dtype=torch.float32) if align_init is None
                          else align_init.detach().contiguous())
        elif align_init is not None:
            raise ValueError('align_init without align: there is no alignment it could start')
        self.last_fitted_mask = self.last_mask_logits = self.last_loss_weight = None
        if self.mask_size is not None:
            refuse_mask_fit(use_graph, None if self.pixel_size == int(target.shape[-1]) else self.pixel_size, self.pixel_filter, pixel_target, self.latent_space, self.feature_layer, self.engine.padded)
            check_mask_fit(self.mask_size, self.mask_lr, self.mask_area, self.mask_area_weight, self.mask_binary_weight, int(target.shape[-1]))
            if loss_weight is not None:
                raise ValueError('a loss weight beside mask_size: the fitted mask IS the loss weight of the run')
            m = self.mask_size
            if (not isinstance(mask_logits, torch.Tensor) or tuple(mask_logits.shape) != (B, 1, m, m) or mask_logits.dtype != torch.float32
                    or mask_logits.device != target.device):
                raise ValueError(f'mask_logits must be a float32 {(B, 1, m, m)} tensor on {target.device} (mask_size {m})')
            if target.shape[-1] != target.shape[-2]:
                raise ValueError(f'mask_size: the image must be square, got {tuple(target.shape[-2:])}')
            mask_logits = mask_logits.detach().contiguous()
        elif mask_logits is not None:
            raise ValueError('mask_logits without mask_size: there is no fitted mask they could start')
        pn = pn_stats if check_pn(self.pn_reg, self.latent_space, pn_stats, int(w0.shape[-1]), w0.device, need_stats=True) != 0.0 else None
        size = check_lpips_size(self.lpips_size, int(target.shape[-1]))
        self._lpips_f = 1 if size is None else int(target.shape[-1]) // size
        pixel_target, psize = check_pixel_target(pixel_target, target, self.pixel_size)
        psize = check_pixel_size(psize, int(target.shape[-1]), 'pixel_size' if pixel_target is None else 'the size of pixel_target')
        self._pixel_f = 1 if psize is None else int(target.shape[-1]) // psize
        if self.pixel_filter is not None and self._pixel_f == 1:
            raise ValueError(f'pixel_filter {self.pixel_filter!r} needs pixel_size (or pixel_target) below the image size: at the image\'s own '
                             f'size there is no view to filter')
        if loss_weight is not None and (self.pixel_filter is not None or pixel_target is not None):
            raise ValueError(f'a loss weight with {"pixel_filter" if self.pixel_filter is not None else "pixel_target"}: the masked objective '
                             f'is taken on the area-pooled view of the full target only')
        if self._pixel_f > 1 and (target.shape[-2] % self._pixel_f or target.shape[-1] % self._pixel_f):
            raise ValueError(f'pixel_size {self.pixel_size}: the image {tuple(target.shape[-2:])} is not a multiple of the factor {self._pixel_f}')
        ids, anchor = self._sched_inputs(w0, noise_ids, latent_anchor)
        check_layer_lr(self.layer_lr, int(w0.shape[1]))
        if self.latent_space == 's' and self.engine.padded:
            raise NotImplementedError("latent_space 's' on a generator whose channel counts are zero-padded to multiples of 16")
        self.last_feature_offset = None
        fshape = None
        if self.feature_layer is not None:      # ValueError for a layer this generator lacks, NotImplementedError on a zero-padded one
            check_feature_layer(self.feature_layer, self.engine.n_latent)
            fshape = self.engine.feature_shape(self.feature_layer)
        if self.latent_space == 'w':            # the start: the layer mean, on every layer (set-up, not the step)
            w0 = w0.detach().mean(dim=1, keepdim=True).expand_as(w0).contiguous()
        if loss_weight is not None:
            if tuple(loss_weight.shape) != (B, 1) + tuple(target.shape[2:]) or loss_weight.dtype != torch.float32 or loss_weight.device != target.device:
                raise ValueError(f'loss_weight must be a float32 {(B, 1) + tuple(target.shape[2:])} tensor on {target.device}, got '
                                 f'{loss_weight.dtype} {tuple(loss_weight.shape)} on {loss_weight.device}')
            loss_weight = loss_weight.contiguous()
        streams = max(1, min(int(streams), B))
        if B == 0:          # an empty shard (oodgan/parallel.py hands a rank with no images an empty batch): nothing to launch
            steps = 0
        if steps <= 0:
            w = (torch.zeros(B, self.engine.R, device=w0.device, dtype=torch.float32) if self.latent_space == 's'
                 else w0.detach().clone().contiguous())
            empty = torch.empty(0, B, device=w0.device, dtype=torch.float32)
            if fshape is not None:
                self.last_feature_offset = torch.zeros((B,) + fshape, device=w0.device, dtype=torch.float32)
            if self.mask_size is not None and B > 0:
                self.last_mask_logits = mask_logits.clone()
                self.last_fitted_mask, self.last_loss_weight = ops.maskfit_expand(self.last_mask_logits, int(target.shape[-1]))
            if self.color is not None:
                self.last_color = color_init.clone()
            if self.align is not None and B > 0:
                self.last_alignment = align_init.clone()
                self.last_aligned_target = ops.similarity_warp(target.contiguous(), self.last_alignment)
            return (w, empty, []) if return_trajectory else (w, empty)
        if return_trajectory:
            streams, use_graph = 1, False
        if use_graph:
            self._refuse_graph(loss_weight)
        from . import _lib
        # the multi-stream threshold of the 8-wave stride-1 kernel, unless the caller set the tunable itself; not for a graph run
        override = (streams > 1 and not use_graph and MULTI_STREAM_S1_BIG_MIN_ITEMS != _S1_BIG_DEFAULT
                    and _lib.lib().oodgan_get_tunable(b's1_big_min_items') == _S1_BIG_DEFAULT)
        if override:
            _lib.set_tunable('s1_big_min_items', MULTI_STREAM_S1_BIG_MIN_ITEMS)
        f0 = None if fshape is None else ops.zeros(B, *fshape, device=w0.device)
        try:
            return self._invert_runs(target, w0, noises, steps, streams, return_trajectory, use_graph, loss_weight, ids, anchor, f0, pn,
                                     pixel_target, mask_logits, align_init if self.align is not None else None,
                                     color_init if self.color is not None else None)
        finally:
            if override:
                _lib.set_tunable('s1_big_min_items', _S1_BIG_DEFAULT)

    def _refuse_graph(self, loss_weight):
        """What the hipGraph option does not take, refused before anything is launched.  (Since the graph replays ``_WRun._eager_step`` these
        are no longer things it cannot express; lifting them is a change of its own.)"""
        for on, what in ((loss_weight is not None, 'a loss weight'),
                         (self.lpips is not None and self.lpips_weight != 0.0, 'the LPIPS term'),
                         (self.ssim_weight != 0.0, 'the SSIM term'),
                         (self.pixel_loss != 'mse', 'a robust pixel term'),
                         (self._pixel_f > 1, 'pixel_size'),
                         (self.pixel_filter is not None, 'pixel_filter'),
                         (self.lr_rampup > 0.0 or self.lr_rampdown > 0.0 or self.latent_noise != 0.0 or self.latent_reg != 0.0,
                          'the projector schedule (lr ramps, latent noise, latent prior)'),
                         (self.latent_space != 'w+', f'latent_space {self.latent_space!r}'),
                         (self.layer_lr is not None, 'layer_lr'),
                         (self.delta_reg != 0.0, 'delta_reg'),
                         (self.feature_layer is not None, 'feature_layer'),
                         (self.pn_reg != 0.0, 'pn_reg')):
            if on:
                raise NotImplementedError(f'use_graph with {what}: use the launch plans (default) instead')

    def _sched_inputs(self, w0, noise_ids, latent_anchor):
        """(ids, anchor) of a call: the noise ids (None when the noise is off) and the prior's anchor (None when the prior is off), checked."""
        B, ids, anchor = w0.shape[0], None, None
        if self.latent_noise != 0.0:
            ids = torch.arange(B, dtype=torch.int64, device=w0.device) if noise_ids is None else noise_ids
            if not isinstance(ids, torch.Tensor) or tuple(ids.shape) != (B,) or ids.dtype != torch.int64 or ids.device != w0.device:
                raise ValueError(f'noise_ids must be an int64 ({B},) tensor on {w0.device}')
            ids = ids.contiguous()
        if self.latent_reg != 0.0:
            if latent_anchor is None:
                raise ValueError('latent_reg > 0 needs latent_anchor: the latent the prior pulls towards')
            anchor = latent_anchor
            if (not isinstance(anchor, torch.Tensor) or tuple(anchor.shape) not in (tuple(w0.shape), tuple(w0.shape[1:]))
                    or anchor.dtype != torch.float32 or anchor.device != w0.device):
                raise ValueError(f'latent_anchor must be a float32 {tuple(w0.shape[1:])} or {tuple(w0.shape)} tensor on {w0.device}')
            anchor = anchor.detach().contiguous()
        return ids, anchor

    def _split(self, target, w0, noises, beta, streams, on_side, ids=None, anchor=None, f0=None, pn=None, px=None, ml0=None, th0=None, c0=None):
        """(streams, engines, [(target, w0, noises, beta, ids, anchor, f0, pn, px, ml0, th0, c0)] per stream; ``px``, the pixel target, ``ml0``, the mask's start logits, ``th0``, the alignment's start, and ``c0``, the colour map's, are sliced like the target): sub-batch i is images [(i*B)//streams, ((i+1)*B)//streams);
        ``pn``, the read-only statistics of the P_N+ prior, is shared by all of them.
        ``on_side``: the sub-batches run on side streams that wait for the caller's; otherwise (one sub-batch) the stream is None, the
        caller's own."""
        B = w0.shape[0]
        cur = torch.cuda.current_stream()
        side = _side_streams(w0.device, streams) if on_side else [None]
        # the state resets enqueue zero-fills on the CALLER's stream: they must precede the wait_stream below, or nothing
        # orders them against the atomicOr / atomic max the side streams do on the same flags (engines[0] keeps its
        # FwdRange and bwd_flag across calls)
        engines = [self.engine] + [self.engine.clone_shared() for _ in range(streams - 1)]
        for eng in engines:
            eng.reset_bwd_state()
            eng.reset_fwd_state()
        parts = []
        for i in range(streams):
            sl = slice((i * B) // streams, ((i + 1) * B) // streams)
            parts.append((target[sl].contiguous(), w0[sl].detach().contiguous(),
                          [n[sl].contiguous() if n.shape[0] == B else n for n in noises], None if beta is None else beta[sl].contiguous(),
                          None if ids is None else ids[sl].contiguous(),
                          anchor[sl].contiguous() if (anchor is not None and anchor.dim() == w0.dim()) else anchor,
                          None if f0 is None else f0[sl].contiguous(), pn, None if px is None else px[sl].contiguous(),
                          None if ml0 is None else ml0[sl].contiguous(), None if th0 is None else th0[sl].contiguous(),
                          None if c0 is None else c0[sl].contiguous()))
        if on_side:
            for st in side:
                st.wait_stream(cur)             # AFTER the slices above were enqueued on the caller's stream
        return side, engines, parts

    @staticmethod
    def _gather(side, w, tables, f=None, ml=None, th=None, ct=None):
        """The per-stream latents (joined along the batch) and loss tables (``tables``: one list per term, None = term off; joined along the
        images) on the caller's stream; of a single run, its own tensors.  ``f``: the per-stream feature offsets, joined along the batch
        like the latents and returned after the tables; ``ml``: the per-stream mask logits, the same way, returned after them; ``th``: the per-stream alignments, after them; ``ct``: the per-stream colour maps, returned last."""
        cur = torch.cuda.current_stream()
        join = lambda ts, dim: ts[0] if len(ts) == 1 else torch.cat(ts, dim)
        for st in side:
            if st is not None:
                cur.wait_stream(st)
        out = [join(w, 0)] + [None if ts[0] is None else join(ts, 1) for ts in tables]
        if f is not None:
            out.append(join(f, 0))
        if ml is not None:
            out.append(join(ml, 0))
        if th is not None:
            out.append(join(th, 0))
        if ct is not None:
            out.append(join(ct, 0))
        for ts in [w] + tables + ([] if f is None else [f]) + ([] if ml is None else [ml]) + ([] if th is None else [th]) + ([] if ct is None else [ct]):     # tensors produced on side streams are consumed on the caller's stream
            for t in ts:
                if t is not None:
                    t.record_stream(cur)
        return out

    def _invert_runs(self, target, w0, noises, steps, streams, return_trajectory, use_graph, beta=None, ids=None, anchor=None, f0=None, pn=None,
                     px=None, ml0=None, th0=None, c0=None):
        self._graphs = []                       # the graphs of the call before (and their private pools) lived until here
        replay = 'graph' if use_graph else 'plan' if self.use_plan else None
        # a hipGraph cannot be captured on the default stream: a graph run takes a side stream also when it is the only one
        side, engines, parts = self._split(target, w0, noises, beta, streams, use_graph or streams > 1, ids, anchor, f0, pn, px, ml0, th0, c0)
        runs = []
        try:
            for st, eng, (x, w, nz, *rest) in zip(side, engines, parts):
                with torch.cuda.stream(st):     # state tensors initialised on the stream that uses them
                    runs.append(_WRun(self, eng, x, w, nz, steps, st, return_trajectory, replay, *rest))
            busy = True
            while busy:
                busy = False
                for r in runs:
                    busy = r.advance() or busy
        finally:
            for r in runs:
                r.close()
            # the runs point back here: left in ``_runs`` they make the inverter, with the graphs it keeps, a reference cycle, which the
            # collector frees whenever it happens to run — inside the next inverter's capture, where destroying a graph aborts the process
            self._runs = []
        self.last_stats = {'steps_run': [r.steps_run for r in runs], 'rollbacks': [r.rollbacks for r in runs]}
        self.last_plan = {'steps': [r.plan_steps for r in runs], 'launches': [r.plan_size for r in runs]}
        w, *tables = self._gather(side, [r.w for r in runs], [[r.lbuf for r in runs], [r.lp_table for r in runs], [r.ss_table for r in runs],
                                                             [r.lat_table for r in runs], [r.dl_table for r in runs], [r.st_table for r in runs],
                                                             [r.ft_table for r in runs], [r.pn_table for r in runs], [r.ma_table for r in runs],
                                                             [r.mb_table for r in runs], [r.al_table for r in runs], [r.co_table for r in runs]],
                                 None if f0 is None else [r.f for r in runs], None if ml0 is None else [r.ml for r in runs],
                                 None if th0 is None else [r.th for r in runs], None if c0 is None else [r.ct for r in runs])
        if c0 is not None:          # the fitted colour map
            self.last_color = tables.pop()
        if th0 is not None:         # the fitted theta and the target in its frame: one more warp, outside the step
            self.last_alignment = tables.pop()
            self.last_aligned_target = ops.similarity_warp(target.contiguous(), self.last_alignment)
        if ml0 is not None:         # a_T and beta_T of the fitted logits: one more expand, outside the step
            self.last_mask_logits = tables.pop()
            self.last_fitted_mask, self.last_loss_weight = ops.maskfit_expand(self.last_mask_logits, int(target.shape[-1]))
        if f0 is not None:
            self.last_feature_offset = tables.pop()
        # a graph run has no per-window guard: its flags are read once, here, and a flagged inversion is repeated through the guarded loop
        if use_graph and any(eng.bwd_scale_violated() or eng.fwd_range_violated() for eng in engines):
            return self.invert(target, w0, noises, steps, streams=streams, use_graph=False)
        losses = self._total(*tables)
        return (w, losses, runs[0].traj) if return_trajectory else (w, losses)

    def _total(self, mse, lp, ss=None, lat=None, dl=None, st=None, ft=None, pn=None, ma=None, mb=None, al=None, co=None):
        self.last_terms = {'pixel': mse, 'mse': mse if self.pixel_loss == 'mse' else None, 'lpips': lp, 'ssim': ss, 'latent': lat, 'delta': dl,
                           'style': st, 'feature': ft, 'pn': pn, 'mask_area': ma, 'mask_binary': mb, 'align': al, 'color': co}
        total = mse if lp is None else mse + self.lpips_weight * lp
        total = total if ss is None else total + self.ssim_weight * ss
        total = total if lat is None else total + self.latent_reg * lat
        total = total if dl is None else total + self.delta_reg * dl
        total = total if st is None else total + self.style_reg * st
        total = total if ft is None else total + self.feature_reg * ft
        total = total if pn is None else total + self.pn_reg * pn
        total = total if ma is None else total + self.mask_area_weight * ma
        total = total if mb is None else total + self.mask_binary_weight * mb
        total = total if al is None else total + self.align_reg * al
        return total if co is None else total + self.color_reg * co
