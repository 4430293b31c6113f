"""The three HIP encoders (oodgan/encoder_hip.py) against the float64 torch mirror at every batch size whose kernels differ.

Which kernel a trunk conv runs on follows the batch size (csrc/conv_f16s_tiny.hip, tiny_shape: the skinny-GEMM kernel takes a stride-1
conv on a 16² / 32² map while B*H² <= tiny_mid_max = 1024, so the 32² convs leave it at B = 2 and the 16² ones at B = 5; the tile
kernels s1big / s1v2 take over), and so do the stride-2 routes (tiny / s2big / s2v2 / the fp32-input s2gen) and the grouped chains of the
style heads.  The reference is tests/torch_encoder_mirror.py in float64 (pinned to the original's vectors by test_encoder.py), walked unit
by unit by tests/encoder_ref.py: ONE pass over eight distinct images per encoder, sliced for the smaller batches.

  chained   the encoder's own forward: w and every tap, all elements, max|d| / max|ref| (no floor at 1), the project's end-to-end bars
            (2e-4; Feature-Style content 1e-3 — test_encoder.py, test_restyle.py)
  isolated  HIP unit i fed the reference's INPUT to unit i (cast to float32), against the reference's output of unit i: no error
            accumulates through the trunk, so a 1e-4-class defect of one kernel family at one batch size cannot hide.  Bar 2e-5 of
            max|ref|, the bar these S-form / 8-wave kernels are held to at op level (test_hip_samm.py); the mirror's own float32 rounding
            per unit is 2e-7 .. 7e-7 (the band the CPU test below asserts), so the bar is 30-100x the reference's rounding
  heads     ``_style_heads`` and the bicubic FPN fed the reference's maps, every head's delta, same 2e-5
  rows      row k of the batch of eight against the same image run alone (other kernel families: not bit-equal): 4e-5 of the batch's
            max|ref| — both are within 2e-5 of one reference, and the lone row's max|ref| is at most the batch's
  dispatch  the per-batch family counts (oodgan_dispatch_count), so that the matrix provably crosses both thresholds

One encoder instance runs the batches in order and then batch 1 again (the ``_memo`` rows keyed by B, the packed-weight cache and the
pooled S-form / workspace buffers are shared between batch sizes).

Float32 mirror against the float64 one, max|d| / max|ref| (CPU, asserted below 2e-6): e4e 2.2e-7 (input layer) .. 6.9e-7 (units 21-23),
w 1.1e-6; ReStyle taps 3.0e-7 .. 5.7e-7; Feature-Style taps 2.5e-7 .. 6.4e-7, content 8.4e-7, latents 5.0e-7 (with this module's images: units up
to 9.6e-7, e4e p1 1.4e-6, Feature-Style block 23 1.1e-6).

Measured on the MI355X (worst over the rows of each batch; the bars above come from the project, not from these):
  e4e       isolated worst unit (always unit 21, a 32² stride-2 unit) B=1 6.4e-7, B=2 8.7e-7, B=4 8.1e-7, B=5 8.1e-7, B=8 8.0e-7: 0.6-1.0x the
            float32 mirror's own 8.4e-7 on that unit; heads 9.2e-7 .. 1.05e-6, p2 7.2e-7 .. 8.1e-7, p1 5.7e-7 .. 6.8e-7; chained worst (w) 1.03e-6 .. 1.23e-6 at every B;
            rows 0 / 4 / 7 of B=8 vs alone: isolated 5.5e-7 (unit 23), chained 9.2e-7; stages 0 .. 18 at B=3: w 7.2e-7 .. 1.07e-6
            tiny / s1v2 / s1big / s2big / s2v2 launches per forward: B=1 36/12/1/2/5, B=2 9/38/2/4/3, B=4 9/33/7/5/2, B=5 5/37/7/5/2,
            B=8 5/30/14/7/0 (s1pp = 1 throughout: the input layer)
  ReStyle   isolated worst (unit 21) B=1 4.7e-7, B=3 5.2e-7, B=8 6.5e-7 (0.6-0.9x the float32 mirror's); heads 4.8e-8 .. 5.5e-8; chained worst tap 5.6e-7 .. 8.4e-7, w 7.7e-8 ..
            1.06e-7 of max|w| = 0.54; row 7 of B=8 vs alone: isolated 3.8e-7, chained 6.8e-7; stages 0 / 5 / 18: w 9.4e-8 .. 1.05e-7; tiny 35 / 8 / 4
  Feature-  isolated worst (content layer) B=1 2.4e-6, B=3 2.0e-6, B=8 2.1e-6 (2.4-2.9x the float32 mirror's 8.3e-7), blocks below 1e-6; chained content 1.9e-6 .. 2.3e-6, latents
  Style     5.6e-7 .. 6.6e-7; row 7 of B=8 vs alone: blocks 7.2e-8, chained content 1.4e-6; s1pp = 46 and five s2v2 / s2big per forward; with
            the stride-2 S-form route off (B=3): four s2gen, content 2.4e-6 chained / 2.1e-6 isolated
Batch 1 repeated after the matrix is bit-equal to the first run for all three encoders.  Nothing was over a bar, so no kernel changed.
The module takes about 30 s on the GPU machine (float64 references of eight images: 9.5 s, 6.7 s and 5.6 s on 16 threads; the HIP side ~1 s each).

Finding on the dispatch: Feature-Style's stride-2 convs carry no BatchNorm in front (only the stride-1 first conv of a block does), so with
the default switches they take the S-form route like every other stride-2 conv of the three encoders and s2gen is on no default path at any
batch size.  The matrix holds one extra Feature-Style pass with that route switched off (what OODGAN_ENC_SMALL_S2_SFORM=0 selects), so the
fp32-input stride-2 branch of ``_conv3x3`` is under the same bars and the dispatch union does contain s2gen."""
import os
import time

import pytest
import torch

import encoder_ref as ER
import torch_encoder_mirror as TM

gpu = pytest.mark.gpu

BAND_BAR = 2e-6             # float32 mirror vs float64 mirror: a condition on the reference (largest measured: 1.4e-6, e4e p1; w 1.2e-6)
ROW_BAR_F64 = 1e-12         # float64 rows are independent (measured 3e-14)
CHAINED_BAR = 2e-4          # test_encoder.py / test_restyle.py
CONTENT_BAR = 1e-3          # test_restyle.py: Feature-Style content
ISOLATED_BAR = 2e-5         # test_hip_samm.py: the S-form / 8-wave conv kernels at op level
ALONE_BAR = 2 * ISOLATED_BAR
STAGE_ROWS = {0: 18, 2: 16, 3: 15, 5: 13, 6: 12, 7: 11, 18: 1}         # rows of w bit-equal to row 0 (psp_encoders.py:198-214)

FAMILIES = ('stripx', 'strip', 's1big', 's1v2', 's1pp', 'tiny', 't2big', 't2v2', 't2gen', 's2big', 's2v2', 's2gen', 'upvb', 's1big_ys',
            's2big_fuse', 's2big_dotx_sform', 's1big_g2', 's2big_g2', 'stripx_g2', 's2big_xh', 's1big_xh')
E4E_BATCHES = (1, 2, 4, 5, 8)           # both sides of B*32² <= 1024 and B*16² <= 1024, and the bench / CLI batch
OTHER_BATCHES = (1, 3, 8)
ALONE_E4E, ALONE_OTHER = (0, 4, 7), (7,)
# conv families with a non-zero count in ONE chained forward, per batch size (default tunables): what the matrix covers, not a
# correctness bar.  Pinned from the first run (the stride-2 split between s2big and s2v2 follows s2_fuse_supported's work-item rule).
_TRUNK = {'s1big', 's1v2', 's1pp', 'tiny'}
DISPATCH = {
    'e4e': {1: _TRUNK | {'s2big', 's2v2'}, 2: _TRUNK | {'s2big', 's2v2'}, 4: _TRUNK | {'s2big', 's2v2'}, 5: _TRUNK | {'s2big', 's2v2'},
            8: _TRUNK | {'s2big'}},
    'restyle': {1: _TRUNK | {'s2v2'}, 3: _TRUNK | {'s2big', 's2v2'}, 8: _TRUNK | {'s2big'}},
    'fs': {1: {'s1pp', 's2v2'}, 3: {'s1pp', 's2big', 's2v2'}, 8: {'s1pp', 's2big'}},
}
FP32_S2 = 'B=3, stride 2 on the fp32-input kernel'
TUNING_ENV = ('OODGAN_TINY_MID_MAX', 'OODGAN_ENC_TRUNK_TINY_MAX', 'OODGAN_ENC_SMALL_S2_SFORM', 'OODGAN_HEADS_TINY',
              'OODGAN_HEADS_TINY_MAX_OUT', 'OODGAN_HEADS_SFORM_MIN_IN', 'OODGAN_S1_BIG_MIN_ITEMS', 'OODGAN_S2_BIG_MIN_ITEMS')


# ------------------------------------------------------------------ the reference itself (CPU)
@pytest.mark.parametrize('kind', ['e4e', 'restyle', 'fs'])
def test_float32_mirror_stays_in_its_band_of_the_float64_mirror(kind):
    """The reference is sound: its float32 evaluation agrees with its float64 one to float32 rounding, tensor by tensor."""
    x = ER.images(kind, 2)
    t0 = time.time()
    t32, t64 = ER.trace(kind, x), ER.reference(kind, 2)
    band = {name: ER.rel_err(a, b) for (name, a), (_, b) in zip(ER.flat(t32), ER.flat(t64))}
    if kind == 'e4e':
        for s in (0, 2, 3, 6, 7, 18):
            band[f'w@stage{s}'] = ER.rel_err(ER.stage_w(t32['deltas'], s), ER.stage_w(t64['deltas'], s))
    print(f'[{kind}] float32 vs float64 mirror ({time.time() - t0:.1f} s): ' + ' '.join(f'{k}={v:.1e}' for k, v in band.items()))
    assert all(torch.isfinite(b).all() for _, b in ER.flat(t64))
    over = {k: v for k, v in band.items() if not v < BAND_BAR}
    assert not over, over
    # the trace is the mirror: same w (and content) as the forward that test_encoder.py pins to the original's vectors
    m = ER.model(kind)
    with torch.no_grad():
        fwd = {'e4e': TM.encoder4editing_forward, 'restyle': TM.progressive_backbone_forward, 'fs': TM.fs_encoder_forward}[kind](m, x[:1])
    w = fwd[0] if kind == 'fs' else fwd
    assert ER.rel_err(w, t64['w'][:1]) < BAND_BAR
    if kind == 'fs':
        assert ER.rel_err(fwd[1], t64['content'][:1]) < BAND_BAR


@pytest.mark.parametrize('kind', ['e4e', 'restyle', 'fs'])
def test_float64_rows_are_independent(kind):
    """Row 1 of a float64 batch of two is image 1 alone: the eight-image reference may be sliced for every smaller batch."""
    both = ER.reference(kind, 2)
    alone = ER.trace(kind, ER.images(kind, 2)[1:], torch.float64)
    err = {name: ER.rel_err(a[1:], b) for (name, a), (_, b) in zip(ER.flat(both), ER.flat(alone))}
    print(f'[{kind}] float64 row 1 of 2 vs alone: worst {max(err.values()):.1e}')
    assert max(err.values()) <= ROW_BAR_F64, {k: v for k, v in err.items() if v > ROW_BAR_F64}
    assert not torch.equal(both['w'][0], both['w'][1])


def test_stage_table_of_the_mirror():
    """progressive_stage -> how many rows of w are delta_0 alone (psp_encoders.py:198-214), on the mirror's own forward; the trace's
    ``stage_w`` builds the same w from the deltas."""
    from oodgan.encoder import ProgressiveStage
    x = ER.images('e4e', 1)
    t32 = ER.trace('e4e', x)
    enc = ER.model('e4e')
    try:
        for s in (0, 2, 3, 6, 7, 18):
            enc.set_progressive_stage(ProgressiveStage(s))
            with torch.no_grad():
                w = TM.encoder4editing_forward(enc, x)
            assert ER.rows_equal_to_first(w) == STAGE_ROWS[s], (s, ER.rows_equal_to_first(w))
            ws = ER.stage_w(t32['deltas'], s)
            assert ER.rows_equal_to_first(ws) == STAGE_ROWS[s]
            assert ER.rel_err(ws, w) < BAND_BAR, (s, ER.rel_err(ws, w))
    finally:
        enc.set_progressive_stage(ProgressiveStage.Inference)


# ------------------------------------------------------------------ the HIP encoders (GPU)
@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


def _hip_encoder(kind, dev):
    from oodgan import encoder_hip as EH
    cls = {'e4e': EH.Encoder4EditingHIP, 'restyle': EH.ProgressiveBackboneEncoderHIP, 'fs': EH.fs_encoder_v2HIP}[kind]
    return ER.build(kind, cls).to(dev)


def _f32(t):
    return t.to(torch.float32).contiguous()


def _chained(kind, enc, x):
    """the encoder's own forward -> {name: tensor}, named as the trace names them"""
    if kind == 'fs':
        lats, content, taps = enc(x, return_feats=True)
        out = {'w': lats, 'content': content}
    else:
        w, taps = enc(x, return_feats=True)
        out = {'w': w}
    out.update({f'taps[{i}]': t for i, t in enumerate(taps)})
    return out


def _isolated(kind, enc, ref):
    """every unit of the trunk on the reference's input to it -> [(name, HIP output, reference output)]; the first unit's input is the
    image, so its isolated output is the chained tap 0 and is not repeated here"""
    u = ref['units']
    if kind == 'fs':
        res = [(f'block {name}', enc._block(name, blk, _f32(u[i])), u[i + 1]) for i, (name, blk) in enumerate(ER.fs_blocks(enc))]
        return res + [('content', enc._content(_f32(u[21])), ref['content'])]
    return [(f'unit {i}', enc._unit(i, layer, _f32(u[i])), u[i + 1]) for i, layer in enumerate(enc.body)]


def _iso_keys(kind):
    """[(name of an isolated output, name of the same tensor in the trace)]"""
    if kind == 'fs':
        return [(f'block {name}', f'units[{i + 1}]') for i, (name, _) in enumerate(ER.fs_blocks(ER.model(kind)))] + [('content', 'content')]
    return [(f'unit {i}', f'units[{i + 1}]') for i in range(24)]


def _heads(kind, enc, ref):
    """the style heads (and e4e's FPN) on the reference's maps -> [(name, HIP output, reference output)]"""
    from oodgan import encoder_hip as EH, samm
    if kind == 'fs':
        return []
    u = ref['units']
    c3 = _f32(u[24])                    # ONE tensor object per map: _style_heads groups the heads by id() of their input
    if kind == 'restyle':
        d = enc._style_heads(list(range(18)), {i: c3 for i in range(18)})
        return [('deltas', torch.stack([d[i] for i in range(18)], 1), ref['deltas'])]
    p2, p1 = _f32(ref['p2']), _f32(ref['p1'])
    d = enc._style_heads(list(range(18)), {i: c3 if i < enc.coarse_ind else (p2 if i < enc.middle_ind else p1) for i in range(18)})
    l1, l2 = enc.latlayer1, enc.latlayer2
    fp2 = EH._resize_bicubic_ac(c3, u[21].shape[-2:], add=samm.conv1x1(_f32(u[21]), l1.weight.detach(), l1.bias.detach()))
    fp1 = EH._resize_bicubic_ac(p2, u[7].shape[-2:], add=samm.conv1x1(_f32(u[7]), l2.weight.detach(), l2.bias.detach()))
    return [('deltas', torch.stack([d[i] for i in range(18)], 1), ref['deltas']), ('p2', fp2, ref['p2']), ('p1', fp1, ref['p1'])]


def _run_matrix(kind, dev, batches, alone):
    """One encoder instance over ``batches`` (rows 0..B-1 of the eight images), batch 1 again, then each image of ``alone`` by itself.
    Returns the error tables; nothing is asserted here."""
    from oodgan import _lib, encoder_hip as EH
    t0 = time.time()
    ref8 = ER.reference(kind, 8)
    t_ref = time.time() - t0
    f32, f64 = dict(ER.flat(ER.trace(kind, ER.images(kind, 8)))), dict(ER.flat(ref8))
    band = {name: ER.rel_err(f32[key], f64[key]) for name, key in _iso_keys(kind)}        # the float32 mirror's own rounding, unit by unit
    del f32, f64
    ref8 = _to(ref8, dev)
    ER.forget(kind)               # the host copy (~1 GB per encoder) is not needed again
    imgs = ER.images(kind, 8).to(dev)
    enc = _hip_encoder(kind, dev)
    big = max(batches)
    passes = [(f'B={B}', slice(0, B)) for B in batches] + [('B=1 again', slice(0, 1))] + [(f'image {k} alone', slice(k, k + 1)) for k in alone if k]
    if kind == 'fs':
        passes.append((FP32_S2, slice(0, 3)))
    R = {'chained': {}, 'isolated': {}, 'heads': {}, 'counts': {}, 'alone': {}, 'finite': True, 'enc': enc, 'repeat_bit_equal': None, 'band': band,
         'deltas64': ref8.get('deltas'), 'imgs': imgs}
    kept, first = {}, None                # rows of the biggest batch's outputs, for the row-independence check
    for label, rows in passes:
        ref = ER.tree_rows(ref8, rows)
        small_s2 = EH.SMALL_S2_SFORM
        try:
            if label == FP32_S2:            # what OODGAN_ENC_SMALL_S2_SFORM=0 selects: _conv3x3's route through _pad_tl and the fp32-input kernel
                EH.SMALL_S2_SFORM = 0
            _lib.dispatch_reset()
            ch = _chained(kind, enc, imgs[rows])
            torch.cuda.synchronize()
            R['counts'][label] = {f: _lib.dispatch_count(f) for f in FAMILIES if _lib.dispatch_count(f)}
            iso, hd = _isolated(kind, enc, ref), _heads(kind, enc, ref)
        finally:
            EH.SMALL_S2_SFORM = small_s2
        named = dict(ER.flat(ref))
        R['chained'][label] = {k: ER.rel_err(v, named[k]) for k, v in ch.items()}
        R['isolated'][label] = {n: ER.rel_err(a, b) for n, a, b in iso}
        R['heads'][label] = {n: ER.rel_err(a, b) for n, a, b in hd}
        outs = {**{'chained ' + k: v for k, v in ch.items()}, **{n: a for n, a, _ in iso + hd}}
        R['finite'] = R['finite'] and all(bool(torch.isfinite(v).all()) for v in outs.values())
        if label == 'B=1':
            first = {k: v.clone() for k, v in ch.items()}
        if label == 'B=1 again':
            R['repeat_bit_equal'] = all(torch.equal(v, first[k]) for k, v in ch.items())
        if label == f'B={big}':
            refmax = {'chained ' + k: named[k] for k in ch}
            refmax.update({n: b for n, _, b in iso + hd})
            kept = {k: (v.clone(), refmax[k].abs().max().item()) for k, v in outs.items()}
        elif rows.start in alone and rows.stop == rows.start + 1 and label != 'B=1':
            k = rows.start
            R['alone'][k] = {n: ((kept[n][0][k:k + 1].double() - v.double()).abs().max().item() / kept[n][1]) for n, v in outs.items()}
    R['seconds'] = (t_ref, time.time() - t0)
    _report(kind, R)
    return R


def _to(t, dev):
    if isinstance(t, dict):
        return {k: _to(v, dev) for k, v in t.items()}
    if isinstance(t, list):
        return [_to(v, dev) for v in t]
    return t.to(dev)


def _worst(d):
    k = max(d, key=d.get)
    return k, d[k]


def _report(kind, R):
    print(f'[{kind}] float64 reference of 8 images {R["seconds"][0]:.1f} s, whole matrix {R["seconds"][1]:.1f} s; '
          f'batch 1 repeated after the matrix bit-equal to the first: {R["repeat_bit_equal"]}; all finite: {R["finite"]}')
    for label in R['chained']:
        ck, cv = _worst(R['chained'][label])
        ik, iv = _worst(R['isolated'][label])
        line = (f'[{kind}] {label}: chained worst {ck} {cv:.2e} (w {R["chained"][label]["w"]:.2e}); isolated worst {ik} {iv:.2e} = '
                f'{iv / R["band"][ik]:.1f}x the float32 mirror\'s {R["band"][ik]:.1e} there')
        if R['heads'][label]:
            line += '; heads ' + ' '.join(f'{k} {v:.2e}' for k, v in R['heads'][label].items())
        print(line + '; dispatch ' + ' '.join(f'{f}={n}' for f, n in R['counts'][label].items()))
    for k, d in R['alone'].items():
        ck, cv = _worst({n: v for n, v in d.items() if n.startswith('chained')})
        ik, iv = _worst({n: v for n, v in d.items() if not n.startswith('chained')})
        print(f'[{kind}] row {k} of the biggest batch vs image {k} alone: {ck} {cv:.2e}; isolated / heads worst {ik} {iv:.2e}')


@pytest.fixture(scope='module')
def e4e(dev):
    return _run_matrix('e4e', dev, E4E_BATCHES, ALONE_E4E)


@pytest.fixture(scope='module')
def restyle(dev):
    return _run_matrix('restyle', dev, OTHER_BATCHES, ALONE_OTHER)


@pytest.fixture(scope='module')
def fs(dev):
    return _run_matrix('fs', dev, OTHER_BATCHES, ALONE_OTHER)


def _over(table, bar):
    """{pass: {name: err}} -> the entries not below ``bar(name)``"""
    return {f'{label}: {n}': f'{v:.2e}' for label, d in table.items() for n, v in d.items() if not v <= bar(n)}


@gpu
@pytest.mark.parametrize('kind', ['e4e', 'restyle', 'fs'])
def test_chained_forward_vs_float64(kind, request):
    R = request.getfixturevalue(kind)
    assert R['finite']
    # no float atomics and no range scale carried from call to call in the encoders: batch 1 after the other batch sizes is the first run bit for bit
    assert R['repeat_bit_equal']
    over = _over(R['chained'], lambda n: CONTENT_BAR if n == 'content' else CHAINED_BAR)
    assert not over, over


@gpu
@pytest.mark.parametrize('kind', ['e4e', 'restyle', 'fs'])
def test_isolated_units_vs_float64(kind, request):
    """Every residual unit on the reference's input to it, at every batch size; the unit fed the image itself (input layer / stem) is
    the chained tap 0, held to the same bar."""
    R = request.getfixturevalue(kind)
    iso = {label: dict(d, **{'input layer': R['chained'][label]['taps[0]']}) for label, d in R['isolated'].items()}
    assert all(len(d) == (26 if kind == 'fs' else 25) for d in iso.values())
    over = _over(iso, lambda n: ISOLATED_BAR)
    assert not over, over


@gpu
@pytest.mark.parametrize('kind', ['e4e', 'restyle'])
def test_style_heads_and_fpn_vs_float64(kind, request):
    R = request.getfixturevalue(kind)
    assert all(set(d) == ({'deltas', 'p2', 'p1'} if kind == 'e4e' else {'deltas'}) for d in R['heads'].values())
    over = _over(R['heads'], lambda n: ISOLATED_BAR)
    assert not over, over


@gpu
@pytest.mark.parametrize('kind', ['e4e', 'restyle', 'fs'])
def test_rows_of_the_batch_of_eight_vs_alone(kind, request):
    R = request.getfixturevalue(kind)
    assert sorted(R['alone']) == sorted(ALONE_E4E if kind == 'e4e' else ALONE_OTHER)
    over = _over({f'row {k}': d for k, d in R['alone'].items()}, lambda n: ALONE_BAR)
    assert not over, over


@gpu
@pytest.mark.parametrize('kind', ['e4e', 'restyle', 'fs'])
def test_dispatch_follows_the_batch_size(kind, request):
    set_ = [v for v in TUNING_ENV if v in os.environ]
    if set_:
        pytest.skip(f'dispatch tunables set in the environment ({set_}): the default thresholds this test pins do not apply')
    R = request.getfixturevalue(kind)
    c = R['counts']
    tiny = {label: d.get('tiny', 0) for label, d in c.items()}
    union = set().union(*c.values())
    if kind == 'e4e':
        # tiny_shape with tiny_mid_max = 1024: the 32² trunk convs leave the skinny-GEMM kernel above B = 1, the 16² ones above B = 4
        assert tiny['B=1'] > tiny['B=2'] == tiny['B=4'] > tiny['B=5'] == tiny['B=8'], tiny
        assert tiny['B=1 again'] == tiny['B=1']
        assert {'tiny', 's1big', 's2big', 's1pp'} <= union, sorted(union)
    elif kind == 'restyle':
        assert tiny['B=1'] > tiny['B=3'] > tiny['B=8'], tiny
        assert {'tiny', 's1big', 's2big', 's1pp'} <= union, sorted(union)
    else:
        # BatchNorm before a conv = in_scale / in_shift of the fp32-input kernels.  Only the stride-1 first conv of a block has one, so with
        # the default switches every stride-2 conv of this encoder (as of the other two) goes through the S-form and s2gen is on no
        # default path, at any batch size (first run: s1pp=46 and five s2v2 / s2big per forward); the matrix therefore holds one pass
        # with that route switched off, which puts _conv3x3's fp32-input stride-2 branch under the same bars
        assert {'s1pp', 's2gen'} <= union, sorted(union)
        assert 's2gen' in c[FP32_S2] and not any('s2gen' in d for label, d in c.items() if label != FP32_S2), c
    reached = {int(label[2:]): set(d) for label, d in c.items() if label[2:].isdigit()}
    assert reached == DISPATCH[kind], {B: sorted(s) for B, s in reached.items()}


@gpu
@pytest.mark.parametrize('kind,stages', [('e4e', (0, 2, 3, 6, 7, 18)), ('restyle', (0, 5, 18))])
def test_progressive_stages(kind, stages, request):
    """Below Inference fewer than 18 heads run: other head sets join at coarse_ind / middle_ind and w is assembled by the per-head loop,
    not from the stacked output.  B = 3; the rows above the stage are copies of delta_0, bit for bit."""
    from oodgan.encoder import ProgressiveStage
    R = request.getfixturevalue(kind)
    enc, x = R['enc'], R['imgs'][:3]
    fails = []
    try:
        for s in stages:
            enc.set_progressive_stage(ProgressiveStage(s))
            w = enc(x)
            ref = ER.stage_w(R['deltas64'][:3], s)
            err, rows = ER.rel_err(w, ref), ER.rows_equal_to_first(w)
            print(f'[{kind}] stage {s}: w vs float64 {err:.2e}, rows equal to row 0: {rows}')
            assert w.shape == (3, 18, 512) and torch.isfinite(w).all()
            if not err <= CHAINED_BAR:
                fails.append(f'stage {s}: w {err:.2e}')
            if rows != STAGE_ROWS[s]:
                fails.append(f'stage {s}: {rows} rows equal row 0, expected {STAGE_ROWS[s]}')
    finally:
        enc.set_progressive_stage(ProgressiveStage.Inference)
    assert not fails, fails
