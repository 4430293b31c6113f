"""TEST INFRASTRUCTURE — per-unit traces of the three encoder graphs through the plain-torch mirror (torch_encoder_mirror.py), in
float32 or float64, for tests that compare the HIP encoders unit by unit (test_hip_encoder_batched.py).

A trace walks the same building blocks as the mirror's forwards (``TM._input_layer``, ``TM._bottleneck``, ``TM._gradual_style``,
``TM._upsample_add``, ``TM._ibasic``) and keeps every intermediate: the output of the input layer and of each residual unit, the
FPN maps, every style head's delta.  ``w`` is assembled from the deltas for any progressive stage (psp_encoders.py:198-214: row 0 is
delta_0, rows 1..stage are delta_0 + delta_i, the rows above are copies of delta_0), so one trace serves all stages; the CPU tests pin
that assembly against the mirror's own forward at every stage they use."""
import torch

import torch_encoder_mirror as TM
from oodgan import synth

E4E_TAPS = (0, 3, 7, 21, 24)            # index into ``units`` (0 = input layer, i + 1 = body[i]) of the five feature taps
FS_TAPS = (0, 3, 7, 21)                 # stem, block_1, block_2, block_3 of fs_encoder_v2 (3 / 4 / 14 / 3 IBasicBlocks)


_STATES = {}


def _container(kind, cls=None):
    from oodgan import encoder as E
    if kind == 'e4e':
        return (cls or E.Encoder4Editing)(50, 'ir_se', {'stylegan_size': 1024}, bn=True)
    if kind == 'restyle':
        return (cls or E.ProgressiveBackboneEncoder)(50, 'ir_se', 18, {'encoder_type': 'ProgressiveBackboneEncoder', 'input_nc': 6})
    assert kind == 'fs', kind
    return (cls or E.fs_encoder_v2)(18, stride=(2, 2))


def state(kind):
    """The recipe weights the other tests use (test_encoder.py, test_restyle.py), generated once per process."""
    if kind not in _STATES:
        if kind == 'e4e':
            with torch.device('meta'):
                shapes = {k: tuple(v.shape) for k, v in _container(kind).state_dict().items()}
            _STATES[kind] = synth.encoder_state(shapes, seed=41)
        elif kind == 'restyle':
            ck = synth.restyle_checkpoint(seed=51)
            assert ck['opts'] == {'encoder_type': 'ProgressiveBackboneEncoder', 'input_nc': 6}
            _STATES[kind] = {k[len('encoder.'):]: v for k, v in ck['state_dict'].items()}
        else:
            _STATES[kind] = synth.featurestyle_state(seed=61)
    return _STATES[kind]


def build(kind, cls=None, dtype=torch.float32):
    """The parameter container (or ``cls``, its HIP subclass) of encoder ``kind`` holding ``state(kind)`` in ``dtype``; built on the meta
    device and filled by assignment (the containers' own random initialisation of ~2e8 parameters is seconds of CPU time)."""
    with torch.device('meta'):
        enc = _container(kind, cls)
    sd = {k: (v.to(dtype) if v.is_floating_point() else v.clone()) for k, v in state(kind).items()}
    enc.load_state_dict(sd, strict=True, assign=True)
    return enc.eval()


def images(kind, n):
    """n distinct 256² inputs (float32): image k from seeds of its own, so no two rows are equal; ReStyle's six channels are two images."""
    if kind == 'restyle':
        return torch.cat([torch.cat([synth.make_images(256, 1, seed=200 + 2 * k), synth.make_images(256, 1, seed=201 + 2 * k)], 1)
                          for k in range(n)])
    base = 100 if kind == 'e4e' else 300
    return torch.cat([synth.make_images(256, 1, seed=base + k) for k in range(n)])


def stage_w(deltas, stage):
    """(B, n, 512) head deltas -> w of progressive stage ``stage`` (18 = Inference)."""
    n = deltas.shape[1]
    w = deltas[:, :1].repeat(1, n, 1)
    top = min(stage + 1, n)
    w[:, 1:top] += deltas[:, 1:top]
    return w


def rows_equal_to_first(w):
    """How many of w's latent rows are bit-equal to row 0 (row 0 included)."""
    return sum(int(torch.equal(w[:, i], w[:, 0])) for i in range(w.shape[1]))


def _trunk(enc, x):
    units = [TM._input_layer(enc.input_layer, x)]
    for layer in enc.body:
        units.append(TM._bottleneck(layer, units[-1]))
    return units


def e4e_trace(enc, x):
    units = _trunk(enc, x)
    c1, c2, c3 = units[7], units[21], units[24]
    p2 = TM._upsample_add(c3, TM._conv(enc.latlayer1, c2))
    p1 = TM._upsample_add(p2, TM._conv(enc.latlayer2, c1))
    feat = lambda i: c3 if i < enc.coarse_ind else (p2 if i < enc.middle_ind else p1)
    deltas = torch.stack([TM._gradual_style(enc.styles[i], feat(i)) for i in range(enc.style_count)], 1)
    return {'units': units, 'taps': [units[i] for i in E4E_TAPS], 'p2': p2, 'p1': p1, 'deltas': deltas, 'w': stage_w(deltas, 18)}


def restyle_trace(enc, x):
    units = _trunk(enc, x)
    deltas = torch.stack([TM._gradual_style(s, units[-1]) for s in enc.styles], 1)
    return {'units': units, 'taps': [units[i] for i in E4E_TAPS], 'deltas': deltas, 'w': stage_w(deltas, 18)}


def fs_blocks(enc):
    """[(name the HIP encoder packs the block's weights under, block)] in forward order."""
    return [(f'b{s}.{i}', blk) for s in (1, 2, 3, 4) for i, blk in enumerate(getattr(enc, f'block_{s}'))]


def fs_trace(enc, x):
    units = [TM._input_layer(enc.conv, x)]
    for _, blk in fs_blocks(enc):
        units.append(TM._ibasic(blk, units[-1]))
    c = enc.content_layer
    content = TM._bn(c[5], TM._conv(c[4], torch.nn.functional.prelu(TM._bn(c[2], TM._conv(c[1], TM._bn(c[0], units[21]))), c[3].weight)))
    pooled = [torch.nn.functional.adaptive_avg_pool2d(units[i], (3, 3)) for i in (3, 7, 21, 24)]
    d = torch.cat(pooled, dim=1).flatten(1)
    lats = torch.stack([torch.nn.functional.linear(d, s.weight, s.bias) for s in enc.styles], dim=1)
    return {'units': units, 'taps': [units[i] for i in FS_TAPS], 'content': content, 'w': lats}


TRACE = {'e4e': e4e_trace, 'restyle': restyle_trace, 'fs': fs_trace}
_MODELS, _REFS = {}, {}


def model(kind, dtype=torch.float32):
    key = (kind, dtype)
    if key not in _MODELS:
        _MODELS[key] = build(kind, dtype=dtype)
    return _MODELS[key]


def trace(kind, x, dtype=torch.float32):
    with torch.no_grad():
        return TRACE[kind](model(kind, dtype), x.to(dtype))


def reference(kind, n):
    """The float64 trace of images(kind, n), computed once per process and sliced for smaller n (rows of the float64 mirror are
    independent to 1e-12: test_float64_rows_are_independent)."""
    have = [m for (k, m) in _REFS if k == kind and m >= n]
    if not have:
        _REFS[(kind, n)] = trace(kind, images(kind, n), torch.float64)
        have = [n]
    return tree_rows(_REFS[(kind, min(have))], slice(0, n))


def forget(kind):
    """Drop the cached float64 traces of ``kind``."""
    for key in [k for k in _REFS if k[0] == kind]:
        del _REFS[key]


def tree_rows(t, rows):
    if isinstance(t, dict):
        return {k: tree_rows(v, rows) for k, v in t.items()}
    if isinstance(t, list):
        return [tree_rows(v, rows) for v in t]
    return t[rows]


def flat(t, prefix=''):
    """trace -> [(name, tensor)]."""
    if isinstance(t, dict):
        return [p for k, v in t.items() for p in flat(v, f'{prefix}{k}')]
    if isinstance(t, list):
        return [p for i, v in enumerate(t) for p in flat(v, f'{prefix}[{i}]')]
    return [(prefix, t)]


def rel_err(a, ref):
    """max|a - ref| / max|ref| in the reference's precision, no floor on the denominator."""
    ref = ref.to(torch.float64)
    return ((a.to(ref.device, torch.float64) - ref).abs().max() / ref.abs().max()).item()
