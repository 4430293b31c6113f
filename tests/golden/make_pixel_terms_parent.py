#!/usr/bin/env python3
"""Generate tests/golden/pixel_terms_parent.npz on the MI355X with the library of the commit BEFORE the pixel terms became one kernel
family (csrc/loss_pixel.hip): that commit's mse_kernel, composite_mse_{plane,flat}_kernel and robust_{plane,flat}_kernel.

The C ABI did not change, so this tree's host layer drives that commit's library.  Build it by the A/B route of the Makefile and point
OODGAN_LIB (oodgan/_lib.py) at it:

    cd ood-gan-inversion_amd && mkdir -p csrc_ab && git archive <parent> csrc | tar -x --strip-components=1 -C csrc_ab
    make CSRC=csrc_ab BUILD=build_ab LIB=oodgan/liboodgan_hip_parent.so
    OODGAN_LIB=$PWD/oodgan/liboodgan_hip_parent.so python ../tests/golden/make_pixel_terms_parent.py

Stored (tests/pixel_terms_cases.py lists the cases; the inputs are seeded and regenerated, not stored): per case the float32 loss values
and the SHA-256 of the raw bytes of the gradient and of the composite."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.dont_write_bytecode = True
for p in (os.path.join(ROOT, 'ood-gan-inversion_amd'), os.path.dirname(HERE)):
    sys.path.insert(0, p)

import pixel_terms_cases as PC  # noqa: E402


def main():
    if not os.environ.get('OODGAN_LIB'):
        raise SystemExit('set OODGAN_LIB to the library built from the parent commit: this tree\'s own library is what the fixture tests')
    if not torch.cuda.is_available():
        raise SystemExit('the fixture is what the kernels compute on the GPU')
    from oodgan import _lib, ops
    dev = torch.device('cuda:0')
    out = {}
    for name, shape in PC.SHAPES.items():
        losses, digests = PC.run(ops, shape, dev)
        keys = sorted(losses)
        out[f'{name}/loss_keys'] = np.array(keys)
        out[f'{name}/loss_sizes'] = np.array([losses[k].size for k in keys], dtype=np.int32)
        out[f'{name}/losses'] = np.concatenate([losses[k] for k in keys])
        keys = sorted(digests)
        out[f'{name}/digest_keys'] = np.array(keys)
        out[f'{name}/digests'] = np.frombuffer(b''.join(digests[k] for k in keys), dtype=np.uint8).reshape(len(keys), 32)
        print(f'{name} {shape}: {len(losses)} losses, {len(digests)} digests; mse {losses["mse"].tolist()}', flush=True)
    path = os.path.join(HERE, 'pixel_terms_parent.npz')
    np.savez_compressed(path, **out)
    print(f'wrote {path} ({os.path.getsize(path)} bytes) with {_lib.LIB_PATH}')


if __name__ == '__main__':
    main()
