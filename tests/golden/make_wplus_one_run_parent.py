#!/usr/bin/env python3
"""Generate tests/golden/wplus_one_run_parent.npz on the MI355X, on the commit BEFORE the hipGraph replay of the W+ step became a third
replay kind of engine._WRun (that commit's WPlusInverter._invert_graph with its own step, state and replay loop).

The cases only use WPlusInverter's public surface, so this file and tests/wplus_one_run_cases.py run unchanged in a checkout of that
commit (copy both in, build its library, run this script there, copy the .npz back):

    python tests/golden/make_wplus_one_run_parent.py [OUT.npz]

Stored (tests/wplus_one_run_cases.py lists the cases; the inputs are seeded and regenerated, not stored): per case and run the float32
bits of the losses, the SHA-256 of the latents' bytes, last_stats and the library's dispatch counters."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.dont_write_bytecode = True
for p in (os.path.join(ROOT, 'ood-gan-inversion_amd'), os.path.dirname(HERE)):
    sys.path.insert(0, p)

import wplus_one_run_cases as WC  # noqa: E402


def main():
    if not torch.cuda.is_available():
        raise SystemExit('the fixture is what the loop computes on the GPU')
    dev = torch.device('cuda:0')
    out = {'counter_names': np.array(WC.COUNTERS)}
    for name in WC.CASES:
        for mode, rec in WC.record(name, dev).items():
            for k, v in rec.items():
                out[f'{name}/{mode}/{k}'] = v
            print(f'{name} {WC.CASES[name]} {mode}: steps_run {rec["steps_run"].tolist()}, rollbacks {rec["rollbacks"].tolist()}, '
                  f'last losses {rec["loss_bits"][-1].view(np.float32).tolist()}, '
                  f'counters {dict((c, int(n)) for c, n in zip(WC.COUNTERS, rec["counters"]) if n)}', flush=True)
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, 'wplus_one_run_parent.npz')
    np.savez_compressed(path, **out)
    print(f'wrote {path} ({os.path.getsize(path)} bytes)')


if __name__ == '__main__':
    main()
