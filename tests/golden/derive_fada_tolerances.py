"""Derive fada_tolerances.json on the CPU: no bound of the feature-adversarial tests is fixed by hand.

    python tests/golden/derive_fada_tolerances.py

For every case the GPU tests run (tests/fada_ref.py holds the cases and draws their inputs) the bound is three times the
deviation of the bf16 storage model from float64 on the same inputs plus K * 2^-24 for the longest f32 accumulation
behind an element (9 * Cin of the layer; fada_ref.head_tolerances says how that reaches the loss and dz).  For the goldens
(fada*.npz) it is three times the deviation of a float32 evaluation of the reference's formulation from the float64 one."""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import fada_ref as R  # noqa: E402

PATH = os.path.join(HERE, 'fada_tolerances.json')


def derive():
    out = dict(margin=3.0, head={}, generic={}, module={}, golden={})
    for shape in R.SHAPES:
        for Ch in R.HEAD_CHANNELS:
            for nc in R.CLASS_COUNTS:
                c = R.head_case(shape, Ch, nc)
                out['head'][R.head_name(shape, Ch, nc)] = R.head_tolerances(c, R.head_reference(c))
    for n in R.GENERIC_CASES:
        c = R.generic_case(n)
        out['generic'][n] = R.generic_tolerances(c, R.generic_reference(c))
    for n in R.MODULE_CASES:
        out['module'][n] = R.module_tolerances(R.module_case(n))
    load = lambda fn: np.load(os.path.join(HERE, fn), allow_pickle=False)      # noqa: E731
    for n in R.GOLDEN_CASES:
        out['golden'][n] = R.golden_tolerances(R.golden_case(load, n))
    return out


if __name__ == '__main__':
    tol = derive()
    json.dump(tol, open(PATH, 'w'), indent=1, sort_keys=True)
    for group in ('generic',):
        for n, t in tol[group].items():
            print(group, n, {k: '%.2e' % v for k, v in t.items()})
    for n, t in tol['module'].items():
        print('module', n, {k: '%.2e' % v for k, v in t['0'].items() if not k.startswith('opposite')})
    print('wrote', PATH)
