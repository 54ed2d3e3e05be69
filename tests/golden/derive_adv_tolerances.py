"""Derive adv_tolerances.json on the CPU: no bound of the adversarial tests is fixed by hand.

    python tests/golden/derive_adv_tolerances.py

For every case the GPU tests run (tests/adv_ref.py holds the cases and draws their inputs) the bound is three times the
deviation of the bf16 storage model from float64 on the same inputs -- the margin the TransNorm tests use; it covers the
accumulation-order differences the model does not capture -- plus K * 2^-24 for the longest f32 accumulation behind an
element (adv_ref's docstring).  For the goldens (adv.npz) it is three times the deviation of a float32 evaluation of the
reference's own formulation from the float64 one."""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import adv_ref as R  # noqa: E402

PATH = os.path.join(HERE, 'adv_tolerances.json')


def derive(module_cases=None):
    out = dict(margin=3.0, conv={}, probs={}, head={}, bce={}, module={}, golden={})
    for n in R.CONV_CASES:
        c = R.conv_case(n)
        out['conv'][n] = R.conv_tolerances(c, R.conv_reference(c))
    for n in R.PROBS_CASES:
        c = R.probs_case(n)
        out['probs'][n] = R.probs_tolerances(c, R.probs_reference(c))
    for n in R.HEAD_CASES:
        c = R.head_case(n)
        out['head'][n] = R.head_tolerances(c, R.head_reference(c))
    for n, size in R.BCE_SIZES.items():
        out['bce'][n] = R.bce_tolerances(size)
    for n in (R.MODULE_CASES if module_cases is None else module_cases):
        out['module'][n] = R.module_tolerances(R.module_case(n))
    load = lambda fn: np.load(os.path.join(HERE, fn), allow_pickle=False)      # noqa: E731
    for n in R.GOLDEN_CASES:
        out['golden'][n] = R.golden_tolerances(R.golden_case(load, n))
    return out


if __name__ == '__main__':
    tol = derive()
    json.dump(tol, open(PATH, 'w'), indent=1, sort_keys=True)
    for group in ('conv', 'probs', 'head', 'bce'):
        for n, t in tol[group].items():
            print(group, n, {k: '%.2e' % v for k, v in t.items()})
    for n, t in tol['module'].items():
        print('module', n, {k: '%.2e' % v for k, v in t['0'].items() if not k.startswith('opposite')})
    print('wrote', PATH)
