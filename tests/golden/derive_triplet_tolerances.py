"""Derive the loose bounds of the triplet GPU tests: how far the arithmetic contract of rgda_triplet_loss (bf16 rows and
fp32 sums for the mining, fp32 distances and gradient, bf16 stored gradient; tests/triplet_ref.py::triplet_emulated)
lies from float64 on the unrounded inputs (triplet_restated), on every case of tests/triplet_ref.py (CASES and
variant_cases).  Runs on the CPU:
    python tests/golden/derive_triplet_tolerances.py
Writes triplet_tolerances.json: per case the observed deviations and the bounds of loss and gradient = margin * the
case's own deviation with margin 3, the margin of the project's other derived tolerances; mining_bound = margin * the
largest mining_rel of all cases (one value: which near-tie the bf16 mining resolves differently is chance, so a case's
own value, often 0, says nothing about the next near-tie).
    loss_rel    |L_emulated - L_float64| / L_float64 (the absolute deviation where L_float64 = 0)
    grad_rel    relative norm of the gradient deviation (0 where the float64 gradient is 0)
    mining_rel  the largest relative distance, over the rows, between the TRUE distance of the emulated selection and the
                true extremum (bf16 mining can pick a neighbouring candidate)
    index_share the share of rows whose emulated p or n differs from float64 (recorded, not a bound)"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from triplet_ref import CASES, case_inputs, mining_deviation, triplet_emulated, triplet_restated, variant_cases  # noqa: E402

MARGIN = 3.0


def deviation(x, labels, ignore_label):
    r = triplet_restated(x, labels, ignore_label=ignore_label)
    e = triplet_emulated(x, labels, ignore_label=ignore_label)
    gn = np.linalg.norm(r['grad'])
    gd = np.linalg.norm(e['grad'].double().numpy() - r['grad'])
    return dict(loss_rel=abs(e['loss'] - r['loss']) / (abs(r['loss']) if r['loss'] else 1.0),
                grad_rel=float(gd / gn) if gn else float(gd),
                mining_rel=mining_deviation(x, e['p'], e['n'], r),
                index_share=float(((e['p'] != r['p']) | (e['n'] != r['n'])).mean()))


def main():
    cases = {name: deviation(*case_inputs(name), None) for name in CASES}
    cases.update({name: deviation(*v) for name, v in variant_cases().items()})
    bounds = {name: {m: MARGIN * v[m] for m in ('loss_rel', 'grad_rel')} for name, v in cases.items()}
    mining = MARGIN * max(v['mining_rel'] for v in cases.values())
    out = dict(margin=MARGIN, observed=cases, bounds=bounds, mining_bound=mining)
    with open(os.path.join(HERE, 'triplet_tolerances.json'), 'w') as fh:
        json.dump(out, fh, indent=1, sort_keys=True)
        fh.write('\n')
    print(json.dumps(out, indent=1, sort_keys=True))


if __name__ == '__main__':
    main()
