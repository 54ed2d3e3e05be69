"""Derive the bounds of the pixel-contrast GPU tests.  Runs on the CPU:
    python tests/golden/derive_pixel_contrast_tolerances.py
Writes pixel_contrast_tolerances.json: per case (every golden case by its name, and 'production': k = 2048, 2 x 32 x 32
from a seeded generator, tests/pixel_contrast_ref.py::production_inputs)

  observed / bounds (the LOOSE bound, kernel against float64): how far the arithmetic contract of
    rgda_pixel_contrast_loss (bf16 rows, fp32 sums, bf16 W + W^T, bf16 stored gradient;
    pixel_contrast_ref.py::contrast_emulated) lies from float64 on the unrounded inputs (contrast_restated): the relative
    loss deviation and the relative norm of the gradient deviation, the larger of the emulation's two summation orders
    (the goldens' features sit on a grid that bf16 holds exactly at scale 1, so in the saturated case the order of the
    fp32 sums is all there is); bound = margin * deviation with margin 3, the margin of the project's other derived
    tolerances.
  order / tight (the TIGHT bound, kernel against the emulated contract): the kernel and the emulation follow the same
    contract and differ in the order of their fp32 sums (and the device exp / log, a few ulp).  `order` is the deviation
    between two legitimate orders on the CPU: every sum exact and rounded once, against plain fp32 sums.  It carries the
    case's own amplification (in the saturated regime the loss is a mean of gaps G_rq - m_r between logits of order 10^3
    to 10^4 in fp32).  tight = margin * order + floor; the floors are the formats': 2^-20 for the loss (fp32 sums of some
    10^2 to 10^3 terms, as for rgda_mmd_loss) and 2^-10 for the gradient (both sides store bf16: where a last-bit
    difference of the fp32 value crosses a rounding boundary the stored values differ by 2^-8 relative; 2^-10 as a
    relative norm lets a sixteenth of the energy sit on such elements)."""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from pixel_contrast_ref import (case_rows, contrast_emulated, contrast_restated, golden_cases, pixel_rows,  # noqa: E402
                                production_inputs, production_plan)

MARGIN = 3.0
FLOOR = dict(loss_rel=2.0 ** -20, grad_rel=2.0 ** -10)


def _dev(l, g, rl, rg):
    return dict(loss_rel=abs(float(l) - float(rl)) / abs(float(rl)), grad_rel=((g.double() - rg.double()).norm() / rg.double().norm()).item())


def deviation(F, cls):
    rl, rg = contrast_restated(F, cls)
    el, eg = contrast_emulated(F, cls, sums='exact')
    fl, fg = contrast_emulated(F, cls, sums='fp32')
    a, b = _dev(el, eg, rl, rg), _dev(fl, fg, rl, rg)
    return {m: max(a[m], b[m]) for m in FLOOR}, _dev(fl, fg, el, eg)


def production_rows():
    feats, labels, predict, _ = production_inputs()
    (rows, cls), _ = production_plan(labels, predict, tuple(feats.shape[2:]))
    return pixel_rows(feats)[rows], cls


def main():
    g = np.load(os.path.join(HERE, 'pixel_contrast.npz'), allow_pickle=False)
    observed, order = {}, {}
    for c in golden_cases(g):
        rows, cls = case_rows(c)
        observed[c['name']], order[c['name']] = deviation(pixel_rows(c['feats'])[rows], cls)
    observed['production'], order['production'] = deviation(*production_rows())
    bounds = {n: {m: MARGIN * v[m] for m in FLOOR} for n, v in observed.items()}
    tight = {n: {m: MARGIN * v[m] + FLOOR[m] for m in FLOOR} for n, v in order.items()}
    out = dict(margin=MARGIN, floor=FLOOR, observed=observed, bounds=bounds, order=order, tight=tight)
    with open(os.path.join(HERE, 'pixel_contrast_tolerances.json'), 'w') as fh:
        json.dump(out, fh, indent=1, sort_keys=True)
        fh.write('\n')
    print(json.dumps(out, indent=1, sort_keys=True))


if __name__ == '__main__':
    main()
