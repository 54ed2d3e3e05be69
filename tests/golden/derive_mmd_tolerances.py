"""Derive the loose bounds of the MMD GPU tests: how far the arithmetic contract of rgda_mmd_loss (centred bf16
operands, fp32 sums, bf16 W, bf16 stored gradient; tests/mmd_ref.py::mmd_emulated) lies from float64 on the unrounded
inputs (mmd_restated), on the golden inputs and on the production-channel inputs of the GPU test.  Runs on the CPU:
    python tests/golden/derive_mmd_tolerances.py
Writes mmd_tolerances.json: per case (every golden case by its name, and 'production') the observed relative loss
deviation and the relative norm of the gradient deviation (both gradients as one vector), and the bound of that case =
margin * its own deviation with margin 3, the margin of the project's other derived tolerances."""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from mmd_ref import golden_cases, mmd_emulated, mmd_restated, production_inputs, rows_of  # noqa: E402

MARGIN = 3.0


def deviation(xs, xt, **st):
    rl, rgs, rgt = mmd_restated(xs, xt, **st)
    el, egs, egt = mmd_emulated(xs, xt, **st)
    ref, emu = torch.cat([rgs, rgt]), torch.cat([egs, egt]).double()
    return dict(loss_rel=abs(float(el) - float(rl)) / abs(float(rl)), grad_rel=((emu - ref).norm() / ref.norm()).item())


def main():
    g = np.load(os.path.join(HERE, 'mmd.npz'), allow_pickle=False)
    cases = {c['name']: deviation(c['xs'], c['xt'], **c['settings']) for c in golden_cases(g)}
    f, b = production_inputs()
    cases['production'] = deviation(rows_of(f[:b]), rows_of(f[b:]))
    bounds = {name: {m: MARGIN * v[m] for m in ('loss_rel', 'grad_rel')} for name, v in cases.items()}
    out = dict(margin=MARGIN, observed=cases, bounds=bounds)
    with open(os.path.join(HERE, 'mmd_tolerances.json'), 'w') as fh:
        json.dump(out, fh, indent=1, sort_keys=True)
        fh.write('\n')
    print(json.dumps(out, indent=1, sort_keys=True))


if __name__ == '__main__':
    main()
