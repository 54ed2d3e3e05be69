"""Derive the loose bounds of the whitening GPU tests: how far the arithmetic contract of rgda_whiten_loss (bf16 centred
operands, bf16(S - I) in the gradient product, bf16 stored gradient; tests/whiten_ref.py::whiten_emulated) lies from
float64 on the unrounded inputs (whiten_restated), on the golden inputs and on the production-shape inputs of the GPU
test.  Runs on the CPU:
    python tests/golden/derive_whiten_tolerances.py
Writes whiten_tolerances.json: per case (every golden case by its name, and 'production') the observed relative loss
deviation and the relative norm of the gradient deviation, and the bound of that case = margin * its own deviation
with margin 3, the margin of the project's other derived tolerances."""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from whiten_ref import golden_cases, production_inputs, whiten_emulated, whiten_restated  # noqa: E402

MARGIN = 3.0


def deviation(feats, labels, class_num, groups):
    ref_l, ref_g = whiten_restated(feats, labels, range(class_num), groups)
    emu_l, emu_g = whiten_emulated(feats, labels, class_num, groups)
    return dict(loss_rel=abs(emu_l.item() - ref_l.item()) / abs(ref_l.item()),
                grad_rel=((emu_g.double() - ref_g).norm() / ref_g.norm()).item())


def main():
    g = np.load(os.path.join(HERE, 'whiten.npz'), allow_pickle=False)
    cases = {c['name']: deviation(c['feats'], c['labels'], c['class_num'], c['groups']) for c in golden_cases(g)}
    feats, labels = production_inputs()
    cases['production'] = deviation(feats, labels, 6, 32)
    bounds = {name: {m: MARGIN * v[m] for m in ('loss_rel', 'grad_rel')} for name, v in cases.items()}
    out = dict(margin=MARGIN, observed=cases, bounds=bounds)
    with open(os.path.join(HERE, 'whiten_tolerances.json'), 'w') as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write('\n')
    print(json.dumps(out, indent=1, sort_keys=True))


if __name__ == '__main__':
    main()
