"""Derive the loose bounds of the SAW GPU tests: how far an fp32 evaluation of the contract of rgda_saw_loss
(tests/saw_ref.py::saw_emulated: fp32 sigmoid, scaled planes, products and sums; no bf16) lies from float64
(saw_restated), on the golden inputs and on the production-shape inputs of the GPU test.  Runs on the CPU:
    python tests/golden/derive_saw_tolerances.py
Writes saw_tolerances.json: per case (every golden case by its name, and 'production') the observed deviations (the
largest over eight pixel orders, see deviation()) and the bound of that case = margin * its own deviation with margin
3, the margin of the project's other derived tolerances.

loss_rel is stated relative to sum over the active groups of s / (nod B), not to the loss: s - margin cancels, so a bound
relative to the loss itself would measure the margin.  grad_rel is the relative norm of the gradient deviation; the GPU
test adds the bf16 store of the gradient to it."""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from saw_ref import golden_cases, production_inputs, saw_emulated, saw_restated  # noqa: E402

MARGIN = 3.0
ORDERS = 8


def loss_scale(r, b):
    """sum over the active groups of s / (nod B): what the loss deviation is measured against"""
    return (r['s'][r['active']].sum() / (r['nod'] * b)).item()


def deviation_once(feats, W, selected, relax_denom):
    ref = saw_restated(feats, W, selected, relax_denom)
    # the gradient on float64's signs and active bits: a near tie that fp32 decides the other way is the subject of the
    # GPU test's tie condition, not of a tolerance
    emu = saw_emulated(feats, W, selected, relax_denom, table=ref)
    assert (emu['active'] == ref['active']).all()
    return dict(loss_rel=abs(emu['loss'].item() - ref['loss'].item()) / loss_scale(ref, feats.shape[0]),
                grad_rel=((emu['grad'].double() - ref['grad']).norm() / ref['grad'].norm()).item())


def deviation(feats, W, selected, relax_denom, orders=ORDERS):
    """The loss is a sum of a few fp32 roundings, so the deviation of ONE evaluation is a draw that can land near zero
    (4.9e-9 was seen where a single rounding of the result is 6e-8) and says little about another order of the same
    sums -- and the kernel's order (thread-strided partials, butterflies) is another one, as is the reference's.  The
    loss does not depend on the order of the pixels, the fp32 sums do: the emulation is evaluated in the stored order and
    in ORDERS - 1 seeded pixel permutations, and the largest deviation is recorded."""
    b, k, h, w = feats.shape
    gen = torch.Generator().manual_seed(7)
    worst = deviation_once(feats, W, selected, relax_denom)
    for _ in range(orders - 1):
        perm = torch.randperm(h * w, generator=gen)
        d = deviation_once(feats.reshape(b, k, h * w)[:, :, perm].reshape(b, k, h, w), W, selected, relax_denom)
        worst = {m: max(worst[m], d[m]) for m in worst}
    return worst


def main():
    g = np.load(os.path.join(HERE, 'saw.npz'), allow_pickle=False)
    cases = {c['name']: deviation(c['feats'], c['W'], c['selected'], c['relax_denom']) for c in golden_cases(g)}
    feats, W = production_inputs()
    cases['production'] = deviation(feats, W, list(range(6)), 2.0)
    bounds = {name: {m: MARGIN * v[m] for m in ('loss_rel', 'grad_rel')} for name, v in cases.items()}
    out = dict(margin=MARGIN, orders=ORDERS, observed=cases, bounds=bounds)
    with open(os.path.join(HERE, 'saw_tolerances.json'), 'w') as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write('\n')
    print(json.dumps(out, indent=1, sort_keys=True))


if __name__ == '__main__':
    main()
