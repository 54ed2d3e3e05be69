"""Derive the loose bounds of the DCA GPU tests: how far the arithmetic contract of rgda_dca_loss (fp32 softmax, fp32 sums,
bf16 gradient rows; tests/dca_ref.py::dca_emulated) lies from float64 on the same inputs (dca_restated), on every case of
tests/dca_ref.py::CASES, for both kinds (pred_kind 'logits2', ignore_bg on, as ICR: both sides receive a gradient).
    python tests/golden/derive_dca_tolerances.py
Writes dca_tolerances.json: per case and kind the observed deviations -- the loss (relative), u (relative norm over both
sides) and the gradient rows (relative norm over both sides) -- and the bounds = margin * the observed values, margin 3,
the project's usual one.  dca_emulated adds the pixels in one of two sequential orders; the observed value is the larger of
the two.  The loss is ONE fp32 number, so its observed deviation is one draw that can fall near zero by chance: it is taken
as at least one fp32 rounding, 2^-23 relative, the precision of the format the loss is returned in."""
import json
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

from dca_ref import CASES, case_inputs, dca_emulated, dca_restated, relnorm  # noqa: E402

MARGIN = 3.0


def observe(name, kind):
    sides = case_inputs(name)
    r = dca_restated(sides, 'logits2', kind, True)
    out = dict(loss_rel=2.0 ** -23, u_rel=0.0, grad_rel=0.0)
    for reverse in (False, True):
        e = dca_emulated(sides, 'logits2', kind, True, reverse=reverse)
        out['loss_rel'] = max(out['loss_rel'], abs(e['loss'] - r['loss']) / abs(r['loss']))
        out['u_rel'] = max(out['u_rel'], relnorm(torch.cat([e['u_a'], e['u_b']]), torch.cat([r['u_a'], r['u_b']])))
        out['grad_rel'] = max(out['grad_rel'], relnorm(torch.cat([e['grad_a'], e['grad_b']]),
                                                       torch.cat([r['rows_a'], r['rows_b']])))
    return out


def main():
    observed = {name: {kind: observe(name, kind) for kind in ('cov', 'mse')} for name in CASES}
    bounds = {name: {kind: {m: MARGIN * v for m, v in o.items()} for kind, o in per.items()} for name, per in observed.items()}
    with open(os.path.join(HERE, 'dca_tolerances.json'), 'w') as fh:
        json.dump(dict(margin=MARGIN, observed=observed, bounds=bounds), fh, indent=1, sort_keys=True)
    for name, per in observed.items():
        print(name, per)


if __name__ == '__main__':
    main()
