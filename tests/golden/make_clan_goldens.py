"""Mint clan.npz from the reference's OWN WeightedBCEWithLogitsLoss (regda/loss.py:60-85, imported behind the stubs of
_refstubs.py, on the CPU).

Run where the reference checkout exists only:
    python tests/golden/make_clan_goldens.py
Data only, a few kilobytes.  The inputs are float32 values (tests/clan_ref.py draws them: logits with +-80, which pin the
stable form, a domain label or a soft target, a weight in [0, 1], both size_average values, weight None); the reference's
module is evaluated on them in float64, so the stored loss and autograd gradients are exact to 1e-15 and every float32
implementation is measured against the same numbers.  Keys: <case>_input, _target, _weight (absent for weight None),
_alpha, _beta, _size_average, _loss, _dinput, _dweight (absent for weight None)."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import _refstubs  # noqa: E402

_refstubs.install()

from regda.loss import WeightedBCEWithLogitsLoss  # noqa: E402
import clan_ref as C  # noqa: E402


def main():
    out = {}
    for name in C.GOLDEN_CASES:
        c = C.golden_inputs(name)
        x = c['input'].double().requires_grad_(True)
        w = None if c['weight'] is None else c['weight'].double().requires_grad_(True)
        loss = WeightedBCEWithLogitsLoss(size_average=c['size_average'])(x, c['target'].double(), w, c['alpha'], c['beta'])
        loss.backward()
        assert torch.isfinite(loss) and torch.isfinite(x.grad).all() and float(c['input'].abs().max()) == 80.0
        out[name + '_input'], out[name + '_target'] = c['input'].numpy(), c['target'].numpy()
        out[name + '_loss'], out[name + '_dinput'] = loss.detach().numpy(), x.grad.numpy()
        out[name + '_alpha'], out[name + '_beta'] = np.float64(c['alpha']), np.float64(c['beta'])
        out[name + '_size_average'] = np.bool_(c['size_average'])
        if w is not None:
            out[name + '_weight'], out[name + '_dweight'] = c['weight'].numpy(), w.grad.numpy()
    path = os.path.join(HERE, 'clan.npz')
    np.savez_compressed(path, **out)
    assert os.path.getsize(path) < (1 << 20)
    load = lambda fn: np.load(os.path.join(HERE, fn), allow_pickle=False)      # noqa: E731
    for name in C.GOLDEN_CASES:
        g = C.golden_case(load, name)
        loss, dz, gw = C.golden_restatement(g)
        print(name, 'loss %.2e' % abs(float(loss - g['loss']) / float(g['loss'])), 'dinput %.2e' % C.R.err(dz, g['dinput']),
              'dweight ' + ('-' if gw is None else '%.2e' % C.R.err(gw, g['dweight'])))
    print('wrote', path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
