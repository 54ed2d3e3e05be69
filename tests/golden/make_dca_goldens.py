"""Mint dca.npz from the reference's OWN regda.dca_modules (CCR, ICR, MSE_cross with multi_layer=True), on the CPU in fp32.

Run where the reference checkout exists only:
    python tests/golden/make_dca_goldens.py
Data only: inputs, the reference's loss and its autograd gradient with respect to the features.

regda/dca_modules.py imports `pearsonr` from audtorch, which is not installed: this script puts a stand-in
`audtorch.metrics.functional.pearsonr` into sys.modules, restated from that package's published definition (the centred
product sum over c - 1, divided by the product of the two unbiased standard deviations; a one-element tensor, which
the reference indexes with [0]).  What this pins: the reference's get_context, batch mean, matrix walk and regularize.

Cases (tests/dca_ref.py::CASES, structured inputs): the two smallest, each for CCR (gradient to the target features) and
ICR (the two sides concatenated to one batch, gradient to both halves), and MSE_cross on the smallest."""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import _refstubs  # noqa: E402  (only for the location of the reference checkout)


def pearsonr(x, y, batch_first=True):
    dim = -1 if batch_first else 0
    cx, cy = x - x.mean(dim=dim, keepdim=True), y - y.mean(dim=dim, keepdim=True)
    cov = (cx * cy).sum(dim=dim, keepdim=True) / (x.shape[dim] - 1)
    return cov / (x.std(dim=dim, keepdim=True) * y.std(dim=dim, keepdim=True))


for _name in ('audtorch', 'audtorch.metrics', 'audtorch.metrics.functional'):
    sys.modules[_name] = types.ModuleType(_name)
sys.modules['audtorch.metrics.functional'].pearsonr = pearsonr
sys.modules['audtorch.metrics'].functional = sys.modules['audtorch.metrics.functional']
sys.modules['audtorch'].metrics = sys.modules['audtorch.metrics']
sys.path.insert(0, _refstubs.REF)

from dca_ref import CASES, GOLDEN_NAMES, make_inputs  # noqa: E402
from regda import dca_modules as ref  # noqa: E402


def rows(g):
    return g.flatten(2).permute(0, 2, 1).reshape(-1, g.shape[1]).contiguous().numpy()


def main():
    out = {}
    for name in GOLDEN_NAMES:
        (fa, (a1, a2)), (fb, (b1, b2)) = make_inputs(*CASES[name])
        C = CASES[name][1]
        out.update({name + '_feat_a': fa.numpy(), name + '_l1_a': a1.numpy(), name + '_l2_a': a2.numpy(),
                    name + '_feat_b': fb.numpy(), name + '_l1_b': b1.numpy(), name + '_l2_b': b2.numpy()})
        xa, xb = fa.clone().requires_grad_(True), fb.clone().requires_grad_(True)
        loss = ref.CCR((a1, a2, xa), (b1, b2, xb), C, multi_layer=True, ignore_bg=True)
        loss.backward()
        assert xa.grad is None
        out.update({name + '_ccr_loss': loss.detach().numpy(), name + '_ccr_rows_b': rows(xb.grad)})
        print(name, 'CCR', loss.item())
        x = torch.cat([fa, fb]).requires_grad_(True)
        loss = ref.ICR((torch.cat([a1, b1]), torch.cat([a2, b2]), x), C, multi_layer=True, ignore_bg=True)
        loss.backward()
        nb = fa.shape[0]
        out.update({name + '_icr_loss': loss.detach().numpy(), name + '_icr_rows_a': rows(x.grad[:nb]),
                    name + '_icr_rows_b': rows(x.grad[nb:])})
        print(name, 'ICR', loss.item())
        if name == GOLDEN_NAMES[0]:
            xb = fb.clone().requires_grad_(True)
            loss = ref.MSE_cross((a1, a2, fa), (b1, b2, xb), multi_layer=True, ignore_bg=True)
            loss.backward()
            out.update({name + '_msecross_loss': loss.detach().numpy(), name + '_msecross_rows_b': rows(xb.grad)})
            print(name, 'MSE_cross', loss.item())
    out['names'] = np.array(GOLDEN_NAMES)
    np.savez_compressed(os.path.join(HERE, 'dca.npz'), **out)
    print('wrote dca.npz', os.path.getsize(os.path.join(HERE, 'dca.npz')), 'bytes')


if __name__ == '__main__':
    main()
