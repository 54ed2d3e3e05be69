"""Mint triplet.npz from the reference's OWN TripletLoss (regda/gast/triple.py needs torch only: no stubs), on the CPU
in fp32.

Run where the reference checkout exists only:
    python tests/golden/make_triplet_goldens.py
Data only: inputs, labels, the reference's loss and its autograd gradient with respect to the inputs.

Cases (tests/triplet_ref.py::CASES, x = cw * centroid[label] + randn; every class has at least two members: for a class
of one the reference's expanded-form fp32 distance gives a self-distance of about 1e-2 instead of the clamp, which is
its noise and not a target):
    n96_k32        96 rows, 32 channels, 3 classes: one ragged tile, every hinge positive
    n300_k64       300 rows, 64 channels, 4 classes: positive and zero hinges mixed
    n130_k96_far   130 rows, 96 channels, 3 classes far apart: no positive hinge (loss 0, gradient 0)"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import _refstubs  # noqa: E402  (only for the location of the reference checkout: nothing is stubbed)

sys.path.insert(0, _refstubs.REF)

from triplet_ref import CASES, GOLDEN_NAMES, make_inputs  # noqa: E402
from regda.gast.triple import TripletLoss  # noqa: E402

MARGIN = 0.3


def main():
    out = {}
    for name in GOLDEN_NAMES:
        x, labels = make_inputs(*CASES[name])
        assert int(torch.bincount(labels).min()) >= 2, name
        xr = x.clone().requires_grad_(True)
        loss = TripletLoss(margin=MARGIN)(xr, labels)
        loss.backward()
        out.update({name + '_x': x.numpy(), name + '_labels': labels.numpy(), name + '_loss': loss.detach().numpy(),
                    name + '_grad': xr.grad.numpy(), name + '_margin': np.float64(MARGIN)})
        print(name, 'loss', loss.item(), 'rows with gradient', int((xr.grad.abs().sum(1) > 0).sum()))
    out['names'] = np.array(GOLDEN_NAMES)
    np.savez_compressed(os.path.join(HERE, 'triplet.npz'), **out)
    print('wrote triplet.npz', os.path.getsize(os.path.join(HERE, 'triplet.npz')), 'bytes')


if __name__ == '__main__':
    main()
