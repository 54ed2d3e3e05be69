"""Mint mmd.npz from the reference's OWN MMDLoss (regda/gast/mmd.py needs torch only: no stubs), on the CPU in fp32.

Run where the reference checkout exists only:
    python tests/golden/make_mmd_goldens.py
Data only: inputs, the reference's loss and its autograd gradients with respect to both inputs.

Cases (ReLU-like rows on a grid of 1/32 stored as uint8; the target is scaled and shifted so the domains differ):
    n24_40_d64      24 + 40 rows, 64 channels, defaults: one partial tile, ns != nt, ns not a multiple of 32
    n130_126_d96    130 + 126 rows, 96 channels, defaults: the domain boundary and a tile edge inside a 128-row tile
    n192_192_d128   192 + 192 rows, 128 channels, fix_sigma near the case's automatic bandwidth
    n64_64_d64_k3   64 + 64 rows, 64 channels, kernel_mul 3, kernel_num 3
    n24_40_d64_lin  24 + 40 rows, 64 channels, kernel_type 'linear'"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import _refstubs  # noqa: E402  (only for the location of the reference checkout: nothing is stubbed)

sys.path.insert(0, _refstubs.REF)

from mmd_ref import bandwidth_closed, relu_like  # noqa: E402
from regda.gast.mmd import MMDLoss  # noqa: E402

CASES = (('n24_40_d64', 24, 40, 64, {}), ('n130_126_d96', 130, 126, 96, {}),
         ('n192_192_d128', 192, 192, 128, dict(fix_sigma='near')), ('n64_64_d64_k3', 64, 64, 64, dict(kernel_mul=3.0, kernel_num=3)),
         ('n24_40_d64_lin', 24, 40, 64, dict(kernel_type='linear')))


def main():
    gen = torch.Generator().manual_seed(20230331)
    out, names = {}, []
    for name, ns, nt, d, st in CASES:
        qs, a, _ = relu_like(gen, ns, d, 1.0, 0.0)
        qt, b, o = relu_like(gen, nt, d, 1.25, 0.25)
        xs = (qs.float() / 32.0 * a).requires_grad_(True)
        xt = (qt.float() / 32.0 * b + o).requires_grad_(True)
        st = dict(st)
        if st.get('fix_sigma') == 'near':
            auto = bandwidth_closed(torch.cat([xs, xt]).detach().double()).item()
            st['fix_sigma'] = float(round(auto * 0.9))
            print(name, 'automatic bandwidth', auto, 'fix_sigma', st['fix_sigma'])
        loss = MMDLoss(**st)(xs, xt)
        loss.backward()
        assert loss.item() >= 0.05, (name, loss.item())
        names.append(name)
        out.update({name + '_qs': qs.numpy(), name + '_qt': qt.numpy(), name + '_scales': np.array([a, b, o], np.float32),
                    name + '_loss': loss.detach().numpy(), name + '_gs': xs.grad.numpy(), name + '_gt': xt.grad.numpy()})
        for k in ('kernel_mul', 'kernel_num', 'fix_sigma'):
            if k in st:
                out[name + '_' + k] = np.float64(st[k])
        if st.get('kernel_type') == 'linear':
            out[name + '_linear'] = np.int32(1)
        print(name, 'loss', loss.item())
    out['names'] = np.array(names)
    np.savez_compressed(os.path.join(HERE, 'mmd.npz'), **out)
    print('wrote mmd.npz', os.path.getsize(os.path.join(HERE, 'mmd.npz')), 'bytes')


if __name__ == '__main__':
    main()
