"""Mint saw.npz from the reference's OWN SAW (imported behind the stubs of _refstubs.py, on the CPU).

Run where the reference checkout exists only:
    python tests/golden/make_saw_goldens.py
Data only: inputs, the reference's loss and its autograd gradient with respect to `x`.

Cases (features on a grid of 1/32, stored as int8, times a float32 scale; classifier weights float32 with pairwise
distinct |w| per class -- the reference's torch.sort leaves the order of ties unspecified; no pair covariance and no
group sum inside the near-tie bands of tests/saw_ref.py, all asserted here):
    k64_c6      (2, 64, 8, 12), 6 classes, relax_denom 2.0: scaled so that some groups are active and some clamped
    k70_c8      (2, 70, 8, 12), 8 classes, relax_denom 2.0: k % C != 0, the six lowest ranks are unused
    k48_c16     (1, 48, 4, 8), 16 classes, relax_denom 2.0
    k32_c2      (2, 32, 5, 7), 2 classes, relax_denom 2.0: margin 1 // 2.0 = 0; hw = 35
    k32_c4_sel  (2, 32, 5, 7), selected_classes [1, 2, 4, 6] of a 7-class classifier, relax_denom 3.0
    hw2         (2, 64, 1, 2), 6 classes, relax_denom 0: hw = 2"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import _refstubs  # noqa: E402

_refstubs.install()

from regda.gast.SAW import SAW  # noqa: E402
from saw_ref import group_band, pair_band, saw_margin, saw_restated  # noqa: E402

CASES = (('k64_c6', (2, 64, 8, 12), 6, list(range(6)), 2.0),
         ('k70_c8', (2, 70, 8, 12), 8, list(range(8)), 2.0),
         ('k48_c16', (1, 48, 4, 8), 16, list(range(16)), 2.0),
         ('k32_c2', (2, 32, 5, 7), 2, [0, 1], 2.0),
         ('k32_c4_sel', (2, 32, 5, 7), 7, [1, 2, 4, 6], 3.0),
         ('hw2', (2, 64, 1, 2), 6, list(range(6)), 0))


class Classifier(torch.nn.Module):
    """a 1 x 1 convolution, the shape of classifier the reference squeezes to (n_cls, k)"""
    def __init__(self, W):
        super().__init__()
        self.conv = torch.nn.Conv2d(W.shape[1], W.shape[0], 1)
        with torch.no_grad():
            self.conv.weight.copy_(W.view(*W.shape, 1, 1))


def main():
    rng = np.random.default_rng(20220601)
    out, names = {}, []
    for name, shape, n_cls, sel, relax in CASES:
        b, k, h, w = shape
        hw, C = h * w, len(sel)
        W = torch.from_numpy(rng.standard_normal((n_cls, k)).astype(np.float32))
        for c in range(n_cls):
            assert len(set(W[c].abs().tolist())) == k, (name, c)
        margin = saw_margin(C, relax)
        for draw in range(100):      # on the 1/32 grid a covariance of few pixels can cancel exactly: draw again
            q = np.clip(np.round(rng.standard_normal(shape) * 32.0 * 0.8), -127, 127).astype(np.int8)
            x0 = torch.from_numpy(q.astype(np.float32) / 32.0)
            if (saw_restated(x0, W, sel, relax)['corr'].abs() >= pair_band(hw)).all():
                break
        scale = 1.0
        if margin > 0:          # s scales with the square of the features: put the margin between the two middle group sums
            s0 = saw_restated(x0, W, sel, relax)['s'].flatten().sort().values
            mid = (s0[s0.numel() // 2 - 1] * s0[s0.numel() // 2]).sqrt().item()
            scale = float(np.float32((margin / mid) ** 0.5))
        feats = (x0 * scale).requires_grad_(True)
        crit = SAW(Classifier(W), sel, relax_denom=relax)
        loss = crit(feats)
        loss.backward()
        r = saw_restated(feats.detach(), W, sel, relax)
        assert r['active'].any(), name
        if name == 'k64_c6':
            assert (~r['active']).any(), name
        assert (r['corr'].abs() >= pair_band(hw)).all(), name
        assert ((r['s'] - margin).abs() >= group_band(hw, C)).all(), name
        print(name, 'loss', loss.item(), 'restated', r['loss'].item(), 'active', int(r['active'].sum()), 'of',
              r['active'].numel(), 'scale', scale)
        names.append(name)
        out.update({name + '_q': q, name + '_scale': np.float32(scale), name + '_W': W.numpy(),
                    name + '_sel': np.array(sel, np.int32), name + '_relax': np.float32(relax),
                    name + '_loss': loss.detach().numpy(), name + '_grad': feats.grad.numpy()})
    out['names'] = np.array(names)
    np.savez_compressed(os.path.join(HERE, 'saw.npz'), **out)
    print('wrote saw.npz', {k: getattr(v, 'shape', None) for k, v in out.items()})


if __name__ == '__main__':
    main()
