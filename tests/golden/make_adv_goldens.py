"""Mint adv.npz from the reference's OWN FCDiscriminator (regda/models/Discriminator.py, imported behind the stubs of
_refstubs.py, on the CPU, in float32).

Run where the reference checkout exists only:
    python tests/golden/make_adv_goldens.py
Data only.  ndf = 8 (about 45 k weights).  Cases: C = 6 and 7, b = 2, inputs 32 x 32 and 64 x 96; one discriminator per C.
No file may exceed 1 MiB and a case's gradients alone are 45 k floats per label, so the fixture is split:
    adv.npz                  keys (the reference's state_dict() keys in order), c<C>_sd.<key>, <case>_z = D(x)
    adv_<case>_t<label>.npz  under F.binary_cross_entropy_with_logits against the constant label: loss, dx, g.<key>
                             (every parameter gradient); the label-0 file also holds x (the probabilities fed in)"""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import _refstubs  # noqa: E402

_refstubs.install()

from regda.models.Discriminator import FCDiscriminator  # noqa: E402
import adv_ref as R  # noqa: E402

NDF = 8
CASES = {'c6_32x32': (6, 32, 32), 'c7_32x32': (7, 32, 32), 'c6_64x96': (6, 64, 96), 'c7_64x96': (7, 64, 96)}


def main():
    torch.manual_seed(20180618)
    base, parts = {}, {}
    models = {C: FCDiscriminator(C, ndf=NDF) for C in (6, 7)}
    for C, m in models.items():
        base.update({f'c{C}_sd.{k}': v.detach().numpy().copy() for k, v in m.state_dict().items()})
        base['keys'] = np.array(list(m.state_dict().keys()))
    for name, (C, H, W) in CASES.items():
        m = models[C]
        x = torch.softmax(torch.randn(2, C, H, W) * 2, 1)
        for t in (0, 1):
            m.zero_grad()
            xg = x.clone().requires_grad_(True)
            z = m(xg)
            loss = F.binary_cross_entropy_with_logits(z, torch.full_like(z, float(t)))
            loss.backward()
            base[f'{name}_z'] = z.detach().numpy().copy()
            part = dict(loss=loss.detach().numpy().copy(), dx=xg.grad.numpy().copy())
            part.update({f'g.{k}': p.grad.numpy().copy() for k, p in m.named_parameters()})
            if t == 0:
                part['x'] = x.numpy().copy()
            parts[R.golden_part(name, t)] = part
    sizes = {}
    for fn, d in [('adv.npz', base)] + list(parts.items()):
        np.savez_compressed(os.path.join(HERE, fn), **d)
        sizes[fn] = os.path.getsize(os.path.join(HERE, fn))
        assert sizes[fn] < (1 << 20), (fn, sizes[fn])
    load = lambda fn: np.load(os.path.join(HERE, fn), allow_pickle=False)      # noqa: E731
    for name in CASES:
        c = R.golden_case(load, name)
        for t in (0, 1):
            r = R.disc_loss_grads(R.params64(c['sd']), c['x'], t)
            print(name, t, 'z %.2e' % R.err(c['z'], r['z']), 'dx %.2e' % R.err(c['dx%d' % t], r['dx']),
                  {k: '%.1e' % R.err(c['g%d' % t][k], r['grads'][k]) for k in R.PARAMS})
    print('wrote', sizes, '; keys', list(base['keys']))


if __name__ == '__main__':
    main()
