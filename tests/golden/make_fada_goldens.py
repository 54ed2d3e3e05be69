"""Mint fada*.npz from the reference's OWN PixelDiscriminator (regda/models/Discriminator.py:60-78, imported behind the
stubs of _refstubs.py, on the CPU, in float32).

Run where the reference checkout exists only:
    python tests/golden/make_fada_goldens.py
Data only.  input_nc = ndf = 64 (about 55 k weights); num_classes 1, 6 and 7, one discriminator each; inputs (2, 64, 8, 8)
and (1, 64, 5, 7) (tests/fada_ref.py draws them: MODULE_CASES).  A case's gradients alone are 55 k floats per side, so the
fixture is split, every file below the largest adv_*.npz:
    fada.npz                keys (the reference's state_dict() keys in order), nc<n>_sd.<key>, <case>_x, <case>_x2 (the
                            logits the soft labels are made of), <case>_z = D(x)
    fada_<case>_s<side>.npz the class-level loss formed on z with torch ops in float32 (fada_ref.autograd_reference) and
                            torch autograd through the reference's module: loss, dx, g.<key>"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import _refstubs  # noqa: E402

_refstubs.install()

from regda.models.Discriminator import PixelDiscriminator  # noqa: E402
import fada_ref as R  # noqa: E402

LIMIT = 811067      # the largest adv_*.npz


def main():
    torch.manual_seed(20200823)
    base, parts = {}, {}
    models = {nc: PixelDiscriminator(R.MODULE_NC, R.MODULE_NDF, nc) for nc in (1, 6, 7)}
    for nc, m in models.items():
        assert tuple(m.state_dict().keys()) == R.PARAMS
        base.update({f'nc{nc}_sd.{k}': v.detach().numpy().copy() for k, v in m.state_dict().items()})
        base['keys'] = np.array(list(m.state_dict().keys()))
    for name in R.GOLDEN_CASES:
        c = R.module_case(name)
        m = models[c['nc']]
        base[name + '_x'], base[name + '_x2'] = c['x'].numpy().copy(), c['x2'].numpy().copy()
        for s in (0, 1):
            m.zero_grad()
            r = R.autograd_reference(m.state_dict(), c['x'], c['x2'], s, dtype=torch.float32, forward=m)
            r['graph_loss'].backward()
            base[name + '_z'] = r['z'].numpy().copy()
            part = dict(loss=r['loss'].numpy().copy(), dx=r['x'].grad.numpy().copy())
            part.update({f'g.{k}': p.grad.numpy().copy() for k, p in m.named_parameters()})
            parts[R.golden_part(name, s)] = part
    sizes = {}
    for fn, d in [('fada.npz', base)] + list(parts.items()):
        np.savez_compressed(os.path.join(HERE, fn), **d)
        sizes[fn] = os.path.getsize(os.path.join(HERE, fn))
        assert sizes[fn] <= LIMIT, (fn, sizes[fn])
    load = lambda fn: np.load(os.path.join(HERE, fn), allow_pickle=False)      # noqa: E731
    for name in R.GOLDEN_CASES:
        c = R.golden_case(load, name)
        for s in (0, 1):
            r = R.disc_loss_grads(R.params64(c['sd']), c['x'], c['x2'], s)
            print(name, s, 'z %.2e' % R.err(c['z'], r['z']), 'dx %.2e' % R.err(c['dx%d' % s], r['dx']),
                  {k: '%.1e' % R.err(c['g%d' % s][k], r['grads'][k]) for k in R.PARAMS})
    print('wrote', sizes, '; keys', list(base['keys']))


if __name__ == '__main__':
    main()
