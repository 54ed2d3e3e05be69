"""Mint transnorm.npz from the reference's OWN TransNorm1d / TransNorm2d (imported behind the stubs of _refstubs.py, on the
CPU, in float32).

Run where the reference checkout exists only:
    python tests/golden/make_transnorm_goldens.py
Data only.  Per case <name>_: x, x2 (the input of a second training step), weight, bias, g (the upstream gradient), eps,
momentum and, from the reference: y, dx, dweight, dbias of the first training step; the four running vectors after the
two training steps (rm_s, rv_s, rm_t, rv_t); y_eval, the eval output on x after them.

Cases:
    plain  (4, 6, 5, 7)  nothing special
    shift  (4, 6, 5, 7)  per-channel mean about 30, standard deviation 0.5: a sum of squares loses the variance here
    odd    (5, 3, 3, 3)  halves of 2 and 3 samples
    rows   (6, 70)       a 2-D input (TransNorm1d)
    one    (2, 1, 1, 2)  a single channel (alpha is exactly 1) and two values per half.  With two values dx is
                         (1 - var / (var + eps)) times a difference: the two values of a half lie 0.01 apart, so that
                         var is of the order of eps and dx is not the rounding residue of a cancellation.
    pretrained           a BatchNorm2d(5) state dict (bn_*) loaded into the reference's TransNorm2d(5), and the
                         reference's buffers and parameters afterwards (tn_*); keys: the reference's state_dict() keys."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import _refstubs  # noqa: E402

_refstubs.install()

from regda.trans_norm import TransNorm1d, TransNorm2d  # noqa: E402
from transnorm_ref import RUNNING, golden_case, golden_steps, rel  # noqa: E402

CASES = (('plain', (4, 6, 5, 7)), ('shift', (4, 6, 5, 7)), ('odd', (5, 3, 3, 3)), ('rows', (6, 70)), ('one', (2, 1, 1, 2)))
EPS, MOMENTUM = 1e-5, 0.1


def draw(name, shape, gen):
    C = shape[1]
    cv = lambda v: v.view(1, C, *([1] * (len(shape) - 2)))      # noqa: E731
    x = torch.randn(shape, generator=gen)
    if name == 'shift':
        x = x * 0.5 + cv(30.0 + torch.randn(C, generator=gen))
    elif name == 'one':
        x = torch.tensor([0.3, 0.31, -0.2, -0.19]).view(shape) + 1e-3 * x
    else:                                                        # the halves differ in mean and spread
        half = shape[0] // 2
        x[half:] = x[half:] * cv(0.5 + torch.rand(C, generator=gen)) + cv(torch.randn(C, generator=gen))
    return x


def main():
    gen = torch.Generator().manual_seed(20191208)
    out = {}
    for name, shape in CASES:
        C = shape[1]
        x = draw(name, shape, gen)
        x2 = draw(name, shape, gen)
        g = torch.randn(shape, generator=gen)
        m = (TransNorm1d if len(shape) == 2 else TransNorm2d)(C, eps=EPS, momentum=MOMENTUM)
        with torch.no_grad():
            m.weight.copy_(torch.rand(C, generator=gen) + 0.5)
            m.bias.copy_(torch.randn(C, generator=gen))
        m.train()
        xg = x.clone().requires_grad_(True)
        y = m(xg)
        y.backward(g)
        m(x2)
        m.eval()
        with torch.no_grad():
            y_eval = m(x)
        assert int(m.num_batches_tracked) == 0
        case = dict(x=x, x2=x2, g=g, weight=m.weight.detach(), bias=m.bias.detach(), eps=torch.tensor(EPS),
                    momentum=torch.tensor(MOMENTUM), y=y.detach(), dx=xg.grad, dweight=m.weight.grad, dbias=m.bias.grad,
                    rm_s=m.running_mean_source, rv_s=m.running_var_source, rm_t=m.running_mean_target,
                    rv_t=m.running_var_target, y_eval=y_eval)
        out.update({f'{name}_{k}': v.detach().numpy().copy() for k, v in case.items()})
    # a BatchNorm checkpoint into the reference
    bn = torch.nn.BatchNorm2d(5)
    with torch.no_grad():
        bn.weight.copy_(torch.rand(5, generator=gen) + 0.5)
        bn.bias.copy_(torch.randn(5, generator=gen))
        bn.running_mean.copy_(torch.randn(5, generator=gen))
        bn.running_var.copy_(torch.rand(5, generator=gen) + 0.5)
        bn.num_batches_tracked.fill_(17)
    tn = TransNorm2d(5)
    tn.load_state_dict(bn.state_dict())
    out.update({'pretrained_bn_' + k: v.numpy().copy() for k, v in bn.state_dict().items()})
    out.update({'pretrained_tn_' + k: v.numpy().copy() for k, v in tn.state_dict().items()})
    out['keys'] = np.array(list(tn.state_dict().keys()))
    assert [k for k in out['keys'] if 'running' in k] == sorted(RUNNING), 'the buffer order of the restatement'
    path = os.path.join(HERE, 'transnorm.npz')
    np.savez_compressed(path, **out)
    # the float64 restatement against what was just minted (the CPU test asserts it; printed here for the record)
    gz = np.load(path, allow_pickle=False)
    for name, _ in CASES:
        c = golden_case(gz, name)
        s1, run, ev = golden_steps(c)
        print(name, {k: '%.2e' % rel(c[k], s1[k]) for k in ('y', 'dx', 'dweight', 'dbias')},
              'running', ['%.2e' % rel(c[k], r) for k, r in zip(('rm_s', 'rv_s', 'rm_t', 'rv_t'), run)],
              'eval', '%.2e' % rel(c['y_eval'], ev['y']))
    print('wrote transnorm.npz', os.path.getsize(path), 'bytes; keys', list(out['keys']))


if __name__ == '__main__':
    main()
