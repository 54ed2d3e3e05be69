"""Derive the bounds of the TransNorm GPU tests: how far an fp32 evaluation of the reference (its own TransNorm1d /
TransNorm2d, imported behind the stubs of _refstubs.py, on the CPU) lies from the float64 restatement
(tests/transnorm_ref.py), on the golden inputs and on the production-shape inputs of the GPU test.  Runs where the
reference checkout exists only:
    python tests/golden/derive_transnorm_tolerances.py
Writes transnorm_tolerances.json: per case (every golden case by its name, and 'production') and per quantity the
observed relative-norm deviation and the bound = margin * deviation with margin 3, the margin of the project's other
derived tolerances.

Quantities: y, dx, dweight, dbias of the first training step; saved (mean_s, rstd_s, mean_t, rstd_t, alpha: the
reference does not expose them, so these are the restatement's formulae -- the reference's -- evaluated in fp32); running
(the four vectors after two training steps, as one vector); y_eval.

The edge shapes of the GPU test (transnorm_ref.EDGE_SHAPES, inputs from edge_inputs) get a bound each in the same way,
under 'edge_<n>_<C>_<s>_<dims>': one training step from fresh running vectors with its gradients, then an eval pass on
the updated vectors with its gradients (y_eval, dx_eval, dweight_eval, dbias_eval).  Their training-mode dx is measured
by transnorm_ref.dx_deviation (against its largest term): these shapes include halves of two values.

One evaluation is one draw of the roundings of its sums (dbias of a small case adds a few dozen values and can land
within a rounding of float64 by luck), and the kernel's order of the same sums is another draw.  None of the quantities
depends on the order of the positions inside a plane (or, for a 2-D input, of the samples inside a half) beyond a
permutation of the outputs, the fp32 sums do: every case is evaluated in the stored order and in ORDERS - 1 seeded
permutations, and the largest deviation is recorded (the convention of derive_saw_tolerances.py).

A floor: no fp32 output can be expected nearer to float64 than its own final rounding, 2^-24 relative.  Where three
times the observed deviation is smaller the bound is 2^-24; that happens in `one` alone, whose four output values make
a deviation a draw of four roundings (dbias was exact there, y_eval 1.2e-8), and the floors applied are listed under
"floored"."""
import json
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
from transnorm_ref import (EDGE_SHAPES, GOLDEN_CASES, dx_deviation, edge_inputs, edge_key, golden_case,  # noqa: E402
                           golden_steps, production_inputs, rel, transnorm_eval, transnorm_train)

MARGIN = 3.0
ORDERS = 8
PRODUCTION_ORDERS = 3
FLOOR = 2.0 ** -24
QUANTITIES = ('y', 'dx', 'dweight', 'dbias', 'saved', 'running', 'y_eval')


def reference_fp32(c):
    """the golden's recipe on the reference's module, float32"""
    x, x2, g = c['x'], c['x2'], c['g']
    C = x.shape[1]
    m = (TransNorm1d if x.dim() == 2 else TransNorm2d)(C, eps=c['eps'], momentum=c['momentum'])
    with torch.no_grad():
        m.weight.copy_(c['weight'])
        m.bias.copy_(c['bias'])
    m.train()
    xg = x.clone().requires_grad_(True)
    y = m(xg)
    y.backward(g)
    out = dict(y=y.detach(), dx=xg.grad, dweight=m.weight.grad, dbias=m.bias.grad)
    if x2 is not None:
        m(x2)
        m.eval()
        with torch.no_grad():
            out['y_eval'] = m(x)
        out['running'] = torch.cat([m.running_mean_source, m.running_var_source, m.running_mean_target, m.running_var_target])
    return out


def permuted(c, gen):
    """the same case with the positions of every plane (2-D: the samples of each half) in another order"""
    x = c['x']
    d = dict(c)
    if x.dim() == 2:
        half = x.shape[0] // 2
        perm = torch.cat([torch.randperm(half, generator=gen), half + torch.randperm(x.shape[0] - half, generator=gen)])
        for k in ('x', 'x2', 'g'):
            if c[k] is not None:
                d[k] = c[k][perm].contiguous()
    else:
        n, C, h, w = x.shape
        perm = torch.randperm(h * w, generator=gen)
        for k in ('x', 'x2', 'g'):
            if c[k] is not None:
                d[k] = c[k].reshape(n, C, h * w)[:, :, perm].reshape(n, C, h, w).contiguous()
    return d


def deviation_once(c):
    ref = reference_fp32(c)
    if c['x2'] is not None:
        s1, run, ev = golden_steps(c)
        f1, _, _ = golden_steps(c, torch.float32)
        exact = dict(s1, running=torch.cat(run), y_eval=ev['y'])
        ref['saved'] = f1['saved']
    else:           # production: the first step only
        exact = transnorm_train(c['x'].double(), c['weight'].double(), c['bias'].double(), None, c['eps'], c['momentum'],
                                c['g'].double())
        ref['saved'] = transnorm_train(c['x'], c['weight'], c['bias'], None, c['eps'], c['momentum'])['saved']
    return {q: rel(ref[q], exact[q]) for q in QUANTITIES if q in ref}


EDGE_QUANTITIES = ('y', 'dx', 'dweight', 'dbias', 'saved', 'running', 'y_eval', 'dx_eval', 'dweight_eval', 'dbias_eval')


def edge_deviation_once(c):
    """one training step with gradients from fresh running vectors, then eval with gradients on the updated vectors:
    the reference in fp32 against the restatement in float64"""
    x, g, w, b = c['x'], c['g'], c['weight'], c['bias']
    C = x.shape[1]
    m = (TransNorm1d if x.dim() == 2 else TransNorm2d)(C)
    with torch.no_grad():
        m.weight.copy_(w)
        m.bias.copy_(b)
    fresh = [torch.zeros(C, dtype=torch.float64), torch.ones(C, dtype=torch.float64)] * 2
    exact = transnorm_train(x.double(), w.double(), b.double(), fresh, 1e-5, 0.1, g.double())
    exact_eval = transnorm_eval(x.double(), w.double(), b.double(), exact['running'], 1e-5, g.double())
    m.train()
    xg = x.clone().requires_grad_(True)
    y = m(xg)
    y.backward(g)
    running = torch.cat([m.running_mean_source, m.running_var_source, m.running_mean_target, m.running_var_target])
    d = dict(y=rel(y.detach(), exact['y']), dx=dx_deviation(xg.grad, exact, w, g), dweight=rel(m.weight.grad, exact['dweight']),
             dbias=rel(m.bias.grad, exact['dbias']), saved=rel(transnorm_train(x, w, b)['saved'], exact['saved']),
             running=rel(running, torch.cat(exact['running'])))
    m.eval()
    m.zero_grad()
    xe = x.clone().requires_grad_(True)
    ye = m(xe)
    ye.backward(g)
    d.update(y_eval=rel(ye.detach(), exact_eval['y']), dx_eval=rel(xe.grad, exact_eval['dx']),
             dweight_eval=rel(m.weight.grad, exact_eval['dweight']), dbias_eval=rel(m.bias.grad, exact_eval['dbias']))
    return d


def edge_deviation(shape, orders):
    x, w, b, g = edge_inputs(*shape)
    c = dict(x=x, x2=None, g=g, weight=w, bias=b)
    gen = torch.Generator().manual_seed(7)
    worst = edge_deviation_once(c)
    for _ in range(orders - 1):
        d = edge_deviation_once(permuted(c, gen))
        worst = {q: max(worst[q], d[q]) for q in worst}
    return worst


def deviation(c, orders):
    gen = torch.Generator().manual_seed(7)
    worst = deviation_once(c)
    for _ in range(orders - 1):
        d = deviation_once(permuted(c, gen))
        worst = {q: max(worst[q], d[q]) for q in worst}
    return worst


def main():
    g = np.load(os.path.join(HERE, 'transnorm.npz'), allow_pickle=False)
    cases = {name: deviation(golden_case(g, name), ORDERS) for name in GOLDEN_CASES}
    x, weight, bias, gy = production_inputs()
    cases['production'] = deviation(dict(x=x, x2=None, g=gy, weight=weight, bias=bias, eps=1e-5, momentum=0.1),
                                    PRODUCTION_ORDERS)
    for shape in EDGE_SHAPES:
        cases[edge_key(*shape)] = edge_deviation(shape, ORDERS)
    bounds = {name: {q: max(MARGIN * v, FLOOR) for q, v in d.items()} for name, d in cases.items()}
    floored = sorted(f'{name}.{q}' for name, d in cases.items() for q, v in d.items() if MARGIN * v < FLOOR)
    out = dict(margin=MARGIN, floor=FLOOR, floored=floored, orders=ORDERS, production_orders=PRODUCTION_ORDERS,
               observed=cases, bounds=bounds)
    with open(os.path.join(HERE, 'transnorm_tolerances.json'), 'w') as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write('\n')
    print(json.dumps(out, indent=1, sort_keys=True))


if __name__ == '__main__':
    main()
