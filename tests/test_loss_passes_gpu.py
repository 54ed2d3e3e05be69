"""GPU: rgda_upsample_ce and rgda_upsample_loss (OHEM, focal, GHM, UPS, UVEM) on every case of tests/loss_cases.py, per
element against the float64 reference there.  Loss (relative), every gradient element and GHM's state at a momentum above
0 are bounded by tests/golden/loss_tolerances.json, which tests/golden/derive_loss_tolerances.py derives on the CPU from
the fp32 restatement's own deviation from the reference (never from a kernel's output).  Integer results are exact: the
OHEM keep mask where the gradient is per pixel, GHM's histogram at momentum 0, the gradients that are exactly zero (every
label ignored, nothing through the gate, low-res pixels no output pixel reads).  Every case runs twice for identical bits
and once without gradients for the same loss bits.  tests/test_loss_cases_cpu.py checks, without a GPU, that each case
reaches the path it names and that the bounds rest on what they claim."""
import functools
import json
import os

import numpy as np
import pytest
import torch

import loss_cases as L

pytestmark = pytest.mark.gpu
TOL = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'loss_tolerances.json')))['cases']
NAMES = [c.name for c in L.CASES]


@pytest.fixture(scope='module')
def ops():
    from regda_amd import ops
    return ops


def cu(t):
    return None if t is None else t.contiguous().cuda()


@functools.lru_cache(maxsize=None)
def reference(name):
    return L.ref64(L.inputs(name))


@functools.lru_cache(maxsize=None)
def device_inputs(name):
    x = L.inputs(name)
    return {k: cu(x[k]) for k in ('p1', 'p2', 'lab', 'soft', 'cw')}


def run(ops, name, want_grad=True):
    """-> (loss, g1, g2, acc_sum) through ops.upsample_ce / ops.upsample_loss"""
    x, d = L.inputs(name), device_inputs(name)
    acc = cu(x['acc0'].clone()) if x['kind'] == 'ghm' else None
    p2 = d['p1'] if x['heads'] == 1 else d['p2']
    if x['kind'] == 'ce':
        out = ops.upsample_ce(d['p1'], p2, d['lab'], ignore_label=x['ignore'], class_weight=d['cw'], want_grad=want_grad)
    else:
        out = ops.upsample_loss(x['kind'], d['p1'], p2, d['lab'], soft=d['soft'], class_weight=d['cw'], acc_sum=acc,
                                m=x['m'], t=x['t'], gamma=x['gamma'], thresh=x['thresh'], momentum=x['momentum'],
                                ignore_label=x['ignore'], want_grad=want_grad, heads=x['heads'])
    return out + (acc,)


def same_bits(a, b):
    if a is None or b is None:
        return a is b
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


def check_outputs(name, out):
    """loss, gradients and GHM's state of one call against the float64 reference, error and bound printed first"""
    x, r, t = L.inputs(name), reference(name), TOL[name]['bound']
    loss, g1, g2, acc = out
    got = float(loss.item())
    fails = []
    if np.isnan(r['loss']):
        assert np.isnan(got), (name, got)
    elif r['loss'] == 0:
        assert got == 0, (name, got)
    else:
        err = abs(got - r['loss']) / abs(r['loss'])
        print('LOSSCASE %s %s loss err %.3e bound %.3e' % (name, x['kind'], err, t['loss']))
        if not err <= t['loss']:
            fails.append('loss: %.3e > %.3e' % (err, t['loss']))
    if x['want_grad']:
        gs = [g1.cpu().double(), g2.cpu().double()]
        assert all(bool(torch.isfinite(g).all()) for g in gs), name
        if x['heads'] == 1:
            gs = [gs[0] + gs[1]]
        for k, (g, ref) in enumerate(zip(gs, r['g'])):
            key = 'g%d' % (k + 1)
            d = (g - ref).abs()
            print('LOSSCASE %s %s %s err %.3e bound %.3e' % (name, x['kind'], key, float(d.max()), t[key]))
            n = int((~(d <= t[key])).sum())
            if n:
                fails.append('%s: %d of %d off, max %.3e > %.3e' % (key, n, d.numel(), float(d.max()), t[key]))
    if x['kind'] == 'ghm':
        if x['momentum'] > 0:
            d = (acc.cpu().double() - r['acc']).abs()
            print('LOSSCASE %s ghm acc err %.3e bound %.3e' % (name, float(d.max()), t['acc']))
            if not bool((d <= t['acc']).all()):
                fails.append('acc: %.3e > %.3e' % (float(d.max()), t['acc']))
        else:       # the integer histogram of the last head, exactly
            assert torch.equal(acc.cpu().double(), r['hist'].double()), name
    assert not fails, (name, fails)


def check_exact(name, out):
    x, r = L.inputs(name), reference(name)
    geo = x['geo']
    _, g1, g2, _ = out
    if not x['want_grad']:
        assert g1 is None and g2 is None
        return
    gs = [g1.cpu(), g2.cpu()]
    # low-res pixels no output pixel reads: exactly zero
    cy, cx = torch.from_numpy(L.covered(geo.h, geo.H)), torch.from_numpy(L.covered(geo.w, geo.W))
    for g in gs:
        assert not g[:, :, ~cy, :].any() and not g[:, :, :, ~cx].any(), name
    if x['kind'] == 'ohem' and (geo.h, geo.w) == (geo.H, geo.W):
        # the keep mask, read off the gradient: a kept valid pixel has a non-zero gradient (p_c > 0 in some class), a
        # pixel that is not kept, or ignored, exactly zero in every class
        valid = (x['lab'] != x['ignore']).reshape(-1)
        for hd, g in enumerate(gs):
            seen = (g != 0).any(1).reshape(-1)
            want = r['keep'][hd] & valid
            assert torch.equal(seen, want), (name, hd, int((seen != want).sum()))
    if name == 'far-ohem-tie_p3':       # rows 0 and 1 of the three tie rows are kept, row 2 is not
        for g in gs:
            assert g[0, :, 0, 0].all() and g[0, :, 1, 0].all() and not g[0, :, 2, 0].any()


@pytest.mark.parametrize('name', NAMES)
def test_case(ops, name):
    x = L.inputs(name)
    out = run(ops, name, x['want_grad'])
    check_outputs(name, out)
    check_exact(name, out)
    again = run(ops, name, x['want_grad'])
    for a, b in zip(out, again):
        assert same_bits(a, b), name
    if x['want_grad']:                  # without gradients: the same loss bits, the same state
        lean = run(ops, name, False)
        assert same_bits(out[0], lean[0]) and same_bits(out[3], lean[3]) and lean[1] is None and lean[2] is None, name


@pytest.mark.parametrize('kind', L.KINDS)
def test_rows_above_the_lds_limit_are_refused_with_gradients(ops, kind):
    """C = 16, w = 64, W = 1024 needs 155 648 B with gradients: refused (ValueError), and nothing is written."""
    name = 'refuse_c16-%s' % kind
    x, d = L.inputs(name), device_inputs(name)
    assert L.row_route(16, 64, 1024, True) == 'refuse'
    g1, g2 = torch.full_like(d['p1'], 7.0), torch.full_like(d['p2'], 7.0)
    with pytest.raises(ValueError):
        if kind == 'ce':
            ops.upsample_ce(d['p1'], d['p2'], d['lab'], g1=g1, g2=g2)
        else:
            ops.upsample_loss(kind, d['p1'], d['p2'], d['lab'], soft=d['soft'], acc_sum=cu(x['acc0']) if kind == 'ghm' else None,
                              thresh=x['thresh'], momentum=x['momentum'], g1=g1, g2=g2)
    torch.cuda.synchronize()
    assert bool((g1 == 7).all()) and bool((g2 == 7).all())


def _raw_ohem(ops, name, ws):
    """rgda_upsample_loss (OHEM) with a workspace of the test's own -> (loss, g1, g2)"""
    from regda_amd._lib import lib
    x, d = L.inputs(name), device_inputs(name)
    geo = x['geo']
    loss = torch.empty(1, device='cuda')
    g1, g2 = torch.empty_like(d['p1']), torch.empty_like(d['p2'])
    lib().call('rgda_upsample_loss', ops.LOSS_KINDS['ohem'], 2, d['p1'].data_ptr(), d['p2'].data_ptr(), d['lab'].data_ptr(), 0,
               ops._p(d['cw']), 0, 0.2, 0.7, 4.0, float(x['thresh']), 0.0, loss.data_ptr(), g1.data_ptr(), g2.data_ptr(),
               geo.b, geo.C, geo.h, geo.w, geo.H, geo.W, x['ignore'], ws.data_ptr(), ws.numel(), ops._stream())
    return loss, g1, g2


def test_a_dirty_workspace_changes_nothing(ops):
    """One workspace, pre-filled with 0xFF, through top-k, threshold, top-k in a row: each result has the bits of the
    same call on a fresh zeroed workspace (the header is zeroed only up to `cut`; the rest is written before it is read)."""
    from regda_amd._lib import lib
    seq = ['id64-ohem-tie_cut', 'id64-ohem-thresh', 'id64-ohem-tie_p4']
    geo = L.GEOS['id64']
    nbytes = lib().size('rgda_upsample_loss_workspace', ops.LOSS_KINDS['ohem'], geo.b, geo.C, geo.h, geo.w, geo.H, geo.W)
    dirty = torch.full((nbytes,), 0xFF, dtype=torch.uint8, device='cuda')
    for name in seq:
        got = _raw_ohem(ops, name, dirty)
        want = _raw_ohem(ops, name, torch.zeros(nbytes, dtype=torch.uint8, device='cuda'))
        for a, b in zip(got, want):
            assert same_bits(a, b), name
        check_outputs(name, got + (None,))
        check_exact(name, got + (None,))
