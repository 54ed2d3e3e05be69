"""CPU: the batch-hard triplet loss restated (tests/triplet_ref.py) against the reference's own TripletLoss
(tests/golden/triplet.npz) and against float64 autograd of the definition; the emulated arithmetic contract of
rgda_triplet_loss against its derived tolerances; the exports, the workspace formula and the argument validation of
rgda_triplet_loss (no GPU needed: every check comes before a launch); AlignStep's triplet_weight."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

from triplet_ref import (CASES, GOLDEN_NAMES, MIXED, case_inputs, golden_cases, mining_deviation, triplet_differentiable,
                         triplet_emulated, triplet_restated, variant_cases)

HERE = os.path.dirname(os.path.abspath(__file__))


def _relnorm(got, ref):
    n = np.linalg.norm(ref)
    d = np.linalg.norm(np.asarray(got, np.float64) - ref)
    return float(d / n) if n else float(d)


def test_restated_triplet_matches_the_reference_goldens(gold):
    """The reference ran in fp32 on the expanded form |x_i|^2 + |x_j|^2 - 2 x_i.x_j: its own noise is measured here, as
    the deviation of an fp32 run of the definition from float64 on the same inputs, with the project's margin of 3 and
    a floor of one fp32 rounding of the expanded form, (|x_i|^2 + |x_j|^2) 2^-24 / (2 d^2) relative to a distance (about
    2^-23 on these inputs, whose distances are of the size of the norms), carried to the loss by d / L."""
    cases = list(golden_cases(gold('triplet.npz')))
    assert [c['name'] for c in cases] == GOLDEN_NAMES
    for c in cases:
        x, lab = case_inputs(c['name'])
        assert torch.equal(x, c['x']) and torch.equal(lab, c['labels'])          # the goldens hold the shared inputs
        assert int(torch.bincount(lab).min()) >= 2
        r = triplet_restated(c['x'], c['labels'], c['margin'])
        f = triplet_restated(c['x'], c['labels'], c['margin'], dtype=np.float32)
        if r['loss'] == 0.0:
            assert c['loss'] == 0.0 and float(c['grad'].abs().max()) == 0.0 and r['active'] == 0
            continue
        dmean = float(r['d_ap'][r['p'] >= 0].mean())
        floor = 2.0 ** -23 * dmean / r['loss']
        noise_l = max(abs(f['loss'] - r['loss']) / r['loss'], floor)
        noise_g = max(_relnorm(f['grad'], r['grad']), 2.0 ** -23)
        lrel = abs(c['loss'] - r['loss']) / r['loss']
        grel = _relnorm(c['grad'].numpy(), r['grad'])
        print(c['name'], 'loss', c['loss'], r['loss'], 'rel', lrel, 'bound', 3 * noise_l, 'grad rel', grel, 'bound', 3 * noise_g)
        assert lrel <= 3 * noise_l, (c['name'], lrel, noise_l)
        assert grel <= 3 * noise_g, (c['name'], grel, noise_g)


@pytest.mark.parametrize('name,ignore', [('n96_k32', None), ('n300_k64', None), ('n300_k64_ignore', -1),
                                         ('n300_k64_dup', None), ('n300_k64_single', None), ('one_class', None),
                                         ('one_class_after_ignore', 5)])
def test_closed_form_gradient_equals_float64_autograd_of_the_definition(name, ignore):
    if name.startswith('one_class'):
        x, lab = case_inputs('n96_k32')
        lab = torch.full_like(lab, 2)
        if ignore is not None:
            lab[::3] = ignore
    elif name in CASES:
        x, lab = case_inputs(name)
    else:
        x, lab, ignore = variant_cases()[name]
    r = triplet_restated(x, lab, 0.3, ignore)
    xt = x.double().requires_grad_(True)
    loss = triplet_differentiable(xt, lab, 0.3, ignore)
    loss.backward()
    if name.startswith('one_class'):
        assert r['loss'] == 0.0 and loss.item() == 0.0 and (r['m'], r['active']) == (0, 0)
        assert not r['grad'].any() and not xt.grad.any()
        return
    assert r['loss'] == pytest.approx(loss.item(), rel=1e-12)
    ref = xt.grad.numpy()
    assert np.abs(r['grad'] - ref).max() <= 1e-12 * np.abs(ref).max(), name
    if ignore is not None:
        ig = (lab == ignore).numpy()
        assert ig.any() and not r['grad'][ig].any() and r['m'] == int((~ig).sum())
    if name == 'n300_k64_dup':          # a duplicate of another class: d_an is the clamp and carries no gradient
        assert (r['d_an'] == 1e-6).sum() >= 10 and r['p'][150] == r['p'][0]
    if name == 'n300_k64_single':
        assert r['p'][17] == 17 and r['d_ap'][17] == 1e-6 and r['hinge'][17] == 0.0


def test_emulated_contract_stays_within_the_derived_tolerances():
    """triplet_tolerances.json is what derive_triplet_tolerances.py observes: the committed file is current.  (n8192_k64,
    the largest GPU shape, is recomputed by the GPU test that uses it.)"""
    tol = json.load(open(os.path.join(HERE, 'golden', 'triplet_tolerances.json')))
    assert tol['margin'] == 3.0
    cases = {name: case_inputs(name) + (None,) for name in CASES if name != 'n8192_k64'}
    cases.update(variant_cases())
    assert set(tol['bounds']) == set(tol['observed']) == set(cases) | {'n8192_k64'}
    for name, (x, lab, ig) in cases.items():
        r = triplet_restated(x, lab, ignore_label=ig)
        e = triplet_emulated(x, lab, ignore_label=ig)
        obs = tol['observed'][name]
        lrel = abs(e['loss'] - r['loss']) / (abs(r['loss']) if r['loss'] else 1.0)
        assert lrel == pytest.approx(obs['loss_rel'], rel=1e-3, abs=1e-9), name
        assert _relnorm(e['grad'].double().numpy(), r['grad']) == pytest.approx(obs['grad_rel'], rel=1e-3, abs=1e-12), name
        assert mining_deviation(x, e['p'], e['n'], r) == pytest.approx(obs['mining_rel'], rel=1e-3, abs=1e-12), name
        assert lrel <= tol['bounds'][name]['loss_rel'] and obs['index_share'] <= 0.05
    for name, obs in tol['observed'].items():
        for m in ('loss_rel', 'grad_rel'):
            assert tol['bounds'][name][m] == pytest.approx(3.0 * obs[m])
    assert tol['mining_bound'] == pytest.approx(3.0 * max(o['mining_rel'] for o in tol['observed'].values()))
    assert tol['mining_bound'] <= 5e-3


def test_share_of_positive_hinges_per_case():
    """a case meant to mix positive and zero hinges has a float64 share of positive hinges in [0.2, 0.8]; one case has
    all of them positive and one none"""
    share = {}
    for name in CASES:
        if name == 'n8192_k64':
            continue
        r = triplet_restated(*case_inputs(name))
        share[name] = r['active'] / r['m']
    print(share)
    for name in MIXED:
        assert 0.2 <= share[name] <= 0.8, (name, share[name])
    assert share['n96_k32'] == 1.0 and share['n130_k96_far'] == 0.0


def test_library_exports_the_triplet_entry_points():
    from regda_amd import _lib, ops
    from regda_amd.gast import TripletLoss
    from regda_amd.gast.triple import TripletLoss as T2
    L = _lib.lib()
    for name in ('rgda_triplet_loss', 'rgda_triplet_loss_workspace'):
        assert name in L.protos and name not in L.missing
        assert L.raw(name) is not None
    assert L.raw('rgda_plan_fn_id')(b'rgda_triplet_loss') >= 0          # replayable through the plan dispatch table
    assert len(L.protos['rgda_triplet_loss'][1]) == 18
    assert len(L.protos['rgda_triplet_loss_workspace'][1]) == 2
    assert L.raw('rgda_abi_version')() == 10
    assert callable(ops.triplet_loss) and TripletLoss is T2
    m = TripletLoss()
    assert (m.margin, m.ignore_label) == (0.3, None)
    assert TripletLoss(0.5, ignore_label=-1).ignore_label == -1
    with pytest.raises(ValueError):
        TripletLoss(margin=-0.1)


def _a(x):
    return (x + 255) // 256 * 256


def workspace_formula(n, k):
    """the formula documented at rgda_triplet_loss_workspace (include/rgda_hip.h)"""
    NP = (n + 127) // 128 * 128
    T = NP // 128
    return 256 + 9 * _a(4 * NP) + _a(16 * T * NP) + _a(2 * NP * k) + _a(4 * NP * k)


def test_triplet_workspace_matches_its_documented_formula():
    from regda_amd import _lib
    L = _lib.lib()
    for n, k in ((8192, 2048), (96, 32), (300, 64), (2, 32), (16384, 2048), (16384, 32), (129, 96)):
        assert L.size('rgda_triplet_loss_workspace', n, k) == workspace_formula(n, k), (n, k)
    assert workspace_formula(16384, 2048) < 1 << 28           # the whole workspace at the limit: under 256 MB
    for n, k in ((1, 64), (0, 64), (16385, 64), (64, 48), (64, 0), (64, 16), (-5, 64)):
        assert L.size('rgda_triplet_loss_workspace', n, k) == 0, (n, k)


def test_triplet_entry_point_rejects_bad_arguments_before_any_launch():
    from regda_amd import _lib
    L = _lib.lib()
    fake = ctypes.c_void_p(256)       # never dereferenced: the arguments are rejected first

    def call(feat=fake, b=2, hw=16, labels=fake, k=64, margin=0.3, loss=fake, df=None, ldd=0, ws=fake, ws_bytes=1 << 40,
             ldc=None, ldb=None):
        L.call('rgda_triplet_loss', feat, b, hw, hw if ldc is None else ldc, k * hw if ldb is None else ldb, labels, k,
               margin, 0, 0, loss, df, ldd, 0, 1.0, ws, ws_bytes, None)
    for kw in (dict(feat=None), dict(labels=None), dict(loss=None), dict(ws=None), dict(ws=ctypes.c_void_p(272)),
               dict(k=48), dict(k=0), dict(k=16), dict(b=1, hw=1), dict(b=0), dict(hw=0),           # k % 32, n < 2
               dict(b=1, hw=16385), dict(b=128, hw=129),                                            # n > 16384
               dict(margin=-0.1), dict(margin=float('nan')),
               dict(ldc=8), dict(ldb=100),
               dict(df=fake, ldd=60), dict(df=fake, ldd=68), dict(df=ctypes.c_void_p(264), ldd=64)):
        with pytest.raises(ValueError):
            call(**kw)
    with pytest.raises(_lib.RgdaError):       # workspace too small
        call(ws_bytes=workspace_formula(32, 64) - 1)


def test_align_step_rejects_a_negative_triplet_weight():
    from regda_amd.align import AlignStep
    with pytest.raises(ValueError):
        AlignStep(None, None, triplet_weight=-1)
    with pytest.raises(ValueError):
        AlignStep(None, None, triplet_weight=-1e-3)
