"""CPU: the MMD loss restated from its formulas (tests/mmd_ref.py) against the reference's own MMDLoss
(tests/golden/mmd.npz) and against float64 autograd of the pairwise definition; the emulated arithmetic contract of
rgda_mmd_loss against its derived tolerances; the exports, the workspace formula and the argument validation of
rgda_mmd_loss (no GPU needed: every check comes before a launch); the steps' align_domain values."""
import ctypes
import json
import os

import pytest
import torch

from mmd_ref import (bandwidth_closed, bandwidth_pairwise, golden_cases, mmd_emulated, mmd_pairwise_autograd,
                     mmd_restated, production_inputs, rows_of)

HERE = os.path.dirname(os.path.abspath(__file__))
NAMES = ['n24_40_d64', 'n130_126_d96', 'n192_192_d128', 'n64_64_d64_k3', 'n24_40_d64_lin']


def _rel(got, ref):
    return ((got.double() - ref.double()).norm() / ref.double().norm()).item()


def test_restated_mmd_matches_the_reference_goldens(gold):
    """The reference ran in fp32: its own noise against float64 was measured at 4e-6 (loss, relative) and 3e-7
    (gradient, relative norm); the bounds are those with the project's margin of 3."""
    cases = list(golden_cases(gold('mmd.npz')))
    assert [c['name'] for c in cases] == NAMES
    shapes = [(c['xs'].shape[0], c['xt'].shape[0], c['xs'].shape[1]) for c in cases]
    assert shapes == [(24, 40, 64), (130, 126, 96), (192, 192, 128), (64, 64, 64), (24, 40, 64)]
    assert cases[2]['settings'].keys() == {'fix_sigma'} and cases[3]['settings'] == dict(kernel_mul=3.0, kernel_num=3)
    auto = bandwidth_closed(torch.cat([cases[2]['xs'], cases[2]['xt']]).double()).item()
    assert 0.8 * auto <= cases[2]['settings']['fix_sigma'] <= 1.25 * auto          # near the automatic bandwidth
    for c in cases:
        assert c['loss'] >= 0.05, c['name']                  # relative bounds mean something
        loss, gs, gt = mmd_restated(c['xs'], c['xt'], **c['settings'])
        lrel = abs(loss.item() - c['loss']) / c['loss']
        grel = _rel(torch.cat([gs, gt]), torch.cat([c['gs'], c['gt']]))
        print(c['name'], 'loss', loss.item(), c['loss'], 'rel', lrel, 'grad rel', grel)
        assert lrel <= 3 * 4e-6, (c['name'], lrel)
        assert grel <= 3 * 3e-7, (c['name'], grel)


def test_closed_form_gradient_equals_float64_autograd_of_the_pairwise_definition(gold):
    """settles the factor -4 and the sign of dL/dx_i = -4 (rho_i x_i - sum_j W_ij x_j)"""
    for c in golden_cases(gold('mmd.npz')):
        if c['settings'].get('kernel_type') == 'linear':
            continue
        st = c['settings']
        loss, gs, gt = mmd_restated(c['xs'], c['xt'], **st)
        al, ags, agt = mmd_pairwise_autograd(c['xs'], c['xt'], **st)
        assert loss.item() == pytest.approx(al.item(), rel=1e-12), c['name']
        ref = torch.cat([ags, agt])
        assert (torch.cat([gs, gt]) - ref).abs().max().item() <= 1e-12 * ref.abs().max().item(), c['name']


def test_linear_closed_form_equals_float64_autograd(gold):
    c = [c for c in golden_cases(gold('mmd.npz')) if c['settings'].get('kernel_type') == 'linear'][0]
    xs, xt = c['xs'].double().requires_grad_(True), c['xt'].double().requires_grad_(True)
    delta = xs.mean(0) - xt.mean(0)
    (delta @ delta / delta.shape[0]).backward()
    loss, gs, gt = mmd_restated(c['xs'], c['xt'], kernel_type='linear')
    assert loss.item() == pytest.approx((delta @ delta / delta.shape[0]).item(), rel=1e-13)
    assert (gs - xs.grad).abs().max().item() <= 1e-13 * xs.grad.abs().max().item()
    assert (gt - xt.grad).abs().max().item() <= 1e-13 * xt.grad.abs().max().item()


def test_closed_form_bandwidth_equals_the_pairwise_sum(gold):
    for c in golden_cases(gold('mmd.npz')):
        total = torch.cat([c['xs'], c['xt']]).double()
        assert bandwidth_closed(total).item() == pytest.approx(bandwidth_pairwise(total).item(), rel=1e-12)
        centred = total - total.mean(0)          # the shift the kernel applies leaves it unchanged
        assert bandwidth_closed(centred).item() == pytest.approx(bandwidth_pairwise(total).item(), rel=1e-12)


def test_emulated_contract_stays_within_the_derived_tolerances(gold):
    """mmd_tolerances.json is what derive_mmd_tolerances.py observes: the committed file is current"""
    tol = json.load(open(os.path.join(HERE, 'golden', 'mmd_tolerances.json')))
    assert tol['margin'] == 3.0
    for c in golden_cases(gold('mmd.npz')):
        rl, rgs, rgt = mmd_restated(c['xs'], c['xt'], **c['settings'])
        el, egs, egt = mmd_emulated(c['xs'], c['xt'], **c['settings'])
        obs = tol['observed'][c['name']]
        assert abs(float(el) - float(rl)) / float(rl) == pytest.approx(obs['loss_rel'], rel=1e-3, abs=1e-9)
        assert _rel(torch.cat([egs, egt]), torch.cat([rgs, rgt])) == pytest.approx(obs['grad_rel'], rel=1e-3)
    assert set(tol['bounds']) == set(tol['observed']) == set(NAMES + ['production'])
    for name, obs in tol['observed'].items():
        for m in ('loss_rel', 'grad_rel'):
            assert tol['bounds'][name][m] == pytest.approx(3.0 * obs[m])
    # the production entry bounds the largest GPU test: recomputed too (n = 4096, d = 2048: a few seconds)
    f, b = production_inputs()
    assert f.shape == (4, 2048, 32, 32) and b == 2
    xs, xt = rows_of(f[:b]), rows_of(f[b:])
    rl, rgs, rgt = mmd_restated(xs, xt)
    el, egs, egt = mmd_emulated(xs, xt)
    obs = tol['observed']['production']
    assert abs(float(el) - float(rl)) / float(rl) == pytest.approx(obs['loss_rel'], rel=1e-3, abs=1e-9)
    assert _rel(torch.cat([egs, egt]), torch.cat([rgs, rgt])) == pytest.approx(obs['grad_rel'], rel=1e-3)


def test_library_exports_the_mmd_entry_points():
    from regda_amd import _lib, ops
    from regda_amd.gast.mmd import MMDLoss
    L = _lib.lib()
    for name in ('rgda_mmd_loss', 'rgda_mmd_loss_workspace'):
        assert name in L.protos and name not in L.missing
        assert L.raw(name) is not None
    assert L.raw('rgda_plan_fn_id')(b'rgda_mmd_loss') >= 0          # replayable through the plan dispatch table
    assert len(L.protos['rgda_mmd_loss'][1]) == 25
    assert callable(ops.mmd_loss)
    m = MMDLoss()
    assert (m.kernel_type, m.kernel_mul, m.kernel_num, m.fix_sigma) == ('rbf', 2.0, 5, None)
    assert MMDLoss(kernel_type='linear', foo=1).ext_params == dict(foo=1)
    with pytest.raises(ValueError):
        MMDLoss(kernel_type='poly')


def _a(x):
    return (x + 255) // 256 * 256


def workspace_formula(ns, nt, d):
    """the formula documented at rgda_mmd_loss_workspace (include/rgda_hip.h)"""
    NP = (ns + nt + 127) // 128 * 128
    T = NP // 128
    U = T * (T + 1) // 2
    return _a(12 * d) + 2 * _a(2 * NP * d) + 2 * _a(4 * NP) + _a(4 * d) + 256 + _a(4 * T * NP) + _a(4 * U) + _a(2 * NP * NP)


def test_mmd_workspace_matches_its_documented_formula():
    from regda_amd import _lib
    L = _lib.lib()
    for ns, nt, d in ((8192, 8192, 2048), (24, 40, 64), (130, 126, 96), (2, 2, 32), (16384, 16384, 32), (2048, 2048, 2048)):
        assert L.size('rgda_mmd_loss_workspace', ns, nt, d) == workspace_formula(ns, nt, d), (ns, nt, d)
    assert workspace_formula(16384, 16384, 32) >= 2 << 30          # W alone is 2 GB at the limit
    for ns, nt, d in ((1, 64, 64), (64, 1, 64), (64, 64, 48), (64, 64, 0), (16384, 16385, 64), (32768, 2, 64)):
        assert L.size('rgda_mmd_loss_workspace', ns, nt, d) == 0, (ns, nt, d)


def test_mmd_entry_point_rejects_bad_arguments_before_any_launch():
    from regda_amd import _lib
    L = _lib.lib()
    fake = ctypes.c_void_p(256)       # never dereferenced: the arguments are rejected first

    def call(feat_s=fake, bs=2, hws=16, feat_t=fake, bt=2, hwt=16, d=64, ktype=0, mul=2.0, num=5, loss=fake, dfs=None,
             ldds=0, ws=fake, ws_bytes=1 << 40):
        L.call('rgda_mmd_loss', feat_s, bs, hws, hws, d * hws, feat_t, bt, hwt, hwt, d * hwt, d, ktype, mul, num, 0.0,
               loss, dfs, ldds, None, 0, 0, 1.0, ws, ws_bytes, None)
    for kw in (dict(feat_s=None), dict(feat_t=None), dict(loss=None), dict(ws=None), dict(ws=ctypes.c_void_p(272)),
               dict(d=48), dict(d=0), dict(bs=1, hws=1), dict(bt=1, hwt=1),                      # d % 32, ns = 1, nt = 1
               dict(num=0), dict(num=9), dict(mul=0.0), dict(mul=-2.0), dict(ktype=2),
               dict(bs=1, hws=16385, bt=1, hwt=16384),                                        # n = 32769
               dict(dfs=fake, ldds=60), dict(dfs=fake, ldds=68)):
        with pytest.raises(ValueError):
            call(**kw)
    with pytest.raises(ValueError):           # the linear form has the same limits
        call(ktype=1, d=48)
    with pytest.raises(_lib.RgdaError):       # workspace too small
        call(ws_bytes=16)
    with pytest.raises(_lib.RgdaError):       # the rbf form does not run on the linear form's a(12 d) bytes
        call(ws_bytes=768)
    with pytest.raises(_lib.RgdaError):       # and the linear form needs those
        call(ktype=1, ws_bytes=767)


def test_steps_reject_an_unknown_align_domain_value():
    from regda_amd.align import AlignStep
    from regda_amd.source import SourceStep, domain_kind
    for bad in ('mmd_rbf', 'CORAL', 2, None, 1.5):
        for make in (lambda: SourceStep(None, align_domain=bad), lambda: AlignStep(None, None, align_domain=bad)):
            with pytest.raises(ValueError):
                make()
    with pytest.raises(ValueError):
        SourceStep(None, align_domain='mmd', mmd=dict(sigma=1.0))
    assert domain_kind(False) == (None, {}) and domain_kind(True) == ('coral', {}) and domain_kind('coral')[0] == 'coral'
    assert domain_kind('mmd', dict(kernel_num=3)) == ('mmd', dict(kernel_num=3)) and domain_kind('mmd_linear')[0] == 'mmd_linear'
