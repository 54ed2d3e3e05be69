"""CPU: the class-aware whitening loss restated from its formulas (tests/whiten_ref.py) against the reference's own
ClassWareWhitening (tests/golden/whiten.npz) and against float64 autograd; the exports, the workspace formula and the
argument validation of rgda_whiten_loss (no GPU needed: every check comes before a launch)."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

from whiten_ref import golden_cases, whiten_emulated, whiten_restated, whiten_restated_autograd

HERE = os.path.dirname(os.path.abspath(__file__))


def test_restated_whitening_matches_the_reference_goldens(gold):
    """fp32 precision: the reference ran in fp32 (relative 2^-24 per operation, sums of <= 200 rows)."""
    g = gold('whiten.npz')
    cases = list(golden_cases(g))
    assert [c['name'] for c in cases] == ['k64g1_c6', 'k64g2_c7', 'k256g4_c16']
    for c in cases:
        lab = c['labels']
        counts = [(lab == i).sum().item() for i in range(c['class_num'])]
        assert 0 in counts and 1 in counts and (lab == -1).any(), c['name']     # empty class, singleton class, ignored
        loss, grad = whiten_restated(c['feats'], lab, range(c['class_num']), c['groups'])
        assert loss.item() == pytest.approx(c['loss'], rel=2e-6), c['name']
        ref = c['grad'].double()
        assert (grad - ref).abs().max().item() <= 2e-6 * ref.abs().max().item(), c['name']
        # the singleton class and the ignored pixels carry no gradient, in the reference too
        single = counts.index(1)
        dead = ((lab == -1) | (lab == single)).unsqueeze(1).expand_as(ref)
        assert ref[dead].abs().max().item() <= 1e-7 * ref.abs().max().item() and grad[dead].abs().max().item() == 0.0


def test_restated_whitening_reproduces_the_hand_worked_example(gold):
    """the 6 x 4 example of the reference's __main__ (class_ids [1, 2], groups 1): it prints 12.4375"""
    g = gold('whiten.npz')
    assert float(g['hand_loss']) == 12.4375
    feats, lab = torch.from_numpy(g['hand_feats']), torch.from_numpy(g['hand_lab'].astype(np.int64))
    loss, grad = whiten_restated(feats, lab, [int(i) for i in g['hand_class_ids']], 1)
    assert loss.item() == pytest.approx(12.4375, rel=1e-12)
    np.testing.assert_allclose(grad.numpy(), g['hand_grad'], rtol=1e-6, atol=1e-6)


def test_closed_form_gradient_equals_float64_autograd(gold):
    g = gold('whiten.npz')
    for c in golden_cases(g):
        loss, grad = whiten_restated(c['feats'], c['labels'], range(c['class_num']), c['groups'])
        al, ag = whiten_restated_autograd(c['feats'], c['labels'], range(c['class_num']), c['groups'])
        assert loss.item() == pytest.approx(al.item(), rel=1e-13)
        assert (grad - ag).abs().max().item() <= 1e-13 * ag.abs().max().item(), c['name']
    gen = torch.Generator().manual_seed(4)
    feats = torch.randn(2, 96, 5, 7, generator=gen)
    lab = torch.randint(-1, 4, (2, 5, 7), generator=gen)
    lab[lab == 3] = -1
    lab[0, 0, 0] = 3                                  # a class with a single pixel
    loss, grad = whiten_restated(feats, lab, range(6), 3)
    al, ag = whiten_restated_autograd(feats, lab, range(6), 3)
    assert loss.item() == pytest.approx(al.item(), rel=1e-13)
    assert (grad - ag).abs().max().item() <= 1e-13 * ag.abs().max().item()
    assert grad[0, :, 0, 0].abs().max().item() == 0.0


def test_emulated_contract_stays_within_the_derived_tolerances(gold):
    """whiten_tolerances.json is what derive_whiten_tolerances.py observes: the committed file is current"""
    tol = json.load(open(os.path.join(HERE, 'golden', 'whiten_tolerances.json')))
    assert tol['margin'] == 3.0
    g = gold('whiten.npz')
    for c in golden_cases(g):
        rl, rg = whiten_restated(c['feats'], c['labels'], range(c['class_num']), c['groups'])
        el, eg = whiten_emulated(c['feats'], c['labels'], c['class_num'], c['groups'])
        obs = tol['observed'][c['name']]
        assert abs(el.item() - rl.item()) / rl.item() == pytest.approx(obs['loss_rel'], rel=1e-3, abs=1e-9)
        assert ((eg.double() - rg).norm() / rg.norm()).item() == pytest.approx(obs['grad_rel'], rel=1e-3)
    assert set(tol['bounds']) == set(tol['observed']) and 'production' in tol['bounds']
    for name, obs in tol['observed'].items():
        for m in ('loss_rel', 'grad_rel'):
            assert tol['bounds'][name][m] == pytest.approx(3.0 * obs[m])


def test_library_exports_the_whitening_entry_points():
    from regda_amd import _lib
    L = _lib.lib()
    for name in ('rgda_whiten_loss', 'rgda_whiten_loss_workspace'):
        assert name in L.protos and name not in L.missing
        assert L.raw(name) is not None
    assert L.raw('rgda_plan_fn_id')(b'rgda_whiten_loss') >= 0          # replayable through the plan dispatch table


def _a(x):
    return (x + 255) // 256 * 256


def workspace_formula(n, k, C, groups):
    """the formula documented at rgda_whiten_loss_workspace (include/rgda_hip.h)"""
    s = k // groups
    NP = (n + 63) // 64 * 64 + 64 * C
    return 256 + _a(4 * NP) + _a(4 * NP // 64) + _a(4 * C * k) + 2 * _a(2 * k * NP) + _a(2 * C * k * s) + _a(4 * C * groups)


def test_whiten_workspace_matches_its_documented_formula():
    from regda_amd import _lib
    L = _lib.lib()
    for n, k, C, groups in ((8192, 2048, 6, 32), (8192, 2048, 16, 32), (192, 64, 6, 1), (192, 64, 7, 2), (100, 256, 16, 4),
                            (1, 96, 9, 1), (4097, 384, 12, 3)):
        assert L.size('rgda_whiten_loss_workspace', n, k, C, groups) == workspace_formula(n, k, C, groups), (n, k, C, groups)
    # rejected arguments: 0
    for n, k, C, groups in ((0, 64, 6, 1), (192, 64, 5, 1), (192, 64, 17, 1), (192, 64, 6, 3), (192, 2048, 6, 1),
                            (192, 64, 6, 4), (192, 64, 6, 0), ((1 << 24) + 1, 64, 6, 1)):
        assert L.size('rgda_whiten_loss_workspace', n, k, C, groups) == 0, (n, k, C, groups)


def test_whiten_entry_point_rejects_bad_arguments_before_any_launch():
    from regda_amd import _lib
    L = _lib.lib()
    fake = ctypes.c_void_p(256)       # never dereferenced: the arguments are rejected first

    def call(feat=fake, b=2, hw=16, labels=fake, k=64, C=6, groups=1, loss=fake, dfeat=None, lddf=0, ws=fake,
             ws_bytes=1 << 30):
        L.call('rgda_whiten_loss', feat, b, hw, hw, k * hw, labels, k, C, groups, -1, loss, dfeat, lddf, 0, 1.0, ws,
               ws_bytes, None)
    for kw in (dict(feat=None), dict(labels=None), dict(loss=None), dict(ws=None),                # null pointers
               dict(k=64, groups=3), dict(groups=0), dict(b=0), dict(hw=0),                        # k % groups, sizes
               dict(dfeat=fake, lddf=68), dict(dfeat=fake, lddf=56), dict(dfeat=ctypes.c_void_p(264), lddf=64),
               dict(ws=ctypes.c_void_p(272)),                                                      # workspace not 256-byte aligned
               dict(k=2048, groups=1), dict(k=64, groups=4), dict(k=160, groups=1), dict(k=320, groups=2),  # unserved block
               dict(C=5), dict(C=17)):                                                             # unserved class count
        with pytest.raises(ValueError):
            call(**kw)
    raw = L.raw('rgda_whiten_loss')

    def status(k, groups, C=6, feat=fake):
        return raw(feat, 2, 16, 16, k * 16, fake, k, C, groups, -1, fake, None, 0, 0, 1.0, fake, 1 << 30, None)
    assert status(64, 1, feat=None) == -1 and status(64, 3) == -1            # RGDA_ERR_ARG
    assert status(2048, 1) == -4 and status(64, 4) == -4 and status(64, 1, C=17) == -4      # RGDA_ERR_UNSUPPORTED
    with pytest.raises(_lib.RgdaError):          # workspace too small
        call(ws_bytes=16)


def test_module_refuses_what_the_kernel_does_not_serve():
    from regda_amd.gast.class_ware_whiten import ClassWareWhitening
    with pytest.raises(NotImplementedError, match=r'range\(C\)'):
        ClassWareWhitening(class_ids=[1, 2], groups=1)
    few = ClassWareWhitening(class_ids=range(5), groups=1)      # built (an Aligner of any class_num is), refused when called
    with pytest.raises(NotImplementedError, match='6 <= C <= 16'):
        few(torch.zeros(1, 64, 2, 2), torch.zeros(1, 2, 2, dtype=torch.long))
    m = ClassWareWhitening(class_ids=range(6), groups=1)
    with pytest.raises(NotImplementedError, match=r'\(32, 64, 96, 128\)'):
        m(torch.zeros(1, 2048, 2, 2), torch.zeros(1, 2, 2, dtype=torch.long))
