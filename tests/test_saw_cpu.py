"""CPU: the semantic-aware whitening loss restated from its formulas (tests/saw_ref.py) against the reference's own SAW
(tests/golden/saw.npz) and against float64 autograd; the exports, the workspace formula and the argument validation of
rgda_saw_loss (no GPU needed: every check comes before a launch); the argument errors of SAW and AlignStep."""
import ctypes
import json
import os

import pytest
import torch

from saw_ref import (golden_cases, group_band, pair_band, saw_differentiable, saw_emulated, saw_margin, saw_plan,
                     saw_restated)

HERE = os.path.dirname(os.path.abspath(__file__))
NAMES = ['k64_c6', 'k70_c8', 'k48_c16', 'k32_c2', 'k32_c4_sel', 'hw2']


def _rel(got, ref):
    return ((got.double() - ref.double()).norm() / ref.double().norm()).item()


def test_restated_saw_matches_the_reference_goldens(gold):
    """fp32 precision: the reference ran in fp32 (sums of <= 96 products, 15 to 120 pairs, <= 20 groups)"""
    cases = list(golden_cases(gold('saw.npz')))
    assert [c['name'] for c in cases] == NAMES
    for c in cases:
        b, k, h, w = c['feats'].shape
        C = len(c['selected'])
        for row in c['selected']:                    # the reference's tie order is unspecified: the goldens have no tie
            assert c['W'][row].abs().unique().numel() == k, c['name']
        r = saw_restated(c['feats'], c['W'], c['selected'], c['relax_denom'])
        assert r['loss'].item() == pytest.approx(c['loss'], rel=1e-6), c['name']
        assert _rel(r['grad'], c['grad']) <= 1e-6, c['name']
        # no near tie: every sign and every active bit is decided far outside the fp32 bands
        assert (r['corr'].abs() >= pair_band(h * w)).all() and ((r['s'] - r['margin']).abs() >= group_band(h * w, C)).all()
        assert r['active'].any(), c['name']
        # the channels that fill no slot carry no gradient, in the reference too
        free = torch.ones(k, dtype=torch.bool)
        free[r['ch'].reshape(-1)] = False
        assert c['grad'][:, free].abs().sum().item() == 0.0 and r['grad'][:, free].abs().sum().item() == 0.0
    by = {c['name']: c for c in cases}
    r = saw_restated(by['k64_c6']['feats'], by['k64_c6']['W'], by['k64_c6']['selected'], 2.0)
    assert r['active'].any() and (~r['active']).any() and r['margin'] == 7.0        # both sides of the clamp
    assert saw_plan(by['k70_c8']['W'], by['k70_c8']['selected'])[0].shape == (8, 8)   # 70 // 8: six ranks unused
    assert saw_margin(2, 2.0) == 0.0 and saw_margin(4, 3.0) == 2.0 and saw_margin(6, 0) == 0.0 and saw_margin(16, 2.0) == 60.0
    assert by['hw2']['feats'].shape[2:] == (1, 2) and by['k32_c4_sel']['W'].shape[0] == 7


def test_closed_form_gradient_equals_float64_autograd(gold):
    for c in golden_cases(gold('saw.npz')):
        f = c['feats'].double().clone().requires_grad_(True)
        loss = saw_differentiable(f, c['W'], c['selected'], c['relax_denom'])
        loss.backward()
        r = saw_restated(c['feats'], c['W'], c['selected'], c['relax_denom'])
        assert r['loss'].item() == pytest.approx(loss.item(), rel=1e-13)
        assert _rel(r['grad'], f.grad) <= 1e-12, c['name']
    # a channel that two classes rank alike (a duplicate inside a group) and equal |w| (the tie rule)
    gen = torch.Generator().manual_seed(5)
    W = torch.randn(4, 24, generator=gen)
    W[0, 3] = W[1, 3] = 9.0
    W[2, 10:14] = -1.5
    ch, _ = saw_plan(W, [0, 1, 2, 3])
    assert ch[0, 0] == 3 and ch[0, 1] == 3
    order2 = torch.sort(W[2].abs(), descending=True, stable=True).indices.tolist()
    at = order2.index(10)
    assert order2[at:at + 4] == [10, 11, 12, 13]                 # equal values: the lower channel first
    feats = torch.randn(2, 24, 3, 5, generator=gen)
    f = feats.double().clone().requires_grad_(True)
    saw_differentiable(f, W, [0, 1, 2, 3], 0).backward()
    assert _rel(saw_restated(feats, W, [0, 1, 2, 3], 0)['grad'], f.grad) <= 1e-12


def test_saw_tolerances_file_is_current(gold):
    """saw_tolerances.json is what derive_saw_tolerances.py writes: bounds = 3 x observed, every case present, and an fp32
    evaluation of every golden on this machine (whose fp32 matrix product may add in another order than the one the file
    was derived with) stays within the bounds"""
    tol = json.load(open(os.path.join(HERE, 'golden', 'saw_tolerances.json')))
    assert tol['margin'] == 3.0 and set(tol['bounds']) == set(tol['observed']) == set(NAMES + ['production'])
    for name, obs in tol['observed'].items():
        for m in ('loss_rel', 'grad_rel'):
            assert tol['bounds'][name][m] == pytest.approx(3.0 * obs[m])
    for c in golden_cases(gold('saw.npz')):
        ref = saw_restated(c['feats'], c['W'], c['selected'], c['relax_denom'])
        emu = saw_emulated(c['feats'], c['W'], c['selected'], c['relax_denom'], table=ref)
        scale = (ref['s'][ref['active']].sum() / (ref['nod'] * c['feats'].shape[0])).item()
        bound = tol['bounds'][c['name']]
        assert abs(emu['loss'].item() - ref['loss'].item()) / scale <= bound['loss_rel'], c['name']
        assert _rel(emu['grad'], ref['grad']) <= bound['grad_rel'], c['name']


def test_library_exports_the_saw_entry_points():
    from regda_amd import _lib, ops
    L = _lib.lib()
    for name in ('rgda_saw_loss', 'rgda_saw_loss_workspace'):
        assert name in L.protos and name not in L.missing
        assert L.raw(name) is not None
    assert L.raw('rgda_plan_fn_id')(b'rgda_saw_loss') >= 0          # replayable through the plan dispatch table
    assert L.raw('rgda_abi_version')() == 10
    assert callable(ops.saw_loss) and callable(ops.saw_tables)


def _a(x):
    return (x + 255) // 256 * 256


def workspace_formula(b, hw, k, C):
    """the formula documented at rgda_saw_loss_workspace (include/rgda_hip.h)"""
    G, nod = k // C, C * (C - 1) // 2
    TS = (nod + 1 + 3) // 4 * 4
    return 256 + _a(TS * b * G) + 2 * _a(4 * b * G) + 2 * _a(4 * G * C) + _a(4 * k * C) + _a(4 * b * G * C * hw)


def test_saw_workspace_matches_its_documented_formula():
    from regda_amd import _lib
    L = _lib.lib()
    for b, hw, k, C in ((8, 1024, 2048, 6), (2, 96, 64, 6), (2, 96, 70, 8), (1, 32, 48, 16), (2, 35, 32, 2), (2, 35, 32, 4),
                        (2, 2, 64, 6), (1, 2, 2, 2), (4, 4096, 4096, 16), (1, 1 << 24, 16, 16)):
        assert L.size('rgda_saw_loss_workspace', b, hw, k, C) == workspace_formula(b, hw, k, C), (b, hw, k, C)
    # rejected arguments: 0
    for b, hw, k, C in ((2, 96, 64, 5), (2, 96, 64, 3), (2, 96, 64, 32), (2, 96, 4, 6), (2, 1, 64, 6), (0, 96, 64, 6),
                        (2, 96, 4097, 6), (2, (1 << 23) + 1, 64, 6), (2, 96, 0, 6), (2, 0, 64, 6)):
        assert L.size('rgda_saw_loss_workspace', b, hw, k, C) == 0, (b, hw, k, C)


def test_saw_entry_point_rejects_bad_arguments_before_any_launch():
    from regda_amd import _lib
    L = _lib.lib()
    fake = ctypes.c_void_p(256)       # never dereferenced: the arguments are rejected first
    raw = L.raw('rgda_saw_loss')

    def status(feat=fake, b=2, hw=16, k=64, cls_w=fake, n_cls=7, ldw=None, sel=(0, 1, 2, 3, 4, 5), C=None, margin=7.0,
               loss=fake, dfeat=None, lddf=0, ws=fake, ws_bytes=1 << 40, ldc=None, ldb=None):
        C = len(sel) if C is None else C
        selected = None if sel is None else (ctypes.c_int32 * max(len(sel), 1))(*sel)
        ldc = hw if ldc is None else ldc
        return raw(feat, b, hw, ldc, k * ldc if ldb is None else ldb, k, cls_w, n_cls, k if ldw is None else ldw, selected,
                   C, margin, loss, dfeat, lddf, 0, 1.0, ws, ws_bytes, None)
    ARG, WORKSPACE, UNSUPPORTED = -1, -2, -4
    # outside the served shapes
    assert status(sel=(0, 1, 2, 3, 4)) == UNSUPPORTED                      # C = 5
    assert status(sel=(0, 1, 2)) == UNSUPPORTED and status(sel=tuple(range(6)), C=32) == UNSUPPORTED
    assert status(k=4) == UNSUPPORTED                                      # k < C
    assert status(hw=1) == UNSUPPORTED                                     # the division by hw - 1
    assert status(k=4097) == UNSUPPORTED
    assert status(b=2, hw=(1 << 23) + 1) == UNSUPPORTED                    # b * hw > 2^24
    # bad arguments
    for kw in (dict(feat=None), dict(cls_w=None), dict(sel=None, C=6), dict(loss=None), dict(ws=None),       # null pointers
               dict(sel=(0, 1, 2, 3, 4, 7)), dict(sel=(0, 1, 2, 3, 4, -1)),                                   # outside [0, n_cls)
               dict(sel=(0, 1, 2, 3, 4, 4)), dict(sel=(2, 1, 2, 3, 4, 5)),                                    # repeated
               dict(b=0), dict(hw=0), dict(k=0), dict(n_cls=0), dict(ldw=63),                                 # sizes, weight stride
               dict(ldc=15), dict(ldb=64 * 16 - 1),                                                           # feature strides
               dict(margin=-1.0), dict(margin=float('nan')),
               dict(dfeat=fake, lddf=68), dict(dfeat=fake, lddf=56), dict(dfeat=ctypes.c_void_p(264), lddf=64),
               dict(ws=ctypes.c_void_p(272))):                                                                # workspace alignment
        assert status(**kw) == ARG, kw
    assert status(ws_bytes=16) == WORKSPACE
    # the wrapper raises ValueError for both kinds
    with pytest.raises(ValueError):
        L.call('rgda_saw_loss', fake, 2, 16, 16, 64 * 16, 64, fake, 7, 64, (ctypes.c_int32 * 5)(0, 1, 2, 3, 4), 5, 0.0, fake,
               None, 0, 0, 1.0, fake, 1 << 40, None)
    with pytest.raises(_lib.RgdaError):
        L.call('rgda_saw_loss', fake, 2, 16, 16, 64 * 16, 64, fake, 7, 64, (ctypes.c_int32 * 6)(0, 1, 2, 3, 4, 5), 6, 0.0,
               fake, None, 0, 0, 1.0, fake, 16, None)


def test_saw_module_and_align_step_argument_errors():
    from regda_amd import ops
    from regda_amd.align import AlignStep, saw_selection
    from regda_amd.gast.SAW import SAW, classifier_weight
    conv = torch.nn.Conv2d(32, 7, 1)
    for sel in ([0, 1, 2], [0, 1, 2, 3, 4], list(range(7)), []):
        with pytest.raises(ValueError, match=r'\(2, 4, 6, 8, 16\)'):
            SAW(conv, sel)
    with pytest.raises(ValueError, match='repeats'):
        SAW(conv, [0, 1, 1, 2])
    m = SAW(conv, [1, 2, 4, 6], relax_denom=3.0)
    assert m.C == 4 and m.margin == 2.0 and m.selected_classes == [1, 2, 4, 6]
    eye, mask, margin, nod = m.get_mask_matrix()
    assert eye.shape == (4, 4) and mask.sum().item() == 6 and margin == 2.0 and nod.item() == 6
    assert SAW(conv, range(6)).margin == 7.0 and SAW(conv, range(6), relax_denom=0).margin == 0.0
    # the weight as the reference finds it: the last "weight" entry, squeezed; or a tensor
    assert classifier_weight(conv).shape == (7, 32)
    seq = torch.nn.Sequential(torch.nn.Conv2d(8, 32, 1), torch.nn.Conv2d(32, 7, 1))
    assert torch.equal(classifier_weight(seq), seq[1].weight.detach().squeeze())
    W = torch.randn(7, 32)
    assert classifier_weight(W) is not None and SAW(W, range(6)).C == 6
    with pytest.raises(ValueError):
        classifier_weight(torch.nn.Conv2d(8, 7, 3))
    with pytest.raises(ValueError):
        classifier_weight(torch.nn.ReLU())
    with pytest.raises(ValueError, match='input channels'):
        SAW(W, range(6))(torch.zeros(1, 16, 2, 2))
    with pytest.raises(RuntimeError, match='GPU only'):          # no CPU fallback
        SAW(W, range(6))(torch.zeros(1, 32, 2, 2))
    assert ops.saw_margin(6, 2.0) == 7.0 and ops.saw_margin(6, 0.0) == 0.0 and ops.saw_margin(2, 2.0) == 0.0
    # AlignStep: the weight is checked before the model is touched; the selection before anything is launched
    with pytest.raises(ValueError, match='saw_weight'):
        AlignStep(None, None, saw_weight=-1.0)
    assert saw_selection(6, None) == list(range(6)) and saw_selection(7, [1, 2, 4, 6]) == [1, 2, 4, 6]
    with pytest.raises(ValueError, match='selected_classes'):
        saw_selection(7, None)
    with pytest.raises(ValueError):
        saw_selection(6, [0, 1, 2])
