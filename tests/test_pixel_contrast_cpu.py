"""CPU: the pixel-contrast loss restated from its formulas (tests/pixel_contrast_ref.py) against the reference's own
PixelContrastLoss (tests/golden/pixel_contrast.npz) and against float64 autograd of the definition; plan_anchors against
the recorded draws; the emulated arithmetic contract of rgda_pixel_contrast_loss against its derived tolerances; the
exports, the workspace formula and the argument validation of both entry points (no GPU needed: every check comes
before a launch); AlignStep's contrast_weight."""
import ctypes
import json
import os

import pytest
import torch

from pixel_contrast_ref import (NAMES, case_rows, contrast_autograd, contrast_emulated, contrast_restated, golden_cases,
                                pixel_rows, production_inputs, production_plan, rows_from_tables, sampling_restated,
                                select_restated, view_major)

HERE = os.path.dirname(os.path.abspath(__file__))
# the reference's fp32 noise against the float64 restatement, measured by tests/golden/make_pixel_contrast_goldens.py
REF_NOISE = dict(loss_rel=1.3e-7, grad_rel=2.5e-7)


def _rel(got, ref):
    return ((got.double() - ref.double()).norm() / ref.double().norm()).item()


@pytest.fixture(scope='module')
def cases(gold):
    return list(golden_cases(gold('pixel_contrast.npz')))


def test_restatement_matches_the_reference_goldens(cases):
    """The reference ran in fp32: its own noise against float64 was measured at 1.3e-7 (loss, relative) and 2.5e-7
    (gradient, relative norm) when the file was minted; the bounds are those with the project's margin of 3.  The
    selected pixels are bit-equal."""
    assert [c['name'] for c in cases] == NAMES
    shape = {c['name']: (tuple(c['feats'].shape), tuple(c['labels'].shape[1:]), tuple(c['sel'].shape)) for c in cases}
    assert shape['b2_k64_16x16_live'] == ((2, 64, 16, 16), (64, 64), (4, 100))
    assert shape['b2_k64_16x16_sat'] == shape['b2_k64_16x16_live']
    assert shape['b3_k96_16x16_live'] == ((3, 96, 16, 16), (32, 32), (5, 100))
    assert shape['b3_k64_16x32'] == ((3, 64, 16, 32), (16, 32), (12, 85))
    for c in cases:
        size = tuple(c['feats'].shape[2:])
        sel, anchors, n_view = sampling_restated(c['labels'], c['predict'], size, c['perms'])
        assert torch.equal(sel, c['sel']) and [a[1] for a in anchors] == c['classes'].tolist(), c['name']
        rows, cls = view_major(sel, anchors, size[0] * size[1])
        loss, grad = contrast_restated(pixel_rows(c['feats'])[rows], cls)
        lrel, grel = abs(loss.item() - c['loss']) / c['loss'], _rel(grad, c['grad'])
        print(c['name'], 'loss', loss.item(), c['loss'], 'rel', lrel, 'grad rel', grel)
        assert lrel <= 3 * REF_NOISE['loss_rel'], (c['name'], lrel)
        assert grel <= 3 * REF_NOISE['grad_rel'], (c['name'], grel)
    by = {c['name']: c for c in cases}
    assert by['b2_k64_16x16_live']['loss'] < 12 and by['b2_k64_16x16_sat']['loss'] > 300        # both regimes
    hk = {n: [a[2] for a in sampling_restated(c['labels'], c['predict'], tuple(c['feats'].shape[2:]), c['perms'])[1]]
          for n, c in by.items()}
    assert hk['b3_k64_16x32'] == [42] * 12                                   # n_view = 85: 42 hard + 43 easy
    assert hk['b2_k64_few_easy'][0] == 80 and hk['b2_k64_few_hard'][0] == 20 and hk['b2_k64_hard0'][0] == 0
    assert any(p.numel() == 0 for p in by['b2_k64_hard0']['perms'])          # the zero-length draw is recorded
    assert {int(r) // 256 for r in case_rows(by['b2_k64_absent'])[0]} == {0}  # image 1 contributes no anchor
    shared = by['b3_k96_16x16_live']['classes'].tolist()
    assert len(shared) > len(set(shared))                                    # a class shared by two images


def test_closed_form_gradient_equals_float64_autograd_of_the_definition(cases):
    """settles c_r, the positive and the negative weights and dF = (W + W^T) F / T"""
    for c in cases:
        rows, cls = case_rows(c)
        F = pixel_rows(c['feats'])[rows]
        loss, grad = contrast_restated(F, cls)
        al, ag = contrast_autograd(F, cls)
        assert loss.item() == pytest.approx(al.item(), rel=1e-12), c['name']
        assert (grad - ag).abs().max().item() <= 1e-11 * ag.abs().max().item(), c['name']


def test_plan_anchors_takes_the_recorded_draws(cases):
    from regda_amd.gast.contrastive import plan_anchors
    for c in cases:
        size = tuple(c['feats'].shape[2:])
        counts, order, flag = select_restated(c['labels'], c['predict'], 16, size)
        assert flag == 0
        torch.manual_seed(c['seed'])                     # generator=None: the global CPU generator, as the reference
        anchors, ranks = plan_anchors(counts)
        assert anchors.dtype == ranks.dtype == torch.int32 and tuple(ranks.shape) == tuple(c['sel'].shape)
        assert anchors[:, 1].tolist() == c['classes'].tolist(), c['name']
        o = 0
        for a in range(anchors.shape[0]):                # the draws themselves, the zero-length ones included
            hk = int(anchors[a, 2])
            assert ranks[a, :hk].tolist() == c['perms'][o][:hk].tolist()
            assert ranks[a, hk:].tolist() == c['perms'][o + 1][:ranks.shape[1] - hk].tolist()
            o += 2
        rows, cls = rows_from_tables(counts, order, anchors, ranks)
        want, wcls = case_rows(c)
        assert torch.equal(rows, want) and torch.equal(cls, wcls), c['name']
        gen = torch.Generator().manual_seed(c['seed'])   # an explicit generator takes the same draws
        a2, r2 = plan_anchors(counts, generator=gen)
        assert torch.equal(a2, anchors) and torch.equal(r2, ranks)
    none = torch.zeros(2, 7, 2, dtype=torch.int32)
    none[:, :, 0] = 50
    none[:, :, 1] = 50                                    # 100 pixels is not MORE than max_views
    assert plan_anchors(none) == (None, None)
    assert plan_anchors(none, max_views=99)[1].shape == (14, 73)


def test_emulated_contract_stays_within_the_derived_tolerances(cases):
    """pixel_contrast_tolerances.json is what derive_pixel_contrast_tolerances.py observes: the committed file is current"""
    tol = json.load(open(os.path.join(HERE, 'golden', 'pixel_contrast_tolerances.json')))
    assert tol['margin'] == 3.0 and tol['floor'] == dict(loss_rel=2.0 ** -20, grad_rel=2.0 ** -10)
    assert set(tol['bounds']) == set(tol['observed']) == set(tol['tight']) == set(tol['order']) == set(NAMES + ['production'])
    feats, labels, predict, C = production_inputs()
    assert feats.shape == (2, 2048, 32, 32)
    (prow, pcls), _ = production_plan(labels, predict, (32, 32))
    assert prow.numel() == 800
    todo = [(c['name'], pixel_rows(c['feats'])[case_rows(c)[0]], case_rows(c)[1]) for c in cases]
    todo.append(('production', pixel_rows(feats)[prow], pcls))
    for name, F, cls in todo:
        rl, rg = contrast_restated(F, cls)
        el, eg = contrast_emulated(F, cls, sums='exact')
        fl, fg = contrast_emulated(F, cls, sums='fp32')
        obs, order = tol['observed'][name], tol['order'][name]
        lo = max(abs(float(el) - float(rl)), abs(float(fl) - float(rl))) / abs(float(rl))
        go = max(_rel(eg, rg), _rel(fg, rg))
        assert lo <= tol['bounds'][name]['loss_rel'] and go <= tol['bounds'][name]['grad_rel'], name
        assert float(el) == pytest.approx(float(rl), rel=tol['bounds'][name]['loss_rel'])
        assert go == pytest.approx(obs['grad_rel'], rel=1e-2), name
        assert lo == pytest.approx(obs['loss_rel'], rel=0.5, abs=2e-7), name          # fp32 sums: the library's order may move
        assert _rel(fg, eg) <= tol['tight'][name]['grad_rel'] and abs(float(fl) - float(el)) / abs(float(el)) <= tol['tight'][name]['loss_rel']
        for m in ('loss_rel', 'grad_rel'):
            assert tol['bounds'][name][m] == pytest.approx(3.0 * obs[m])
            assert tol['tight'][name][m] == pytest.approx(3.0 * order[m] + tol['floor'][m])


def test_library_exports_the_pixel_contrast_entry_points():
    from regda_amd import _lib, ops
    from regda_amd.gast.contrastive import PixelContrastLoss, plan_anchors
    L = _lib.lib()
    for name in ('rgda_pixel_contrast_select', 'rgda_pixel_contrast_loss', 'rgda_pixel_contrast_loss_workspace'):
        assert name in L.protos and name not in L.missing
        assert L.raw(name) is not None
    for name in (b'rgda_pixel_contrast_select', b'rgda_pixel_contrast_loss'):
        assert L.raw('rgda_plan_fn_id')(name) >= 0          # replayable through the plan dispatch table
    assert len(L.protos['rgda_pixel_contrast_select'][1]) == 14 and len(L.protos['rgda_pixel_contrast_loss'][1]) == 24
    assert L.raw('rgda_abi_version')() == 10
    assert callable(ops.pixel_contrast_select) and callable(ops.pixel_contrast_loss) and callable(plan_anchors)
    m = PixelContrastLoss()
    assert (m.temperature, m.base_temperature, m.ignore_label, m.max_samples, m.max_views, m.eps) == (0.1, 0.07, -1, 1024, 100, 1e-5)
    assert m.generator is None
    m.max_views = 50                                        # assignable afterwards, as in the reference
    assert m.max_views == 50


def _a(x):
    return (x + 255) // 256 * 256


def workspace_formula(N, k):
    """the formula documented at rgda_pixel_contrast_loss_workspace (include/rgda_hip.h)"""
    NP = (N + 127) // 128 * 128
    T = NP // 128
    U = T * (T + 1) // 2
    g = k // 32
    S0 = min(g, min(max(256 // U, 1), 8))
    per = -(-g // S0)
    S = -(-g // per)
    return 2 * _a(4 * NP) + 2 * _a(2 * NP * k) + _a(20 * NP) + _a(4 * NP * NP) + _a(65536 * U * S) + _a(2 * NP * NP)


def test_pixel_contrast_workspace_matches_its_documented_formula():
    from regda_amd import _lib
    L = _lib.lib()
    for N, k in ((400, 64), (1020, 64), (500, 96), (800, 2048), (1024, 2048), (1, 32), (4096, 2048), (4096, 32), (200, 160)):
        assert L.size('rgda_pixel_contrast_loss_workspace', N, k) == workspace_formula(N, k), (N, k)
    for N, k in ((0, 64), (4097, 64), (400, 48), (400, 0), (-1, 64)):
        assert L.size('rgda_pixel_contrast_loss_workspace', N, k) == 0, (N, k)


def test_entry_points_reject_bad_arguments_before_any_launch():
    from regda_amd import _lib
    L = _lib.lib()
    fake = ctypes.c_void_p(256)       # never dereferenced: the arguments are rejected first

    def select(labels=fake, predict=fake, kind=0, b=2, C=7, H=64, W=64, h=16, w=16, counts=fake, order=fake, flag=fake):
        L.call('rgda_pixel_contrast_select', labels, predict, kind, b, C, H, W, h, w, -1, counts, order, flag, None)
    for kw in (dict(labels=None), dict(predict=None), dict(counts=None), dict(order=None), dict(flag=None), dict(kind=2),
               dict(b=0), dict(h=0), dict(C=1), dict(C=17), dict(H=65), dict(W=72), dict(H=40, h=16),     # H % h, W % w
               dict(H=256, W=256, h=256, w=128)):                                                      # h * w > 16384
        with pytest.raises(ValueError):
            select(**kw)

    def loss(feat=fake, b=2, hw=256, k=64, C=7, order=fake, counts=fake, anchors=fake, A=4, ranks=fake, n_view=100, T=0.1,
             Tb=0.07, eps=1e-5, out=fake, dfeat=None, lddf=0, ws=fake, ws_bytes=1 << 40, ldc=None):
        L.call('rgda_pixel_contrast_loss', feat, b, hw, hw if ldc is None else ldc, k * hw, k, C, order, counts, anchors, A,
               ranks, n_view, T, Tb, eps, out, dfeat, lddf, 0, 1.0, ws, ws_bytes, None)
    for kw in (dict(feat=None), dict(order=None), dict(counts=None), dict(anchors=None), dict(ranks=None), dict(out=None),
               dict(ws=None), dict(ws=ctypes.c_void_p(272)), dict(k=48), dict(k=0), dict(T=0.0), dict(Tb=-1.0), dict(eps=-1.0),
               dict(ldc=255), dict(A=0), dict(n_view=0), dict(A=41, n_view=100),                      # N = 0, N = 4100
               dict(C=1), dict(C=17), dict(dfeat=fake, lddf=60), dict(dfeat=fake, lddf=68),
               dict(dfeat=ctypes.c_void_p(264), lddf=64)):
        with pytest.raises(ValueError):
            loss(**kw)
    for kw in (dict(A=0), dict(A=41), dict(C=17)):          # the limits are "unsupported", not "bad argument"
        with pytest.raises(ValueError, match='status -4'):
            loss(**kw)
    with pytest.raises(ValueError, match='status -4'):
        select(H=40, h=16)
    with pytest.raises(_lib.RgdaError):       # workspace too small
        loss(ws_bytes=workspace_formula(400, 64) - 1)


def test_align_step_validates_contrast_weight():
    from regda_amd.align import AlignStep
    with pytest.raises(ValueError):
        AlignStep(None, None, contrast_weight=-0.5)
    import inspect
    assert inspect.signature(AlignStep.__init__).parameters['contrast_weight'].default == 0.0
