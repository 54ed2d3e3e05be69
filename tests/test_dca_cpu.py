"""CPU: Deep Covariance Alignment restated (tests/dca_ref.py) against the reference's own module (tests/golden/dca.npz)
and against float64 autograd of the definition; the conditions the structured inputs of every cov case satisfy; the
emulated contract of rgda_dca_loss against its derived tolerances; the exports, the workspace formulas and the argument
validation of rgda_dca_context / rgda_dca_loss (no GPU needed: every check comes before a launch); AlignStep's
dca_weight."""
import ctypes
import json
import os

import pytest
import torch

from dca_ref import (CASES, GOLDEN_NAMES, LOW, case_inputs, check_cov_conditions, cov_conditions, dca_differentiable,
                     dca_emulated, dca_restated, golden_cases, make_inputs, probs, random_inputs, relnorm)

HERE = os.path.dirname(os.path.abspath(__file__))


def _golden_sides(g):
    return tuple((torch.from_numpy(g['feat_' + s]), (torch.from_numpy(g['l1_' + s]), torch.from_numpy(g['l2_' + s])))
                 for s in 'ab')


def test_restated_dca_matches_the_reference_goldens(gold):
    """The reference ran in fp32: its own noise is measured here, as the deviation of an fp32 run of the restatement from
    float64 on the same inputs, with the project's margin of 3 and a floor of one fp32 rounding (2^-23)."""
    cases = list(golden_cases(gold('dca.npz')))
    assert [name for name, _ in cases] == GOLDEN_NAMES
    seen = set()
    for name, g in cases:
        sides = _golden_sides(g)
        for got, want in zip(sides, case_inputs(name)):          # the goldens hold the shared inputs
            assert torch.equal(got[0], want[0]) and all(torch.equal(a, b) for a, b in zip(got[1], want[1]))
        for key, kind, with_a in (('ccr', 'cov', False), ('icr', 'cov', True), ('msecross', 'mse', False)):
            if key + '_loss' not in g:
                continue
            seen.add(key)
            r = dca_restated(sides, 'logits2', kind, True)
            f = dca_restated(sides, 'logits2', kind, True, dtype=torch.float32)
            noise_l = max(abs(f['loss'] - r['loss']) / abs(r['loss']), 2.0 ** -23)
            lrel = abs(float(g[key + '_loss']) - r['loss']) / abs(r['loss'])
            print(name, key, 'loss', float(g[key + '_loss']), r['loss'], 'rel', lrel, 'bound', 3 * noise_l)
            assert lrel <= 3 * noise_l, (name, key, lrel, noise_l)
            assert (key + '_rows_a' in g) == with_a
            for s in ('ab' if with_a else 'b'):
                noise_g = max(relnorm(f['rows_' + s], r['rows_' + s]), 2.0 ** -23)
                grel = relnorm(g[key + '_rows_' + s], r['rows_' + s])
                print(name, key, 'rows', s, 'rel', grel, 'bound', 3 * noise_g)
                assert grel <= 3 * noise_g, (name, key, s, grel, noise_g)
    assert seen == {'ccr', 'icr', 'msecross'}


def _rows(g):
    return g.flatten(2).permute(0, 2, 1).reshape(-1, g.shape[1])


@pytest.mark.parametrize('kind', ['cov', 'mse'])
@pytest.mark.parametrize('ignore_bg', [True, False])
@pytest.mark.parametrize('name', ['b2_k6_c32_5x7', 'b4_k7_c96_9x9', 'b2_k16_c64_8x8'])
def test_closed_form_gradient_equals_float64_autograd_of_the_definition(name, ignore_bg, kind):
    """both sides; the source side of CCR / MSE_cross is a constant of the definition: detached, it receives exactly
    zero, and the target gradient is unchanged"""
    (fa, pa), (fb, pb) = sides = case_inputs(name)
    Pa, Pb = probs(pa, 'logits2'), probs(pb, 'logits2')
    r = dca_restated(sides, 'logits2', kind, ignore_bg)
    xa, xb = fa.double().requires_grad_(True), fb.double().requires_grad_(True)
    loss = dca_differentiable(xa, Pa, xb, Pb, kind, ignore_bg)
    loss.backward()
    assert r['loss'] == pytest.approx(loss.item(), rel=1e-10)
    for got, ref in ((r['rows_a'], _rows(xa.grad)), (r['rows_b'], _rows(xb.grad))):
        assert (got - ref).abs().max() <= 1e-10 * ref.abs().max(), (name, kind, ignore_bg)
    if kind == 'cov':
        clamped = (r['R'] <= LOW) & ~torch.eye(r['R'].shape[0], dtype=torch.bool)
        assert (r['W'][clamped] == 0).all()
        if name == 'b2_k6_c32_5x7' and ignore_bg:
            assert clamped.any()                                  # a clamped off-diagonal entry carries no gradient
    xa2, xb2 = fa.double().requires_grad_(True), fb.double().requires_grad_(True)
    dca_differentiable(xa2.detach(), Pa, xb2, Pb, kind, ignore_bg).backward()
    assert xa2.grad is None and torch.equal(xb2.grad, xb.grad)


def test_structured_inputs_meet_the_cov_conditions_and_unstructured_ones_do_not():
    """float64: min diag >= 0.5, max off-diagonal <= 0.9, every off-diagonal entry at least 1e-4 from the 1e-6 switch
    (fp32 noise of R is around 1e-6, so no case depends on which side of the switch an entry falls); no entry excused"""
    for name in CASES:
        got = check_cov_conditions(dca_restated(case_inputs(name))['R'], name)
        print(name, 'min diag %.3f max offdiag %.3f gap to the switch %.2e clamped share %.2f' % got)
    variants = {'ccr 2+3': make_inputs(2, 6, 64, 6, 7, 1.0, 3.0, 51, b_b=3), 'view': make_inputs(2, 6, 64, 5, 7, 1.0, 3.0, 61)}
    (_, _), (fb, pb) = variants['ccr 2+3']
    variants['icr 1+2'] = ((fb[:1], tuple(p[:1] for p in pb)), (fb[1:], tuple(p[1:] for p in pb)))
    for tag, sides in variants.items():
        check_cov_conditions(dca_restated(sides)['R'], tag)
    sides = case_inputs('b4_k7_c96_9x9')
    for pk, sd in (('prob', tuple((f, (p[0].softmax(1),)) for f, p in sides)), ('logits', tuple((f, (p[0],)) for f, p in sides)),
                   ('logits2', sides)):
        for ig in (True, False):
            check_cov_conditions(dca_restated(sd, pk, 'cov', ig)['R'], (pk, ig))
    from test_dca_gpu import NAN_SEED
    r = dca_restated(random_inputs(2, 6, 64, 8, 8, NAN_SEED))
    assert cov_conditions(r['R'])[0] <= -0.01 and r['loss'] != r['loss']


def test_emulated_contract_stays_within_the_derived_tolerances():
    """dca_tolerances.json is what derive_dca_tolerances.py observes: the committed file is current"""
    tol = json.load(open(os.path.join(HERE, 'golden', 'dca_tolerances.json')))
    assert tol['margin'] == 3.0 and set(tol['bounds']) == set(tol['observed']) == set(CASES)
    for name in CASES:
        sides = case_inputs(name)
        for kind in ('cov', 'mse'):
            r = dca_restated(sides, 'logits2', kind, True)
            obs = dict(loss_rel=2.0 ** -23, u_rel=0.0, grad_rel=0.0)
            for reverse in (False, True):
                e = dca_emulated(sides, 'logits2', kind, True, reverse=reverse)
                obs['loss_rel'] = max(obs['loss_rel'], abs(e['loss'] - r['loss']) / abs(r['loss']))
                obs['u_rel'] = max(obs['u_rel'], relnorm(torch.cat([e['u_a'], e['u_b']]), torch.cat([r['u_a'], r['u_b']])))
                obs['grad_rel'] = max(obs['grad_rel'], relnorm(torch.cat([e['grad_a'], e['grad_b']]),
                                                               torch.cat([r['rows_a'], r['rows_b']])))
            for m, v in obs.items():
                assert v == pytest.approx(tol['observed'][name][kind][m], rel=1e-3), (name, kind, m)
                assert tol['bounds'][name][kind][m] == pytest.approx(3.0 * tol['observed'][name][kind][m])
            assert obs['grad_rel'] <= 2.0 ** -8 and obs['u_rel'] <= 1e-5          # bf16 rows; fp32 contexts


def test_emulated_prior_joins_before_the_one_rounding():
    sides = case_inputs('b2_k6_c32_5x7')
    e = dca_emulated(sides, weight=0.5)
    prior = torch.randn(e['rows_b'].shape, generator=torch.Generator().manual_seed(1)).bfloat16()
    p = dca_emulated(sides, weight=0.5, prior=(None, prior))
    assert torch.equal(p['grad_a'], e['grad_a'])
    assert torch.equal(p['grad_b'], (e['rows_b'] + prior.float()).bfloat16())
    assert e['loss'] == pytest.approx(0.5 * dca_emulated(sides)['loss'], rel=1e-6)


def test_library_exports_the_dca_entry_points():
    from regda_amd import _lib, dca_modules, ops
    from regda_amd.plan import MAX_ARGS
    L = _lib.lib()
    for name in ('rgda_dca_context', 'rgda_dca_context_workspace', 'rgda_dca_loss', 'rgda_dca_loss_workspace'):
        assert name in L.protos and name not in L.missing
        assert L.raw(name) is not None
    assert L.raw('rgda_plan_fn_id')(b'rgda_dca_loss') >= 0 and L.raw('rgda_plan_fn_id')(b'rgda_dca_context') >= 0
    assert L.raw('rgda_plan_fn_id')(b'rgda_dca_loss_workspace') == -1
    assert len(L.protos['rgda_dca_loss'][1]) == 27 <= MAX_ARGS and len(L.protos['rgda_dca_context'][1]) == 17
    assert L.raw('rgda_abi_version')() == 10
    assert callable(ops.dca_loss) and callable(ops.dca_context)
    m = dca_modules.CategoryAlign_Module()
    assert (m.num_classes, m.ignore_bg) == (7, False)
    for fn in ('ICR', 'CCR', 'MSE_intra', 'MSE_cross'):
        assert callable(getattr(dca_modules, fn))
    import inspect
    assert list(inspect.signature(dca_modules.ICR).parameters) == ['inputs', 'num_classes', 'multi_layer', 'ignore_bg']
    assert list(inspect.signature(dca_modules.CCR).parameters) == ['source', 'target', 'num_classes', 'multi_layer', 'ignore_bg']
    assert list(inspect.signature(dca_modules.MSE_intra).parameters) == ['inputs', 'multi_layer', 'ignore_bg']
    assert list(inspect.signature(dca_modules.MSE_cross).parameters) == ['source', 'target', 'multi_layer', 'ignore_bg']


def _a(x):
    return (x + 255) // 256 * 256


def loss_workspace_formula(ba, bb, c, C, ignore_bg):
    """the formula documented at rgda_dca_loss_workspace (include/rgda_hip.h)"""
    n = C - 1 if ignore_bg else C
    per_side = sum(_a(4 * b * n * c) + _a(4 * b * c) + _a(4 * b * C) + _a(4 * b * C * c) for b in (ba, bb))
    return 256 + per_side + 2 * _a(8 * n * c) + _a(4 * (2 * n + 2 * n * n)) + _a(4 * ((c + 255) // 256) * max(ba, bb))


def test_dca_workspaces_match_their_documented_formulas():
    from regda_amd import _lib
    L = _lib.lib()
    for ba, bb, c, C, ig in ((8, 8, 2048, 16, 1), (8, 8, 2048, 6, 1), (2, 3, 32, 6, 0), (1, 2, 96, 7, 1), (4, 4, 64, 16, 0)):
        assert L.size('rgda_dca_loss_workspace', ba, bb, c, C, ig) == loss_workspace_formula(ba, bb, c, C, ig), (ba, bb, c, C)
    assert loss_workspace_formula(8, 8, 2048, 16, 1) < 8 << 20          # the production shape: under 8 MB
    for ba, bb, c, C in ((0, 2, 64, 6), (2, 0, 64, 6), (2, 2, 48, 6), (2, 2, 0, 6), (2, 2, 16, 6), (2, 2, 64, 5), (2, 2, 64, 17)):
        assert L.size('rgda_dca_loss_workspace', ba, bb, c, C, 1) == 0, (ba, bb, c, C)
    for b, c in ((8, 2048), (1, 32), (3, 96)):
        assert L.size('rgda_dca_context_workspace', b, c) == _a(4 * b * c)
    for b, c in ((0, 64), (2, 48), (2, 16)):
        assert L.size('rgda_dca_context_workspace', b, c) == 0


def test_dca_entry_points_reject_bad_arguments_before_any_launch():
    from regda_amd import _lib
    L = _lib.lib()
    fake = ctypes.c_void_p(256)       # never dereferenced: the arguments are rejected first

    def loss(feat_a=fake, b_a=2, ldc_a=None, ldb_a=None, p1_a=fake, p2_a=fake, df_a=None, feat_b=fake, b_b=2, ldc_b=None,
             ldb_b=None, p1_b=fake, p2_b=fake, df_b=None, hw=16, c=64, C=6, pred_kind=2, ignore_bg=1, kind=0, out=fake, ldd=0,
             ws=fake, ws_bytes=1 << 40):
        L.call('rgda_dca_loss', feat_a, b_a, hw if ldc_a is None else ldc_a, c * hw if ldb_a is None else ldb_a, p1_a, p2_a,
               df_a, feat_b, b_b, hw if ldc_b is None else ldc_b, c * hw if ldb_b is None else ldb_b, p1_b, p2_b, df_b, hw, c,
               C, pred_kind, ignore_bg, kind, out, ldd, 0, 1.0, ws, ws_bytes, None)
    for kw in (dict(feat_a=None), dict(feat_b=None), dict(p1_a=None), dict(p1_b=None), dict(p2_a=None), dict(p2_b=None),
               dict(out=None), dict(ws=None), dict(ws=ctypes.c_void_p(272)),
               dict(c=48), dict(c=0), dict(c=16), dict(hw=0),
               dict(b_a=0), dict(b_b=0), dict(b_a=-1),
               dict(ldc_a=8), dict(ldc_b=8), dict(ldb_a=100), dict(ldb_b=100),
               dict(df_a=fake, ldd=60), dict(df_b=fake, ldd=68), dict(df_b=ctypes.c_void_p(264), ldd=64),
               dict(df_a=ctypes.c_void_p(264), ldd=64),
               dict(pred_kind=3), dict(pred_kind=-1), dict(kind=2), dict(kind=-1),
               dict(kind=1, b_a=2, b_b=3)):
        with pytest.raises(ValueError, match='status -1'):
            loss(**kw)
    loss_ok = dict(p2_a=None, p2_b=None, pred_kind=1)                  # one logit map needs no second plane ...
    for C in (5, 17, 0):                                               # ... and reaches the class-count check
        with pytest.raises(ValueError, match='status -4'):
            loss(C=C, **loss_ok)
    with pytest.raises(_lib.RgdaError, match='status -2'):             # workspace too small
        loss(ws_bytes=loss_workspace_formula(2, 2, 64, 6, 1) - 1)

    def context(feat=fake, b=2, hw=16, ldc=None, ldb=None, p1=fake, p2=fake, pred_kind=2, c=64, C=6, u=fake, ws=fake,
                ws_bytes=1 << 40):
        L.call('rgda_dca_context', feat, b, hw, hw if ldc is None else ldc, c * hw if ldb is None else ldb, p1, p2, pred_kind,
               c, C, 1, u, None, None, ws, ws_bytes, None)
    for kw in (dict(feat=None), dict(p1=None), dict(p2=None), dict(u=None), dict(ws=None), dict(ws=ctypes.c_void_p(272)),
               dict(c=48), dict(c=16), dict(hw=0), dict(b=0), dict(ldc=8), dict(ldb=100), dict(pred_kind=3)):
        with pytest.raises(ValueError, match='status -1'):
            context(**kw)
    with pytest.raises(ValueError, match='status -4'):
        context(C=17)
    with pytest.raises(_lib.RgdaError, match='status -2'):
        context(ws_bytes=_a(4 * 2 * 64) - 1)


def test_align_step_rejects_a_negative_dca_weight_and_icr_on_one_image():
    from regda_amd.align import AlignStep
    for w in (-1, -1e-3):
        with pytest.raises(ValueError):
            AlignStep(None, None, dca_weight=w)
    st = AlignStep.__new__(AlignStep)                # the check comes first in step(): no model, no GPU
    st.dca_weight, st.dca = 1.0, dict(kind='cov', ccr=True, icr=True, ignore_bg=True)
    one, two = torch.zeros(1, 3, 8, 8), torch.zeros(2, 3, 8, 8)
    for a, b in ((one, one), (one, two), (two, one)):
        with pytest.raises(ValueError, match='icr'):
            st.step(a, None, b, None, 1e-3)
