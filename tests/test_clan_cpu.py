"""CPU: the category-level adversarial path without a GPU -- the float64 restatement (tests/clan_ref.py) against the
goldens minted from the reference's own WeightedBCEWithLogitsLoss, the four new entry points as the header declares
them, the argument checks (which return before any launch), the refusals the step and the module make before they touch
the GPU, and the committed tolerance file against what its derive script observes."""
import ctypes
import json
import os
import sys

import pytest
import torch

import clan_ref as C
from regda_amd import _lib

HERE = os.path.dirname(os.path.abspath(__file__))
ARGS = {'rgda_clan_probs_fwd': 12, 'rgda_clan_probs_bwd': 15, 'rgda_wbce_logits_workspace': 3, 'rgda_wbce_logits': 20}
ARG, WS, UNSUP = -1, -2, -4


@pytest.fixture(scope='module')
def tol():
    return json.load(open(os.path.join(HERE, 'golden', 'clan_tolerances.json')))


def test_library_exports_the_entry_points_with_the_documented_arguments():
    L = _lib.lib()
    assert L.raw('rgda_abi_version')() == 10
    for name, n in ARGS.items():
        assert name in L.protos and name not in L.missing, name
        assert len(L.protos[name][1]) == n, (name, len(L.protos[name][1]))
        if name != 'rgda_wbce_logits_workspace':
            assert L.raw('rgda_plan_fn_id')(name.encode()) >= 0, name
    assert L.protos['rgda_wbce_logits_workspace'][0] is ctypes.c_size_t
    from regda_amd import ops
    for f in ('clan_probs', 'clan_probs_backward', 'wbce_logits'):
        assert callable(getattr(ops, f))


@pytest.mark.parametrize('name', list(C.GOLDEN_CASES))
def test_restatement_reproduces_the_reference(gold, name):
    """float64 against the reference's module evaluated in float64 on the same float32 inputs: two stable forms of one
    function, equal to rounding"""
    c = C.golden_case(gold, name)
    assert float(c['input'].abs().max()) == 80.0 and c['loss'].dtype == torch.float64
    loss, dz, gw = C.golden_restatement(c)
    assert torch.isfinite(c['loss']) and abs(float(loss - c['loss'])) < 1e-13 * abs(float(c['loss']))
    assert C.R.err(dz, c['dinput']) < 1e-13
    assert (gw is None) == (c['weight'] is None)
    if gw is not None:
        assert C.R.err(gw, c['dweight']) < 1e-13


def test_pair_restatement():
    x1, x2 = torch.randn(2, 6, 2, 3, dtype=torch.float64), torch.randn(2, 6, 2, 3, dtype=torch.float64)
    P, wmap = C.pair(x1, x2, (8, 9))
    assert P.shape == (2, 6, 8, 9) and wmap.shape == (2, 8, 9)
    assert torch.allclose(P.sum(1), torch.ones(2, 8, 9, dtype=torch.float64)) and (wmap > 0).all() and (wmap < 1).all()
    assert torch.allclose(P[..., 0, 0], torch.softmax(x1[..., 0, 0] + x2[..., 0, 0], 1))
    cos = torch.nn.functional.cosine_similarity(torch.softmax(x1, 1), torch.softmax(x2, 1), dim=1)
    assert torch.allclose(C.pair(x1, x2, (2, 3))[1], 1 - cos)
    assert C.pair(x1, x1, (8, 9))[1].abs().max() < 1e-15
    # the transpose helper is the adjoint of up()
    v, z = torch.randn(2, 1, 8, 9, dtype=torch.float64), torch.randn(2, 1, 2, 3, dtype=torch.float64)
    assert abs(float((C.up(z, (8, 9)) * v).sum() - (z * C.up_transpose(v, (2, 3))).sum())) < 1e-12


def test_workspace_query():
    L = _lib.lib()
    assert L.size('rgda_wbce_logits_workspace', 8, 512, 512) == 8 * 512 * 512 // 256 * 4
    assert L.size('rgda_wbce_logits_workspace', 2, 33, 35) == 256            # 10 partials, rounded up to 256 bytes
    for shape in ((0, 32, 32), (2, 0, 32), (2, 32, 0), (-1, 32, 32), (1, 1 << 16, 1 << 16), (1 << 10, 1 << 10, 1 << 10)):
        assert L.size('rgda_wbce_logits_workspace', *shape) == 0, shape


def test_argument_errors_before_any_launch():
    L = _lib.lib()
    p = ctypes.c_void_p(4096)          # non-null, aligned, never dereferenced: every call below returns before a launch
    odd = ctypes.c_void_p(4096 + 2)

    def pf(x1=p, x2=p, P=p, wmap=p, b=2, C=6, h=2, w=2, H=32, W=32, Cp=16):
        return L.raw('rgda_clan_probs_fwd')(x1, x2, P, wmap, b, C, h, w, H, W, Cp, None)

    def pb(dP=p, gw=p, x1=p, x2=p, dx1=p, dx2=p, b=2, C=6, h=2, w=2, H=32, W=32, Cp=16, scale=1.0):
        return L.raw('rgda_clan_probs_bwd')(dP, gw, x1, x2, dx1, dx2, b, C, h, w, H, W, Cp, scale, None)

    def wb(z=p, b=2, hz=1, wz=1, H=32, W=32, target=None, label=0.0, wmap=p, alpha=0.4, beta=40.0, scale=1.0, mean=1, loss=p,
           acc=0, dz=p, gw=p, ws=p, ws_bytes=1 << 20):
        return L.raw('rgda_wbce_logits')(z, b, hz, wz, H, W, target, label, wmap, alpha, beta, scale, mean, loss, acc, dz, gw,
                                         ws, ws_bytes, None)

    for kw in (dict(x1=None), dict(x2=None), dict(P=None), dict(wmap=None), dict(b=0), dict(h=0), dict(W=0), dict(P=odd),
               dict(x1=odd), dict(wmap=odd)):
        assert pf(**kw) == ARG, kw
    for kw in (dict(C=5), dict(C=17), dict(Cp=32), dict(Cp=8), dict(b=1 << 10, H=1 << 10, W=1 << 10)):
        assert pf(**kw) == UNSUP, kw
    for kw in (dict(dP=None), dict(x1=None), dict(x2=None), dict(dx1=None), dict(dx2=None), dict(scale=float('nan')),
               dict(dP=odd), dict(gw=odd), dict(w=0)):
        assert pb(**kw) == ARG, kw
    for kw in (dict(C=5), dict(C=17), dict(Cp=32), dict(b=1 << 10, H=1 << 10, W=1 << 10)):
        assert pb(**kw) == UNSUP, kw
    for kw in (dict(z=None), dict(loss=None), dict(ws=None), dict(b=0), dict(hz=0), dict(W=0), dict(label=0.5),
               dict(scale=float('nan')), dict(alpha=float('nan')), dict(wmap=None), dict(ws=odd), dict(dz=odd), dict(z=odd)):
        assert wb(**kw) == ARG, kw          # wmap=None with gw wanted: no weight, no gradient with respect to it
    assert wb(b=1, H=1 << 16, W=1 << 16) == UNSUP and wb(b=1 << 10, H=1 << 10, W=1 << 10) == UNSUP
    assert wb(ws_bytes=16, b=8, H=512, W=512) == WS
    with pytest.raises(ValueError):
        L.call('rgda_clan_probs_fwd', None, None, None, None, 2, 6, 2, 2, 32, 32, 16, None)


def test_refusals_need_no_gpu():
    from regda_amd.align import TERMS, AlignStep
    from regda_amd.loss import WeightedBCEWithLogitsLoss
    with pytest.raises(ValueError, match='adv_kind'):
        AlignStep(None, None, adv_kind='x')             # before the model is touched: there is none
    with pytest.raises(ValueError, match='adv_kind'):
        AlignStep(None, None, adv_kind=None, adv_weight=0.5)
    adv = [t for t in TERMS if t.name == 'adv'][0].params
    assert adv['kind'] == 'adaptsegnet' and adv['epsilon'] == 0.4 and adv['lambda_local'] == 40.0
    assert adv['preheat_steps'] == 0 and adv['weight_grad'] is True and adv['head_weights'] == (1.0, 1.0)
    crit = WeightedBCEWithLogitsLoss()
    assert crit.size_average is True and WeightedBCEWithLogitsLoss(size_average=False).size_average is False
    x = torch.zeros(2, 1, 4, 4)
    with pytest.raises(ValueError, match='Target size'):
        crit(x, torch.zeros(2, 1, 4, 5), None, 0.4, 40.0)
    with pytest.raises(ValueError, match='target'):
        crit(x, torch.zeros(2, 1, 4, 4, requires_grad=True), None, 0.4, 40.0)
    with pytest.raises(ValueError, match='Weight size'):
        crit(x, torch.zeros(2, 1, 4, 4), torch.zeros(4, 4), 0.4, 40.0)
    with pytest.raises(ValueError, match='GPU'):                 # served sizes on the CPU: no fallback
        crit(x, torch.zeros(2, 1, 4, 4), None, 0.4, 40.0)
    from regda_amd.gast.clan import CategoryAdversarialAligner
    for bad in (None, [object(), object()]):
        with pytest.raises(ValueError, match='exactly one'):
            CategoryAdversarialAligner(bad)
    with pytest.raises(ValueError, match='preheat_steps'):
        CategoryAdversarialAligner(object(), preheat_steps=-1)
    with pytest.raises(ValueError, match='lambda_local'):
        CategoryAdversarialAligner(object(), lambda_local=float('nan'))


def test_committed_tolerances_are_what_the_derive_script_observes(tol):
    """every case of the GPU tests has its bounds in the file, and the file is what derive_clan_tolerances.py computes here
    (float64 on the CPU: another machine's summation order moves a bound in its last digits)"""
    sys.path.insert(0, os.path.join(HERE, 'golden'))
    from derive_clan_tolerances import derive
    now = derive()
    assert tol['margin'] == 3.0 and tol['ulp_expf'] == C.ULP_EXPF and tol['ulp_log1pf'] == C.ULP_LOG1PF
    assert set(tol['pair']) == set(C.PAIR_CASES) and set(tol['golden']) == set(C.GOLDEN_CASES)
    assert set(tol['wbce']) == {C.bounds_key(s, v) for s in C.WBCE_SHAPES for v in C.wbce_variants(s)}
    for group in ('pair', 'wbce', 'golden'):
        for n, t in tol[group].items():
            assert set(t) == set(now[group][n]), (group, n)
            for q, v in t.items():
                assert v == pytest.approx(now[group][n][q], rel=1e-3), (group, n, q)
