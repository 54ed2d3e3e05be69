"""CPU: the PyCDA region pyramid term.  The new entry points (rgda_upsample_pycda, its workspace) are exported,
replayable and refuse bad arguments before anything touches the GPU; the float64 restatement (tests/pycda_ref.py) is
consistent with itself (closed-form gradient, image level, the strict integer threshold); and the generated inputs hold
what the GPU tests rely on: active and inactive regions at every finite level."""
import ctypes

import pytest
import torch

import pycda_ref

P = 4096        # a non-null pointer that is never dereferenced: every check here comes before a launch


def _ints(v):
    return (ctypes.c_int * len(v))(*v)


def test_new_entry_points_are_exported_and_replayable():
    from regda_amd import _lib, gast, ops
    from regda_amd.plan import MAX_ARGS
    L = _lib.lib()
    assert L.raw('rgda_abi_version')() == 10
    for name in ('rgda_upsample_pycda', 'rgda_upsample_pycda_workspace'):
        assert name in L.protos and name not in L.missing, name
    assert L.raw('rgda_plan_fn_id')(b'rgda_upsample_pycda') >= 0
    assert len(L.protos['rgda_upsample_pycda'][1]) <= MAX_ARGS
    assert callable(ops.upsample_pycda) and callable(gast.PyramidCurriculumLoss)


def _args(**kw):
    """A valid rgda_upsample_pycda call at 2 x 6 x 5 x 7 -> 33 x 45, sizes (4, 16, 0) (fake pointers), with overrides."""
    from regda_amd import _lib
    sizes = kw.pop('sizes', (4, 16, 0))
    b, c, h, w, H, W = kw.pop('b', 2), kw.pop('c', 6), kw.pop('h', 5), kw.pop('w', 7), kw.pop('H', 33), kw.pop('W', 45)
    arr = None if sizes is None else _ints(sizes)
    n = 0 if sizes is None else len(sizes)
    a = dict(heads=2, p1=P, p2=P + 4096, soft=P, sizes=arr, lw=None, levels=n, thresh=0.5, weight=1.0, acc=0, loss=P, n_active=P,
             g1=P, g2=P, flag=None, b=b, c=c, h=h, w=w, H=H, W=W, ws=P,
             ws_bytes=_lib.lib().size('rgda_upsample_pycda_workspace', b, c, h, w, H, W, arr, n), stream=None)
    a.update(kw)
    return list(a.values())


def test_upsample_pycda_refuses_bad_arguments_before_the_gpu():
    from regda_amd import _lib
    L = _lib.lib()
    good = _ints((4, 16, 0))
    need = L.size('rgda_upsample_pycda_workspace', 2, 6, 5, 7, 33, 45, good, 3)
    # at least: the finest cells' f64 means and int64 targets, and the row-contracted gradient
    assert need >= 2 * 9 * 12 * (2 * 6 * 8 + 6 * 8) + 2 * 33 * 2 * 6 * 7 * 4
    assert L.size('rgda_upsample_pycda_workspace', 0, 6, 5, 7, 33, 45, good, 3) == 0
    assert L.size('rgda_upsample_pycda_workspace', 2, 6, 5, 7, 33, 45, None, 3) == 0
    bad_sizes = [(4, 12, 0), (6,), (16, 4), (4, 4), (0, 4), (4, 0, 0), (2, 4, 8, 16, 32, 64, 128), (1, 4), (4, 512), (512,), ()]
    for sizes in bad_sizes:
        assert L.size('rgda_upsample_pycda_workspace', 2, 6, 5, 7, 33, 45, _ints(sizes), len(sizes)) == 0, sizes
        with pytest.raises(ValueError):
            L.call('rgda_upsample_pycda', *_args(sizes=sizes, ws_bytes=1 << 30))
    bad = [dict(p1=None), dict(p2=None), dict(soft=None), dict(sizes=None), dict(loss=None), dict(n_active=None), dict(ws=None),
           dict(g1=None), dict(g2=None), dict(heads=0), dict(heads=3), dict(heads=1), dict(b=0), dict(W=0), dict(thresh=1.5),
           dict(thresh=float('nan')), dict(weight=float('inf')), dict(lw=(ctypes.c_float * 3)(1.0, float('nan'), 1.0)),
           dict(b=1 << 16, H=1 << 8, W=1 << 7, ws_bytes=1 << 40)]
    for kw in bad:
        with pytest.raises(ValueError):
            L.call('rgda_upsample_pycda', *_args(**kw))
    for c in (5, 17):        # class counts outside 6..16: unsupported
        with pytest.raises(ValueError, match='status -4'):
            L.call('rgda_upsample_pycda', *_args(c=c))
    with pytest.raises(_lib.RgdaError, match='workspace'):
        L.call('rgda_upsample_pycda', *_args(ws_bytes=need - 1))
    # a row too wide for the row pass's LDS: the refusal of rgda_upsample_ce (16 classes: W <= 1008)
    with pytest.raises(ValueError, match='status -4'):
        L.call('rgda_upsample_pycda', *_args(c=16, h=64, w=64, H=1024, W=1024, b=1))


def test_python_surface_refuses_on_the_host():
    from regda_amd import ops
    from regda_amd.align import AlignStep
    from regda_amd.gast import PyramidCurriculumLoss
    from regda_amd.source import SourceStep
    for sizes in ((4, 12), (16, 4), (0, 4), (1,), (512,), (), (2, 4, 8, 16, 32, 64, 128), 8):
        with pytest.raises(ValueError):
            ops.pycda_sizes(sizes)
        with pytest.raises(ValueError):
            PyramidCurriculumLoss(sizes=sizes)
    assert ops.pycda_sizes([8, 16, 0]) == (8, 16, 0) and PyramidCurriculumLoss().sizes == (8, 16, 32, 64, 0)
    with pytest.raises(ValueError):
        PyramidCurriculumLoss(thresh=1.5)
    with pytest.raises(ValueError):
        PyramidCurriculumLoss(sizes=(4, 8), level_weight=(1.0,))
    with pytest.raises(RuntimeError, match='GPU only'):
        PyramidCurriculumLoss(sizes=(2, 0))(torch.zeros(1, 6, 4, 4), torch.zeros(1, 6, 8, 8))
    with pytest.raises(NotImplementedError, match='pycda_weight'):
        AlignStep(None, None, pycda_weight=0.5)
    with pytest.raises(NotImplementedError, match='pycda_weight'):
        SourceStep(None, pycda_weight=0.5)


# ------------------------------------------------------------------------------------------------- the restatement
@pytest.mark.parametrize('k', (0, 2, 4))
def test_closed_form_gradient_equals_autograd(k):
    """The kernels' form of the gradient (coefficients pushed down to the pixels) against autograd of the restated
    loss, in float64 at the label resolution."""
    d = pycda_ref.case(7, k)
    g = torch.Generator().manual_seed(k)
    z = 3.0 * torch.randn(pycda_ref.BATCH, 7, *d['hi'], generator=g, dtype=torch.float64)
    lw = [0.5 + 0.25 * i for i in range(len(d['sizes']))]
    _, _, (auto,) = pycda_ref.loss_and_grads([z], d['soft'], d['sizes'], level_weight=lw)
    closed = pycda_ref.closed_form_grad(z, d['soft'], d['sizes'], level_weight=lw)
    assert auto.abs().max() > 0
    torch.testing.assert_close(closed, auto, rtol=1e-9, atol=1e-12 * float(auto.abs().max()))


def test_a_finite_size_that_covers_the_image_is_the_image_level():
    d = pycda_ref.case(6, 2)        # 48 x 80
    big, _, gb = pycda_ref.loss_and_grads(d['p'], d['soft'], (2, 128))
    img, _, gi = pycda_ref.loss_and_grads(d['p'], d['soft'], (2, 0))
    torch.testing.assert_close(big, img, rtol=1e-14, atol=0)
    for a, b in zip(gb, gi):        # (the padded sum adds in another order)
        torch.testing.assert_close(a, b, rtol=1e-12, atol=1e-15)


def tie_soft(C=6, H=12, W=20, bump=False):
    """One image whose every 4 x 4 region sits exactly at the threshold 0.5 in class 0 (inactive: the comparison is
    strict); bump: one pixel of region (1, 2) is raised by 2^-24, which makes exactly that region active."""
    soft = torch.full((1, C, H, W), 0.5 / (C - 1))
    soft[:, 0] = 0.5
    if bump:
        soft[0, 0, 5, 9] = 0.5 + 2.0 ** -24
    return soft


def test_the_threshold_is_strict_and_exact_to_one_fixed_point_step():
    flat, bumped = tie_soft(), tie_soft(bump=True)
    assert float(bumped[0, 0, 5, 9]) > 0.5
    (_, a0, _, n0), = pycda_ref.targets(flat, (4,))
    (_, a1, _, n1), = pycda_ref.targets(bumped, (4,))
    assert n0 == 0 and not a0.any()
    assert n1 == 1 and a1.sum() == 1 and bool(a1[0, 0, 1, 2])
    p = pycda_ref.make_logits(1, 6, 3, 5, 3, heads=1)
    loss0, _, (g0,) = pycda_ref.loss_and_grads(p, flat, (4,))
    loss1, _, (g1,) = pycda_ref.loss_and_grads(p, bumped, (4,))
    assert not loss0.any() and not g0.any() and loss1[0] > 0 and g1.abs().max() > 0


def test_out_of_contract_values_are_clamped():
    s = torch.tensor([1.5, -0.1, float('nan'), 0.25, float('inf')])
    assert torch.equal(pycda_ref.clamp_soft(s), torch.tensor([1.0, 0.0, 0.0, 0.25, 1.0]))


def test_generated_cases_have_active_and_inactive_regions_at_every_level():
    image = set()
    for C in pycda_ref.CLASSES:
        for k in range(len(pycda_ref.CASE_SHAPES)):
            d = pycda_ref.case(C, k)
            soft = d['soft']
            assert soft.dtype == torch.float32 and soft.min() >= 0 and soft.max() <= 1 and torch.isfinite(soft).all()
            for s, (_, active, area, n) in zip(d['sizes'], pycda_ref.targets(soft, d['sizes'])):
                regions = active.shape[0] * active.shape[2] * active.shape[3]
                if s:
                    assert 0 < n < regions, (C, k, s, n, regions)
                else:
                    image.update((n > 0, n < regions))
                assert int(area.sum()) == soft.shape[2] * soft.shape[3]
    assert image == {True, False}
