"""CPU: the region-overlap term (Dice / Jaccard / Tversky).  The new entry points (rgda_upsample_overlap, its workspace)
are exported, replayable and refuse bad arguments before anything touches the GPU; the restatement
(tests/overlap_ref.py) is consistent with itself (closed-form gradient, the perfect prediction, Jaccard against Dice);
the generated labels hold what the GPU tests rely on (ignored pixels, an absent class, a class of one pixel); and the
Python surface refuses bad keywords on the host."""
import pytest
import torch

import overlap_ref

P = 4096        # a non-null pointer that is never dereferenced: every check here comes before a launch
NAN, INF = float('nan'), float('inf')


def test_new_entry_points_are_exported_and_replayable():
    from regda_amd import _lib, gast, ops
    from regda_amd.plan import MAX_ARGS
    L = _lib.lib()
    assert L.raw('rgda_abi_version')() == 10
    for name in ('rgda_upsample_overlap', 'rgda_upsample_overlap_workspace'):
        assert name in L.protos and name not in L.missing, name
    assert L.raw('rgda_plan_fn_id')(b'rgda_upsample_overlap') >= 0
    assert len(L.protos['rgda_upsample_overlap'][1]) <= MAX_ARGS
    assert callable(ops.upsample_overlap) and callable(ops.upsample_overlap_workspace)
    for name in ('TverskyLoss', 'DiceLoss', 'JaccardLoss'):
        assert callable(getattr(gast, name)), name
    assert issubclass(gast.DiceLoss, gast.TverskyLoss) and issubclass(gast.JaccardLoss, gast.TverskyLoss)


def _args(**kw):
    """A valid rgda_upsample_overlap call at 2 x 6 x 5 x 7 -> 33 x 45 (fake pointers), with overrides."""
    from regda_amd import _lib
    b, c, h, w, H, W = kw.pop('b', 2), kw.pop('c', 6), kw.pop('h', 5), kw.pop('w', 7), kw.pop('H', 33), kw.pop('W', 45)
    a = dict(heads=2, p1=P, p2=P + 4096, label=P, alpha=0.5, beta=0.5, gamma=1.0, smooth=0.0, weight=1.0, acc=0, loss=P,
             index=P, present=P, g1=P, g2=P, flag=None, b=b, c=c, h=h, w=w, H=H, W=W, ignore=-1, ws=P,
             ws_bytes=_lib.lib().size('rgda_upsample_overlap_workspace', b, c, h, w, H, W), stream=None)
    a.update(kw)
    return list(a.values())


def test_workspace_query():
    from regda_amd import _lib
    L = _lib.lib()
    need = L.size('rgda_upsample_overlap_workspace', 2, 6, 5, 7, 33, 45)
    # at least: the row partials (6 c floats and c counts per row) and the row-contracted gradient
    assert need >= 2 * 33 * (6 * 6 * 4 + 6 * 4) + 2 * 33 * 2 * 6 * 7 * 4
    for bad in ((0, 6, 5, 7, 33, 45), (2, 6, 0, 7, 33, 45), (2, 6, 5, 0, 33, 45), (2, 6, 5, 7, 0, 45), (2, 6, 5, 7, 33, 0),
                (2, 5, 5, 7, 33, 45), (2, 17, 5, 7, 33, 45), (-1, 6, 5, 7, 33, 45), (1 << 15, 6, 5, 7, 1 << 8, 1 << 8)):
        assert L.size('rgda_upsample_overlap_workspace', *bad) == 0, bad


def test_upsample_overlap_refuses_bad_arguments_before_the_gpu():
    from regda_amd import _lib
    L = _lib.lib()
    need = L.size('rgda_upsample_overlap_workspace', 2, 6, 5, 7, 33, 45)
    bad = [dict(p1=None), dict(p2=None), dict(label=None), dict(loss=None), dict(ws=None), dict(g1=None), dict(g2=None),
           dict(heads=0), dict(heads=3), dict(heads=1), dict(b=0), dict(h=0), dict(w=0), dict(H=0), dict(W=0),
           dict(gamma=0.5), dict(gamma=9.0), dict(gamma=NAN),
           dict(alpha=-0.1), dict(alpha=NAN), dict(alpha=INF), dict(beta=-0.1), dict(beta=NAN), dict(beta=INF),
           dict(smooth=-1.0), dict(smooth=NAN), dict(smooth=INF), dict(weight=-1.0), dict(weight=NAN), dict(weight=INF),
           dict(b=1 << 15, H=1 << 8, W=1 << 8, ws_bytes=1 << 40)]
    for kw in bad:
        with pytest.raises(ValueError):
            L.call('rgda_upsample_overlap', *_args(**kw))
    for c in (5, 17):        # class counts outside 6..16: unsupported
        with pytest.raises(ValueError, match='status -4'):
            L.call('rgda_upsample_overlap', *_args(c=c, ws_bytes=1 << 30))
    with pytest.raises(_lib.RgdaError, match='workspace'):
        L.call('rgda_upsample_overlap', *_args(ws_bytes=need - 1))
    # a row too wide for the row pass's LDS: the refusal of rgda_upsample_ce (16 classes: W <= 1008)
    with pytest.raises(ValueError, match='status -4'):
        L.call('rgda_upsample_overlap', *_args(c=16, h=64, w=64, H=1024, W=1024, b=1))


def test_python_surface_refuses_on_the_host():
    from regda_amd import ops
    from regda_amd.align import AlignStep
    from regda_amd.gast import DiceLoss, JaccardLoss, TverskyLoss
    from regda_amd.source import SourceStep
    from regda_amd.ssl import SSLStep
    for kw in (dict(alpha=-1.0), dict(beta=NAN), dict(gamma=0.5), dict(gamma=9), dict(smooth=-0.5), dict(alpha=INF),
               dict(alpha='x')):
        with pytest.raises(ValueError):
            ops.overlap_params(**kw)
        with pytest.raises(ValueError):
            TverskyLoss(**dict(dict(alpha=0.5, beta=0.5), **kw))
    assert ops.overlap_params() == (0.5, 0.5, 1.0, 0.0)
    d, j, t = DiceLoss(), JaccardLoss(gamma=2), TverskyLoss(0.3, 0.7, smooth=1)
    assert (d.alpha, d.beta, d.gamma, d.smooth, d.ignore_label) == (0.5, 0.5, 1.0, 0.0, -1)
    assert (j.alpha, j.beta, j.gamma) == (1.0, 1.0, 2.0) and (t.alpha, t.beta, t.smooth) == (0.3, 0.7, 1.0)
    assert d.index is None and d.present is None and d.flag_value() == 0
    with pytest.raises(ValueError):
        DiceLoss(gamma=0.0)
    with pytest.raises(RuntimeError, match='GPU only'):
        DiceLoss()(torch.zeros(1, 6, 4, 4), torch.zeros(1, 8, 8, dtype=torch.int64))
    with pytest.raises(ValueError):
        DiceLoss()([torch.zeros(1, 6, 4, 4)] * 3, torch.zeros(1, 8, 8, dtype=torch.int64))
    # the steps: refused before the model (None here) is touched
    with pytest.raises(NotImplementedError, match='overlap_weight_t'):
        AlignStep(None, None, overlap_weight_t=0.5)
    with pytest.raises(NotImplementedError, match='overlap_weight_t'):
        SourceStep(None, overlap_weight_t=0.5)
    for make in (lambda **kw: SourceStep(None, **kw), lambda **kw: AlignStep(None, None, **kw),
                 lambda **kw: SSLStep(None, None, **kw)):
        for kw in (dict(overlap_weight_s=-1.0), dict(overlap_weight_s=NAN), dict(overlap_weight_s=INF),
                   dict(overlap_weight_s=1.0, overlap=dict(gamma=0.5)), dict(overlap=dict(alpha=-1.0)),
                   dict(overlap=dict(delta=1.0))):
            with pytest.raises(ValueError):
                make(**kw)
    for kw in (dict(overlap_weight_t=-0.5), dict(overlap_weight_t=NAN)):
        with pytest.raises(ValueError):
            SSLStep(None, None, **kw)


# ------------------------------------------------------------------------------------------------- the restatement
@pytest.mark.parametrize('variant', sorted(overlap_ref.VARIANTS))
@pytest.mark.parametrize('k', (0, 2, 4))
def test_closed_form_gradient_equals_autograd(k, variant):
    """The kernels' form of the gradient (two coefficients per class, pushed through the softmax) against autograd of
    the restated loss, in float64 at the label resolution."""
    d = overlap_ref.case(7, k)
    g = torch.Generator().manual_seed(k)
    z = 3.0 * torch.randn(overlap_ref.BATCH, 7, *d['hi'], generator=g, dtype=torch.float64)
    prm = overlap_ref.VARIANTS[variant]
    _, _, _, (auto,) = overlap_ref.loss_and_grads([z], d['label'], *prm)
    closed = overlap_ref.closed_form_grad(z, d['label'], *prm)
    assert auto.abs().max() > 0
    torch.testing.assert_close(closed, auto, rtol=1e-9, atol=1e-12 * float(auto.abs().max()))
    assert not closed[(d['label'] == -1)[:, None].expand_as(closed)].any()       # ignored pixels carry no gradient


def test_dice_of_a_perfect_prediction_tends_to_zero():
    d = overlap_ref.case(6, 2)
    label = d['label']
    ok = label >= 0
    onehot = torch.nn.functional.one_hot(label.clamp(min=0), 6).permute(0, 3, 1, 2).double()
    last = None
    for scale in (5.0, 20.0, 40.0):
        total, index, present, _ = overlap_ref.loss_and_grads([scale * onehot], label)
        assert last is None or total < last
        last = total
    assert float(last) < 1e-6
    assert torch.all(index[0][present > 0] > 1 - 1e-6) and not index[0][present == 0].any()
    assert int(present.sum()) == int(ok.sum())


def test_jaccard_is_dice_over_two_minus_dice():
    """Per class at smooth = 0: J = TP / (TP + FP + FN) and D = 2 TP / (2 TP + FP + FN), so J = D / (2 - D) up to the
    1e-7 in the denominators."""
    for C in overlap_ref.CLASSES:
        d = overlap_ref.case(C, 0)
        _, dice, present, _ = overlap_ref.loss_and_grads(d['p'], d['label'], 0.5, 0.5)
        _, jacc, _, _ = overlap_ref.loss_and_grads(d['p'], d['label'], 1.0, 1.0)
        on = present > 0
        torch.testing.assert_close(jacc[:, on], (dice / (2 - dice))[:, on], rtol=1e-6, atol=1e-7)
        assert not jacc[:, ~on].any() and not dice[:, ~on].any()


def test_everything_ignored_is_exactly_zero():
    d = overlap_ref.case(6, 0)
    total, index, present, grads = overlap_ref.loss_and_grads(d['p'], torch.full_like(d['label'], -1), 0.3, 0.7, 1.5, 1.0)
    assert float(total) == 0.0 and not index.any() and not present.any() and not any(g.any() for g in grads)


def test_generated_labels_hold_ignored_pixels_an_absent_class_and_a_single_pixel_class():
    for C in overlap_ref.CLASSES:
        for k in range(len(overlap_ref.CASE_SHAPES)):
            d = overlap_ref.case(C, k)
            label = d['label']
            assert label.dtype == torch.int64 and tuple(label.shape) == (overlap_ref.BATCH, *d['hi'])
            assert label.min() == -1 and label.max() < C
            counts = torch.bincount(label[label >= 0], minlength=C)
            assert (label == -1).sum() > 0 and (counts == 0).any() and (counts == 1).any(), (C, k, counts)
            assert (counts > 1).sum() >= 2, (C, k, counts)
