"""CPU: the IAST restatement (tests/iast_ref.py) against the reference's own entropyloss / kldloss / ias_thresh /
generate_pseudo (tests/golden/iast.npz), and the new entry points (rgda_upsample_reg, rgda_iast_*): exported, replayable,
and refusing bad arguments before anything touches the GPU."""
import numpy as np
import pytest
import torch

import iast_ref

CLASSES = (6, 7, 16)
KINDS = ('bin', 'frac', 'zero', 'neg')
ENTRY_POINTS = ('rgda_upsample_reg', 'rgda_iast_hist', 'rgda_iast_percentile', 'rgda_iast_label')
P = 4096        # a non-null pointer that is never dereferenced: every check here comes before a launch


@pytest.mark.parametrize('C', CLASSES)
@pytest.mark.parametrize('kind', KINDS)
def test_restated_regularisers_match_the_reference(gold, C, kind):
    g = gold('iast.npz')
    z = g[f'reg/c{C}/logits']
    w = g[f'reg/c{C}/w_{kind}']
    for name, fn in (('ent', iast_ref.entropyloss), ('kld', iast_ref.kldloss)):
        for bits, dt, tol in ((32, torch.float32, 1e-6), (64, torch.float64, 1e-13)):
            x = torch.from_numpy(z).to(dt).requires_grad_(True)
            loss = fn(x, torch.from_numpy(w).to(dt))
            loss.backward()
            np.testing.assert_allclose(loss.detach().numpy(), g[f'reg/c{C}/{kind}/{name}_loss{bits}'], rtol=tol, equal_nan=True)
            np.testing.assert_allclose(x.grad.numpy(), g[f'reg/c{C}/{kind}/{name}_grad{bits}'], rtol=tol * 10, atol=tol * 1e-2,
                                       equal_nan=True)
    if kind == 'zero':      # the reference's 0 / 0
        assert np.isnan(g[f'reg/c{C}/{kind}/ent_loss32']) and np.isnan(g[f'reg/c{C}/{kind}/kld_grad32']).all()


def test_reg_contract_of_the_restatement(gold):
    """reg(): derived masks, the mean over the heads and the zero form of an empty region."""
    g = gold('iast.npz')
    z = torch.from_numpy(g['reg/c6/logits']).float()
    lab = torch.full((2, 9, 11), -1, dtype=torch.int64)
    we, wk = iast_ref.derived_weights(lab)
    assert float(we.sum()) == lab.numel() and float(wk.sum()) == 0
    ent, kld, obj = iast_ref.reg([z, z * 0.5], (9, 11), we, wk, 2.0, 3.0, empty_is_zero=True)
    assert float(kld) == 0.0 and float(obj) == pytest.approx(2.0 * float(ent))
    e1, e2 = iast_ref.entropyloss(z, we), iast_ref.entropyloss(z * 0.5, we)
    assert float(ent) == pytest.approx(float(e1 + e2) / 2, rel=1e-6)
    assert torch.isnan(iast_ref.reg([z], (9, 11), we, wk)[1])


@pytest.mark.parametrize('C', (6, 16))
def test_restated_selector_matches_the_reference_loop(gold, C):
    g = gold('iast.npz')
    sel = iast_ref.Selector(C, float(g['sel/alpha']), float(g['sel/beta']), float(g['sel/gamma']))
    for k in range(3):
        probs = g[f'sel/c{C}/probs'][k]
        prepend = sel.cls_thresh.copy()
        lab = sel.update(probs)
        assert np.array_equal(sel.tmp, g[f'sel/c{C}/tmp'][k]) and sel.tmp.dtype == np.float32
        assert np.array_equal(sel.cls_thresh, g[f'sel/c{C}/thresh'][k]) and sel.cls_thresh.dtype == np.float64
        assert np.array_equal(lab, g[f'sel/c{C}/labels'][k])
        # the histogram form of the same percentile: what the kernels compute
        arg, maxp, h = iast_ref.hist(probs)
        assert int(h.sum()) == arg.size and h.shape == (C, iast_ref.BINS)
        q = np.array([np.true_divide(100 * (1 - sel.alpha * prepend[c] ** sel.gamma), 100) for c in range(C)])
        got = np.array([iast_ref.percentile_from_hist(h[c], prepend[c], q[c]) for c in range(C)])
        assert np.array_equal(got, sel.tmp)
        assert np.array_equal(iast_ref.label_from(arg, maxp, sel.cls_thresh), lab)
    assert not np.array_equal(g[f'sel/c{C}/thresh'][0], g[f'sel/c{C}/thresh'][2])      # the EMA state matters


@pytest.mark.parametrize('kind', ('softmax', 'confident', 'fp16_ties', 'missing_class', 'class_ties'))
def test_selector_inputs_hold_what_they_are_named_for(kind):
    p = iast_ref.selector_inputs(kind, 2, 6, 7, 13, seed=3)
    assert p.dtype == np.float32 and p.shape == (2, 6, 7, 13) and p.min() >= 0 and p.max() <= 1 and np.isfinite(p).all()
    arg, maxp, h = iast_ref.hist(p)
    if kind == 'confident':
        assert (maxp == 1).all() and h[:, 0x3C00].sum() == arg.size
    if kind == 'fp16_ties':       # exact half-way points between two fp16 values are there, and round to even
        b = maxp.astype(np.float16).view(np.uint16)
        f = b.view(np.float16).astype(np.float32)
        up = (b + 1).astype(np.uint16).view(np.float16).astype(np.float32)
        dn = (b - 1).astype(np.uint16).view(np.float16).astype(np.float32)
        tie = ((maxp > f) & (up - maxp == maxp - f)) | ((maxp < f) & (maxp - dn == f - maxp))
        assert tie.sum() > 10 and (b[tie] % 2 == 0).all() and (maxp != f).mean() > 0.9
    if kind == 'missing_class':
        assert h[1].sum() == 0 and (arg != 1).all()
    if kind == 'class_ties':
        assert (np.sort(p, axis=1)[:, -1] == np.sort(p, axis=1)[:, -2]).mean() > 0.5 and (arg[:, 0] == 0).all()


def test_new_entry_points_are_exported_and_replayable():
    from regda_amd import _lib
    from regda_amd.plan import MAX_ARGS
    L = _lib.lib()
    assert L.raw('rgda_abi_version')() == 10
    for name in ENTRY_POINTS + ('rgda_upsample_reg_workspace', 'rgda_iast_workspace'):
        assert name in L.protos and name not in L.missing, name
    for name in ENTRY_POINTS:
        assert L.raw('rgda_plan_fn_id')(name.encode()) >= 0, name
        assert len(L.protos[name][1]) <= MAX_ARGS
    from regda_amd.utils import tools
    for fn in ('entropyloss', 'kldloss', 'IASTSelector', 'generate_pseudo'):
        assert callable(getattr(tools, fn))


def _reg_args(**kw):
    """A valid rgda_upsample_reg call at 2 x 6 x 5 x 7 -> 33 x 45 (fake pointers), with overrides."""
    from regda_amd import _lib
    b, c, h, w, H, W = 2, kw.pop('c', 6), 5, 7, 33, 45
    a = dict(heads=2, p1=P, p2=P + 4096, label=P, w_ent=None, w_kld=None, terms=3, le=1.0, lk=1.0, acc=0, ez=0, loss=P, g1=P,
             g2=P, b=b, c=c, h=h, w=w, H=H, W=W, ig=-1, ws=P,
             ws_bytes=_lib.lib().size('rgda_upsample_reg_workspace', b, c, h, w, H, W), stream=None)
    a.update(kw)
    return list(a.values())


def test_upsample_reg_refuses_bad_arguments_before_the_gpu():
    from regda_amd import _lib
    L = _lib.lib()
    need = L.size('rgda_upsample_reg_workspace', 2, 6, 5, 7, 33, 45)
    assert need >= 512 + 2 * 33 * 4 * 4 + 2 * 33 * 2 * 6 * 7 * 4
    assert L.size('rgda_upsample_reg_workspace', 0, 6, 5, 7, 33, 45) == 0
    bad = [dict(p1=None), dict(p2=None), dict(loss=None), dict(ws=None), dict(g2=None), dict(g1=None), dict(label=None),
           dict(heads=1), dict(heads=3), dict(terms=0), dict(terms=4), dict(b=0), dict(W=0), dict(b=1 << 16, H=1 << 8, W=1 << 7)]
    for kw in bad:
        with pytest.raises(ValueError):
            L.call('rgda_upsample_reg', *_reg_args(**kw))
    for c in (5, 17):        # class counts outside 6..16: unsupported
        with pytest.raises(ValueError, match='status -4'):
            L.call('rgda_upsample_reg', *_reg_args(c=c))
    with pytest.raises(_lib.RgdaError, match='workspace'):
        L.call('rgda_upsample_reg', *_reg_args(ws_bytes=need - 1))
    # a row too wide for the row pass's LDS: the refusal of rgda_upsample_ce (16 classes: W <= 1008)
    wide = dict(c=16, h=64, w=64, H=1024, W=1024, b=1)
    wide['ws_bytes'] = L.size('rgda_upsample_reg_workspace', 1, 16, 64, 64, 1024, 1024)
    with pytest.raises(ValueError, match='status -4'):
        L.call('rgda_upsample_reg', *_reg_args(**wide))
    # a label is not needed when both maps are given -- but then everything else is still checked
    with pytest.raises(ValueError):
        L.call('rgda_upsample_reg', *_reg_args(label=None, w_ent=P, w_kld=P, heads=1))


def test_iast_stages_refuse_bad_arguments_before_the_gpu():
    from regda_amd import _lib
    L = _lib.lib()
    n, c, H, W = 2, 6, 7, 13
    need = L.size('rgda_iast_workspace', n, c, H, W)
    a256 = lambda x: (x + 255) & ~255
    assert need == a256(c * 0x7C01 * 4) + a256(n * H * W * 4) + a256(n * H * W)
    assert L.size('rgda_iast_workspace', n, 5, H, W) == 0 and L.size('rgda_iast_workspace', 0, c, H, W) == 0
    for args in ((None, n, c, H, W, P, need, None), (P, n, c, H, W, None, need, None), (P, 0, c, H, W, P, need, None),
                 (P, n, 5, H, W, P, need, None), (P, n, 17, H, W, P, need, None), (P, 1 << 16, c, 1 << 8, 1 << 7, P, need, None)):
        with pytest.raises(ValueError):
            L.call('rgda_iast_hist', *args)
    with pytest.raises(_lib.RgdaError, match='workspace'):
        L.call('rgda_iast_hist', P, n, c, H, W, P, need - 1, None)
    for args in ((None, P, P, c, P, need, None), (P, None, P, c, P, need, None), (P, P, None, c, P, need, None),
                 (P, P, P, c, None, need, None), (P, P, P, 5, P, need, None)):
        with pytest.raises(ValueError):
            L.call('rgda_iast_percentile', *args)
    with pytest.raises(_lib.RgdaError, match='workspace'):
        L.call('rgda_iast_percentile', P, P, P, c, P, c * 0x7C01 * 4 - 1, None)
    for args in ((None, P, n, c, H, W, P, need, None), (P, None, n, c, H, W, P, need, None), (P, P, n, c, H, W, None, need, None),
                 (P, P, n, 5, H, W, P, need, None), (P, P, n, c, 0, W, P, need, None)):
        with pytest.raises(ValueError):
            L.call('rgda_iast_label', *args)
    with pytest.raises(_lib.RgdaError, match='workspace'):
        L.call('rgda_iast_label', P, P, n, c, H, W, P, need - 1, None)


def test_python_surface_refuses_on_the_host():
    from regda_amd.align import AlignStep
    from regda_amd.utils.tools import IASTSelector, entropyloss, kldloss
    z = torch.zeros(1, 6, 4, 4)
    with pytest.raises(TypeError):
        entropyloss(z)
    with pytest.raises(TypeError):
        kldloss(z, None)
    with pytest.raises(RuntimeError, match='GPU only'):
        entropyloss(z, torch.ones(1, 1, 4, 4))
    with pytest.raises(ValueError):
        IASTSelector(5, 0.2, 0.9, 8.0)
    sel = IASTSelector(6, 0.2, 0.9, 8.0)
    assert sel.cls_thresh.dtype == np.float64 and (sel.cls_thresh == 0.9).all()
    q = sel.quantiles()
    assert q.dtype == np.float64 and q[0] == (100 * (1 - 0.2 * np.float64(0.9) ** 8.0)) / 100
    with pytest.raises(ValueError, match='Percentiles'):       # numpy's own refusal of a percentile outside [0, 100]
        IASTSelector(6, 3.0, 0.9, 1.0).quantiles()
    with pytest.raises(NotImplementedError):
        AlignStep(None, None, ent_weight=0.1)
