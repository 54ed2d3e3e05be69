"""CPU: the pseudo-label analysis restatement (tests/analysis_ref.py) against the reference's own loop
(tests/golden/pseudo_analysis.npz), the exact fixed-point difficulty, and the new entry points (rgda_pseudo_analysis,
rgda_pseudo_analysis_fold): exported, replayable, and refusing bad arguments before anything touches the GPU.

Bounds: the integer lists are equal.  acc_list rtol 5e-7: counts below 2^24 are exact in f32, so the reference's value is
the same quotient after two f32 roundings.  diffi_list rtol 1e-5: the reference's f32 sum of up to 3 x 10^4 values carries
about log2(N) * 6e-8."""
import numpy as np
import pytest

import analysis_ref as ar

SEED = 20               # tests/golden/make_analysis_goldens.py
P = 4096                # a non-null, aligned pointer that is never dereferenced: every check here comes before a launch
CASES = [(kind,) + s for s in ar.shapes() for kind in ar.KINDS]


@pytest.mark.parametrize('kind,b,C,H,W', CASES)
def test_restatement_matches_the_reference_loop(gold, kind, b, C, H, W):
    g = gold('pseudo_analysis.npz')
    soft, gt = ar.inputs(kind, b, C, H, W, SEED)
    got = ar.run(soft, gt, per_image=True)
    want = {k: g[f'{kind}/c{C}/{H}x{W}/{k}'] for k in ('acc_list', 'diffi_list', 'cnt_true_list', 'cnt_used_list')}
    assert np.array_equal(got['cnt_true_list'], want['cnt_true_list'])
    assert np.array_equal(got['cnt_used_list'], want['cnt_used_list'])
    np.testing.assert_allclose(got['acc_list'], want['acc_list'], rtol=5e-7)
    np.testing.assert_allclose(got['diffi_list'], want['diffi_list'], rtol=1e-5)
    assert got['images'] == b and np.array_equal(got['used'].sum(1), got['cnt_used_list'])
    if kind == 'zeros':         # the NaN row is there, and it is counted in all bins
        t = ar.analyse(soft, gt)
        assert t['inbin'][:, ar.R].min() > 0 and got['nan_pixels'] == t['inbin'][:, ar.R].sum()
        assert got['cnt_used_list'].min() >= t['used'][:, ar.R].sum() > 0
    if kind == 'uniform':       # at or above the last edge: no bin, and no label used
        assert got['in_bin'].sum() == 0 and got['nan_pixels'] == 0 and got['cnt_used_list'].sum() == 0
        assert not np.any(got['diffi_list']) and not np.any(got['acc_list'])
    if kind == 'gt_argmax':
        assert np.array_equal(got['cnt_true_list'], got['cnt_used_list']) and got['cnt_used_list'].sum() > 0
    if kind == 'gt_ignore':
        assert got['cnt_true_list'].sum() == 0 and got['cnt_used_list'].sum() > 0


def test_batch_fold_equals_the_per_image_fold():
    soft, gt = ar.inputs('softmax', 3, 6, 96, 100, SEED)
    a, b = ar.run(soft, gt), ar.run(soft, gt, per_image=True)
    for k in a:
        assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), k


@pytest.mark.parametrize('C', ar.CLASSES)
def test_edge_tables_partition_the_entropy_range(C):
    _, lo, hi = ar.edges(C)
    assert lo.dtype == hi.dtype == np.float32 and lo[0] == 0 and np.array_equal(hi[:-1], lo[1:])
    from regda_amd.gast.pseudo_generation import entropy_bin_edges
    x, lo2, hi2 = entropy_bin_edges(C, ar.R)
    assert np.array_equal(lo, lo2) and np.array_equal(hi, hi2) and x == ar.edges(C)[0]
    # a uniform pixel's f32 entropy is at or above the last edge
    e = ar.entropy64(np.full((1, C, 1, 1), np.float32(1) / np.float32(C), np.float32)).astype(np.float32)
    assert e[0, 0, 0] >= hi[-1]


@pytest.mark.parametrize('kind,b,C,H,W', CASES)
def test_every_difficulty_is_a_multiple_of_2_to_the_minus_24(kind, b, C, H, W):
    soft, gt = ar.inputs(kind, b, C, H, W, SEED)
    d = ar.difficulty(soft, gt).astype(np.float64) * 2.0 ** 24
    assert d.min() >= 0 and d.max() <= 2 ** 24 and np.array_equal(d, np.floor(d))


def test_inputs_hold_what_they_are_named_for():
    for C in ar.CLASSES:
        soft, gt = ar.inputs('zeros', 2, C, 33, 45, SEED)
        assert (soft == 0).any() and ((soft == 1).sum(1) == 1).any() and np.isnan(ar.entropy64(soft)).mean() > 0.3
        soft, gt = ar.inputs('confident', 2, C, 33, 45, SEED)
        assert (soft > 0).all() and (soft.max(1) >= 0.95).all()
        soft, gt = ar.inputs('gt_ignore', 2, C, 33, 45, SEED)
        assert (gt == -1).all()
        soft, gt = ar.inputs('softmax', 2, C, 33, 45, SEED)
        assert (gt == -1).any() and gt.max() == C - 1 and soft.dtype == np.float32 and gt.dtype == np.int64
        assert np.array_equal(soft, ar.inputs('softmax', 2, C, 33, 45, SEED)[0])


def test_new_entry_points_are_exported_and_replayable():
    from regda_amd import _lib
    from regda_amd.plan import MAX_ARGS
    L = _lib.lib()
    assert L.raw('rgda_abi_version')() == 10
    for name in ('rgda_pseudo_analysis', 'rgda_pseudo_analysis_fold', 'rgda_pseudo_analysis_workspace',
                 'rgda_pseudo_analysis_fold_workspace'):
        assert name in L.protos and name not in L.missing, name
    for name in ('rgda_pseudo_analysis', 'rgda_pseudo_analysis_fold'):
        assert L.raw('rgda_plan_fn_id')(name.encode()) >= 0, name
        assert len(L.protos[name][1]) <= MAX_ARGS


def _args(**kw):
    """A valid rgda_pseudo_analysis call at 2 x 6 x 33 x 45, 100 bins (fake pointers), with overrides."""
    from regda_amd import _lib
    a = dict(soft=P, gt=P, lo=P, hi=P, b=2, c=6, H=33, W=45, R=100, top=0.8, low=0.6, ig=-1, tables=P, tables_bytes=None,
             stream=None)
    a.update(kw)
    if a['tables_bytes'] is None:
        a['tables_bytes'] = max(_lib.lib().size('rgda_pseudo_analysis_workspace', a['b'], a['c'], a['R']), 1 << 20)
    return list(a.values())


def test_analysis_refuses_bad_arguments_before_the_gpu():
    from regda_amd import _lib
    L = _lib.lib()
    need = L.size('rgda_pseudo_analysis_workspace', 2, 6, 100)
    assert need == (2 * 101 * (2 * 6 + 2) * 8 + 8 + 2 * 6 * 4 + 15) // 16 * 16
    for bad in ((0, 6, 100), (2, 5, 100), (2, 17, 100), (2, 6, 0), (2, 6, 257)):
        assert L.size('rgda_pseudo_analysis_workspace', *bad) == 0
    for kw in (dict(soft=None), dict(gt=None), dict(lo=None), dict(hi=None), dict(tables=None), dict(b=0), dict(H=0), dict(W=0),
               dict(R=0), dict(R=257), dict(b=1 << 16, H=1 << 8, W=1 << 7), dict(soft=P + 2), dict(gt=P + 4), dict(tables=P + 4),
               dict(b=1, H=(1 << 31) - 1, W=1),         # below 2^31, but the passes' int steps would overflow
               dict(b=65535 // 6 + 1, H=1, W=1)):       # b * c beyond a grid's y extent
        with pytest.raises(ValueError):
            L.call('rgda_pseudo_analysis', *_args(**kw))
    for c in (5, 17):
        with pytest.raises(ValueError, match='status -4'):
            L.call('rgda_pseudo_analysis', *_args(c=c))
    with pytest.raises(_lib.RgdaError, match='workspace'):
        L.call('rgda_pseudo_analysis', *_args(tables_bytes=need - 1))


def test_fold_refuses_bad_arguments_before_the_gpu():
    from regda_amd import _lib
    L = _lib.lib()
    tb, sb = L.size('rgda_pseudo_analysis_workspace', 2, 6, 100), L.size('rgda_pseudo_analysis_fold_workspace', 6, 100)
    assert sb == (101 * 14 * 8 + 2 * 100 * 8 + 8 + 2 * 100 * 4 + 4 + 7) // 8 * 8
    assert L.size('rgda_pseudo_analysis_fold_workspace', 5, 100) == 0 and L.size('rgda_pseudo_analysis_fold_workspace', 6, 257) == 0
    for args in ((None, tb, 2, 6, 100, P, sb, None), (P, tb, 2, 6, 100, None, sb, None), (P, tb, 0, 6, 100, P, sb, None),
                 (P, tb, 2, 6, 0, P, sb, None), (P, tb, 2, 6, 257, P, sb, None), (P + 4, tb, 2, 6, 100, P, sb, None)):
        with pytest.raises(ValueError):
            L.call('rgda_pseudo_analysis_fold', *args)
    for c in (5, 17):
        with pytest.raises(ValueError, match='status -4'):
            L.call('rgda_pseudo_analysis_fold', P, tb, 2, c, 100, P, sb, None)
    for args in ((P, tb - 1, 2, 6, 100, P, sb, None), (P, tb, 2, 6, 100, P, sb - 1, None)):
        with pytest.raises(_lib.RgdaError, match='workspace'):
            L.call('rgda_pseudo_analysis_fold', *args)


def test_python_surface_refuses_on_the_host(tmp_path):
    import torch
    from regda_amd.gast.pseudo_generation import PseudoLabelAnalysis, analysis_pseudo_labels, range_static
    for c in (5, 17):
        with pytest.raises(ValueError):
            PseudoLabelAnalysis(c)
    with pytest.raises(ValueError):
        PseudoLabelAnalysis(6, range_cnt=257)
    a = PseudoLabelAnalysis(7, range_cnt=50)
    with pytest.raises(ValueError):
        a.update(torch.zeros(1, 6, 4, 4), torch.zeros(1, 4, 4, dtype=torch.int64))
    with pytest.raises(RuntimeError, match='GPU only'):
        a.update(torch.zeros(1, 7, 4, 4), torch.zeros(1, 4, 4, dtype=torch.int64))
    s = a.summary()         # nothing seen yet: all zero, no device needed
    assert s['images'] == 0 and len(s['x']) == 50 and s['used'].shape == (50, 7) and not np.any(s['acc_list'])
    sd = a.state_dict()
    PseudoLabelAnalysis(7, range_cnt=50).load_state_dict(sd)
    with pytest.raises(ValueError):
        PseudoLabelAnalysis(7, range_cnt=60).load_state_dict(sd)
    from regda_amd.gast.pseudo_generation import gener_target_pseudo
    with pytest.raises(TypeError, match='PseudoLabelAnalysis'):      # a `scales` tuple that landed on analysis= by position
        gener_target_pseudo(None, None, [], str(tmp_path / 'p'), True, False, (8, 8), -1, None, (1.0, 1.5))
    (tmp_path / 'a.png').write_bytes(b'')
    with pytest.raises(AssertionError):     # one label, no soft label
        analysis_pseudo_labels(str(tmp_path), str(tmp_path))
    # range_static is plain torch: one bin of one image against the reference's own call
    e = torch.tensor([[0.05, 0.2, float('nan'), 0.07]])
    d = torch.tensor([[0.5, 0.25, 1.0, 0.125]])
    ct, cu, acc, diffi = range_static(e, d, torch.tensor([[1, 2, 3, 6]]), torch.tensor([[1, 2, 0, -1]]), 0.0, 0.1, 6)
    assert int(ct) == 1 and int(cu) == 2 and float(acc) == pytest.approx(0.5) and float(diffi) == pytest.approx(1.625 / 2)


def test_range_static_matches_the_reference_on_one_bin(gold):
    import math
    import torch
    from regda_amd.gast.pseudo_generation import range_static
    kind, C, H, W, img, i = 'softmax', 6, 33, 45, 0, 7          # make_analysis_goldens.ONE_BIN
    soft, gt = ar.inputs(kind, 2, C, H, W, SEED)
    s, g = torch.from_numpy(soft[img:img + 1]), torch.from_numpy(gt[img:img + 1])
    from oracle import labels as olab
    pseudo = torch.from_numpy(olab.pseudo_selection(soft[img:img + 1], 0.8, 0.6, -1))
    pseudo[pseudo == -1] = C
    entropy = torch.sum(-s * torch.log(s), dim=1)
    diff = torch.from_numpy(ar.difficulty(soft[img:img + 1], gt[img:img + 1]))
    step = math.log(C) / 100
    got = [float(r) for r in range_static(entropy, diff, pseudo, g, 1.0 * i * step, 1.0 * i * step + step, C)]
    want = gold('pseudo_analysis.npz')['one_bin/result']
    assert got[0] == want[0] and got[1] == want[1] and want[1] > 0
    np.testing.assert_allclose(got[2:], want[2:], rtol=1e-6)
