"""GPU: every label-path kernel of regda_amd/csrc/label_kernels.hip on every case of tests/label_cases.py, per element
against the plain references there.  Integer outputs and flag words must match bit for bit; float outputs (label_refine*,
teacher_probs, the prototype sums and the prototypes) are bounded per element by tests/golden/label_tolerances.json, which
tests/golden/derive_label_tolerances.py derives on the CPU from the fp32 oracle's own deviation from the fp64 reference
(never from a kernel's output).  tests/test_label_cases_cpu.py checks, without a GPU, that each case reaches the path it
names and that the references agree with the oracles."""
import json
import os

import numpy as np
import pytest
import torch

import label_cases as L

pytestmark = pytest.mark.gpu
TOL = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'label_tolerances.json')))['bounds']


@pytest.fixture(scope='module')
def ops():
    from regda_amd import ops
    return ops


def cu(a):
    return None if a is None else torch.as_tensor(a).contiguous().cuda()


def _check(name, got, ref, bound):
    d = (got.detach().cpu().double() - torch.as_tensor(ref).double()).abs()
    n = int((~(d <= bound)).sum())
    print('%s: max |diff| %.3e, bound %.3e' % (name, float(d.max()), bound))
    assert n == 0, '%s: %d of %d off; max |diff| %.3e, bound %.3e' % (name, n, d.numel(), float(d.max()), bound)


def _word(buf, byte_offset):
    return int(buf[byte_offset:byte_offset + 4].view(torch.int32).item())


def _ids(cases):
    return [c.name for c in cases]


# ---------------------------------------------------------------- pseudo_select
def _pseudo_abi(ops, soft, cm, top=0.8, low=0.6, ignore=-1):
    """rgda_pseudo_select with a workspace of the test's own -> (labels, flag word, classmax)."""
    from regda_amd._lib import lib
    b, c, h, w = soft.shape
    ws = torch.zeros(lib().size('rgda_pseudo_select_workspace', b, c), dtype=torch.uint8, device='cuda')
    if cm is not None:
        ws[:b * c * 4].view(torch.float32).copy_(cu(cm).reshape(-1))
    out = torch.empty((b, h, w), dtype=torch.int64, device='cuda')
    lib().call('rgda_pseudo_select', soft.data_ptr(), out.data_ptr(), b, c, h * w, top, low, ignore, int(cm is not None),
               ws.data_ptr(), ws.numel(), ops._stream())
    return out.cpu().numpy(), _word(ws, b * c * 4), ws[:b * c * 4].view(torch.float32).cpu().numpy().reshape(b, c), ws


@pytest.mark.parametrize('case', L.PSEUDO_CASES, ids=_ids(L.PSEUDO_CASES))
def test_pseudo_select(ops, case):
    soft, cm = L.pseudo_inputs(case)
    ref, flag, refmax = L.pseudo_ref(soft, L.EDGE_TOP, L.EDGE_LOW, -1, cm)
    out, got_flag, got_max, ws = _pseudo_abi(ops, cu(soft), cm)
    assert np.array_equal(out, ref) and got_flag == flag == 0
    assert np.array_equal(got_max, refmax)                      # a maximum has one answer (and the given ones stay)
    via = ops.pseudo_select(cu(soft), L.EDGE_TOP, L.EDGE_LOW, -1, classmax_ws=ws if cm is not None else None)
    assert np.array_equal(via.cpu().numpy(), ref)


@pytest.mark.parametrize('case', L.PSEUDO_FLAG_CASES, ids=_ids(L.PSEUDO_FLAG_CASES))
def test_pseudo_select_range_flag(ops, case):
    """One value just above 1, just below 0, or NaN in the last chunk of either route sets the flag (the reference's
    assert fails on each).  The NaN cases failed before the range check of pseudo_max_kernel looked for NaN itself:
    fmaxf / fminf drop it."""
    soft, _ = L.pseudo_inputs(case)
    assert L.pseudo_ref(soft)[1] == 1
    assert _pseudo_abi(ops, cu(soft), None)[1] == 1
    with pytest.raises(AssertionError):
        ops.pseudo_select(cu(soft), 0.8, 0.6, -1)


# ---------------------------------------------------------------- LRH, the fused pass
def _lrh_flag_offset(c):
    return (c.b * c.R * c.C + c.b * c.R) * 4


@pytest.mark.parametrize('case', L.LRH_CASES, ids=_ids(L.LRH_CASES))
def test_lrh(ops, case):
    from regda_amd._lib import lib
    lab, reg = L.lrh_inputs(case)
    ref, flag = L.lrh_ref(lab, reg, case.percent, case.C, case.ignore, case.R)
    ws = torch.empty(lib().size('rgda_lrh_workspace', case.b, case.R, case.C), dtype=torch.uint8, device='cuda')
    out = ops.lrh(cu(lab), cu(reg), case.percent, case.C, case.ignore, max_regions=case.R, check=False, ws=ws)
    assert np.array_equal(out.cpu().numpy(), ref)
    assert _word(ws, _lrh_flag_offset(case)) == flag
    if flag:
        with pytest.raises(ValueError):
            ops.lrh(cu(lab), cu(reg), case.percent, case.C, case.ignore, max_regions=case.R)


@pytest.mark.parametrize('case', L.FUSED_CASES, ids=_ids(L.FUSED_CASES))
def test_pseudo_lrh(ops, case):
    lab, reg = L.lrh_inputs(case, True)
    soft = L.soft_from_labels(lab, case.C, case.ignore, case.name)
    sel, _, cm = L.pseudo_ref(soft, 0.8, 0.6, case.ignore)
    ref, flag = L.lrh_ref(sel, reg, case.percent, case.C, case.ignore, case.R)
    sc, rc = cu(soft), cu(reg)
    out, ws = ops.pseudo_lrh(sc, cu(cm), rc, 0.8, 0.6, case.percent, case.C, case.ignore, max_regions=case.R)
    assert np.array_equal(out.cpu().numpy(), ref)
    assert _word(ws, _lrh_flag_offset(case)) == flag
    two = ops.lrh(ops.pseudo_select(sc, 0.8, 0.6, case.ignore), rc, case.percent, case.C, case.ignore, max_regions=case.R,
                  check=False)
    assert torch.equal(out, two)
    if flag:                                                    # a region id >= R: those pixels keep the selected label
        bad = (reg < 0) | (reg >= case.R)
        assert bad.any() and np.array_equal(out.cpu().numpy()[bad], sel[bad])
    out2, _ = ops.pseudo_lrh(sc, cu(cm), rc, 0.8, 0.6, case.percent, case.C, case.ignore, max_regions=case.R, ws=ws)
    assert torch.equal(out2, out)                               # the same workspace again: cleared per call


def test_pseudo_lrh_refusals(ops):
    c = L.FUSED_CASES[0]
    lab, reg = L.lrh_inputs(c, True)
    soft = cu(L.soft_from_labels(lab, c.C, c.ignore, c.name))
    cm = soft.amax((2, 3)).contiguous()
    with pytest.raises(ValueError):                             # max_regions > 65535: region ids travel as 16 bits
        ops.pseudo_lrh(soft, cm, cu(reg), 0.8, 0.6, 0.5, c.C, -1, max_regions=L.FUSED_MAX_REGIONS + 1)
    with pytest.raises(ValueError):                             # hw % 4 != 0: the two-call route serves it
        ops.pseudo_lrh(soft[..., :3].contiguous(), cm, cu(reg)[..., :3].contiguous(), 0.8, 0.6, 0.5, c.C, -1, max_regions=c.R)


# ---------------------------------------------------------------- downscale + prototypes
@pytest.mark.parametrize('case', L.DS_CASES, ids=_ids(L.DS_CASES))
def test_downscale_and_prototypes(ops, case):
    C, k, s = case.C, case.k, case.scale
    label, feat, protos, _ = L.ds_inputs(case)
    ref_ds, ref_cnt, flag, _ = L.downscale_ref(label, s, C, -1, case.min_ratio)
    s64, n64 = L.proto_sums_ref(feat, ref_ds, C)
    fi = ops.proto_flag_index(C, k)
    stats, ds = ops.proto_stats(cu(feat), cu(label), s, -1, case.min_ratio, C, check=True)
    assert np.array_equal(ds.cpu().numpy(), ref_ds)
    assert np.array_equal(stats[C * k:C * k + C].cpu().numpy(), ref_cnt.astype(np.float32))
    assert int(stats.view(torch.int32)[fi].item()) == flag == 0
    _check('sums', stats[:C * k].reshape(C, k), s64, TOL['proto_sums'])
    for decay in (0.996, 0.0):                                  # decay 0: Aligner.init_avg
        p = cu(protos).clone()
        ops.proto_apply(p, stats, decay)
        _check('protos decay %g' % decay, p, L.proto_apply_ref(protos, s64, n64, decay), TOL['protos'])
    # rgda_proto_update is stats + apply: the same bits
    p_apply, p_update = cu(protos).clone(), cu(protos).clone()
    ops.proto_apply(p_apply, stats, 0.996)
    ds_u = ops.proto_update(cu(feat), cu(label), p_update, s, -1, case.min_ratio, 0.996, check=True)
    assert torch.equal(ds_u, ds) and torch.equal(p_update, p_apply)
    # a class without pixels keeps its prototype (the bound of the EMA of a value with itself)
    assert ref_cnt[L.DS_ABSENT] == 0
    # the sums of two half-batches add up to the whole batch's: counts exactly, each half's sums within the bound
    if case.b >= 2:
        parts = [ops.proto_stats(cu(feat[a:b]), cu(label[a:b]), s, -1, case.min_ratio, C)[0] for a, b in ((0, 1), (1, case.b))]
        assert torch.equal(parts[0][C * k:C * k + C] + parts[1][C * k:C * k + C], stats[C * k:C * k + C])
        both = parts[0][:C * k].double() + parts[1][:C * k].double()
        _check('half sums', both.reshape(C, k), s64, 2 * TOL['proto_sums'])
    # the same cells through the generic kernel (one column, w = 1): the same decisions, bit for bit
    col = L.cells_as_column(label, s)
    n = col.shape[1] // s
    st_c, ds_c = ops.proto_stats(torch.zeros(1, 1, n, 1, device='cuda'), cu(col), s, -1, case.min_ratio, C)
    assert np.array_equal(ds_c.cpu().numpy().reshape(-1), ref_ds.reshape(-1))
    assert np.array_equal(st_c[C:2 * C].cpu().numpy(), ref_cnt.astype(np.float32))
    # a label outside [0, C) that is not ignore: bit 2 on this route, the cells without it unchanged, check=True raises
    for bad in (C, -2):
        lb = L.ds_inputs(case, bad)[0]
        ds2, _, f2, clean = L.downscale_ref(lb, s, C, -1, case.min_ratio)
        st_b, ds_b = ops.proto_stats(cu(feat), cu(lb), s, -1, case.min_ratio, C)
        assert int(st_b.view(torch.int32)[fi].item()) == f2 == 2, bad
        assert np.array_equal(ds_b.cpu().numpy()[:, 0][clean], ds2[:, 0][clean])
        with pytest.raises(ValueError):
            ops.proto_stats(cu(feat), cu(lb), s, -1, case.min_ratio, C, check=True)
        with pytest.raises(ValueError):
            ops.proto_update(cu(feat), cu(lb), cu(protos).clone(), s, -1, case.min_ratio, 0.996, check=True)


# ---------------------------------------------------------------- label_refine, teacher_probs
@pytest.mark.parametrize('case', L.REFINE_CASES, ids=_ids(L.REFINE_CASES))
def test_label_refine(ops, case):
    x = L.refine_inputs(case)
    ref = L.refine_ref(x['feat'], x['protos'], x['p1'], x['p2'], x['soft'], x['sup'], case.temp, case.views)
    g = {k: cu(v) for k, v in x.items()}
    b, C = case.b, case.C
    if case.sup:
        out, ws = ops.label_refine_sup(g['feat'], g['protos'], g['p1'], g['p2'], g['soft'], g['sup'], case.temp, case.views,
                                       max_regions=int(x['sup'].max()) + 1, return_ws=True)
    else:
        out, ws = ops.label_refine(g['feat'], g['protos'], g['p1'], g['p2'], g['soft'], case.temp, return_ws=True,
                                   views=case.views)
    _check(case.name, out, ref, TOL['refine_sup' if case.sup else 'refine'])
    # the per-class maxima pseudo_selection consumes are the maxima of the output, exactly
    cm = ws[:b * C * 4].view(torch.float32).reshape(b, C)
    assert torch.equal(cm, out.flatten(2).max(-1)[0])


@pytest.mark.parametrize('ref', L.REFINE_REFUSALS, ids=[r[0] for r in L.REFINE_REFUSALS])
def test_label_refine_refusals(ops, ref):
    """The limits refine_run states, through the C ABI: every one answers before anything is launched."""
    from regda_amd._lib import lib
    name, entry, k, C, views, short, status = ref
    b, h, w, H, W, R = 1, 2, 2, 4, 4, 8
    buf = torch.zeros(1 << 20, device='cuda')
    sup = torch.zeros(H * W, dtype=torch.int64, device='cuda')
    out = torch.zeros(b * C * H * W, device='cuda')
    ws = torch.zeros(1 << 22, dtype=torch.uint8, device='cuda')
    nbytes = 16 if short else ws.numel()
    st = ops._stream()
    p = buf.data_ptr()
    if entry == 'views':
        rc = lib().raw('rgda_label_refine_views')(p, p, p, p, p, out.data_ptr(), b, k, C, h, w, H, W, 2.0, views,
                                                  ws.data_ptr(), nbytes, st)
    else:
        rc = lib().raw('rgda_label_refine_sup')(p, p, p, p, p, sup.data_ptr(), out.data_ptr(), b, k, C, h, w, H, W, 2.0,
                                                views, R, ws.data_ptr(), nbytes, st)
    assert rc == status


@pytest.mark.parametrize('i', range(len(L.TEACHER_CASES)))
def test_teacher_probs(ops, i):
    p1, p2, size = L.teacher_inputs(i)
    out = ops.teacher_probs(cu(p1), cu(p2), size)
    _check('teacher %d' % i, out, L.teacher_ref(p1, p2, size), TOL['teacher'])


# ---------------------------------------------------------------- class_count, masks_to_regions
@pytest.mark.parametrize('n,C', L.COUNT_CASES)
def test_class_count(ops, n, C):
    lab = L.count_inputs(n, C)
    out = ops.class_count(cu(lab), C)
    assert out.dtype == torch.int32 and np.array_equal(out.cpu().numpy(), L.class_count_ref(lab, C))


@pytest.mark.parametrize('case', L.REGION_CASES, ids=[c[0] for c in L.REGION_CASES])
def test_masks_to_regions(ops, case):
    masks, areas, thr = L.region_inputs(*case)
    out = ops.masks_to_regions(cu(masks), cu(areas), thr)
    assert out.dtype == torch.int32 and np.array_equal(out.cpu().numpy(), L.regions_ref(masks, areas, thr))
