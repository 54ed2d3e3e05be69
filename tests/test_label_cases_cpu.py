"""CPU: the case table of tests/label_cases.py reaches every path it names, its restatement of the host-side decisions
still matches label_kernels.hip, its references agree with the oracles on the golden inputs (and, for the scales the
oracle does not take, with torch's own one_hot -> avg_pool2d -> max), and the inputs keep the conditions the per-element
bounds of tests/test_label_passes_gpu.py rest on."""
import json
import os
import re

import numpy as np
import pytest
import torch

import label_cases as L
from oracle import labelpath as opath
from oracle import labels as olab
from oracle import regions as oreg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = open(os.path.join(ROOT, 'regda_amd', 'csrc', 'label_kernels.hip')).read()
COMMON = open(os.path.join(ROOT, 'regda_amd', 'csrc', 'common.h')).read()
HDR = open(os.path.join(ROOT, 'include', 'rgda_hip.h')).read()


def _const(pattern, src=SRC):
    m = re.search(pattern, src)
    assert m, pattern
    return int(m.group(1))


def _body(name):
    """The text of an entry point from its name to the next `extern "C"`."""
    i = SRC.index(name + '(')
    j = SRC.find('extern "C"', i)
    return SRC[i:j if j > 0 else len(SRC)]


def test_every_named_path_is_reached():
    reached = L.paths_reached()
    print('\n'.join('%-28s %s' % (p, ', '.join(sorted(set(reached.get(p, []))))) for p in L.REQUIRED))
    missing = [p for p in L.REQUIRED if not reached.get(p)]
    assert not missing, missing
    for prefix, cases in (('', L.PSEUDO_CASES + L.PSEUDO_FLAG_CASES), ('', L.LRH_CASES), ('fused:', L.FUSED_CASES),
                          ('', L.DS_CASES), ('', L.REFINE_CASES)):
        for c in cases:
            got = {p for p, names in reached.items() if prefix + c.name in names}
            assert set(c.paths) <= got, (c.name, set(c.paths) - got)


def test_restatement_matches_the_source():
    # pseudo_select: the chunk and the float4 route
    ps = _body('int rgda_pseudo_select')
    assert _const(r'int chunk = (\d+);', ps) == L.PSEUDO_CHUNK
    assert re.search(r'if \(\(hw & 3\) == 0 && \(chunk & 3\) == 0\) \{', SRC)
    assert re.search(r'c <= 0 \|\| c > 16', ps)
    # lrh: lds_regions, the chunk and its halving
    lrh = _body('int rgda_lrh')
    assert re.search(r'int lds_regions = min\(R, \(48 \* 1024\) / \(C \* 4\)\);', lrh) and L.HIST_LDS_BYTES == 48 * 1024
    assert _const(r'int chunk = (\d+);', lrh) == L.LRH_CHUNK
    m = re.search(r'while \(chunk > (\d+) && \(long long\)cdiv\(hw, chunk\) \* b < (\d+)\) chunk >>= 1;', lrh)
    assert m and (int(m.group(1)), int(m.group(2))) == (L.LRH_CHUNK_MIN, L.LRH_MIN_WG)
    # the fused pass
    pl = _body('int rgda_pseudo_lrh')
    assert re.search(r'int lds_regions = min\(R, \(48 \* 1024\) / \(C \* 4\)\);', pl)
    m = re.search(r'int chunk = (\d+), min_wg = (\d+);', pl)
    assert m and (int(m.group(1)), int(m.group(2))) == (L.PICK_CHUNK, L.PICK_MIN_WG)
    assert _const(r'while \(chunk > (\d+) && \(long long\)cdiv\(hw, chunk\) \* b < min_wg\) chunk >>= 1;', pl) == L.PICK_CHUNK_MIN
    assert _const(r'max_regions <= 0 \|\| max_regions > (\d+)\)', pl) == L.FUSED_MAX_REGIONS
    assert re.search(r'if \(!class_count_ok\(class_num\) \|\| \(hw & 3\)\) return RGDA_ERR_UNSUPPORTED;', pl)
    # the downscale route
    st = _body('int rgda_proto_stats')
    assert re.search(r'if \(scale == 16 && !\(w & 1\)\) \{\s*if constexpr \(C <= 7\)\s*downscale_label16_kernel<C>.*?'
                     r'else\s*downscale_label16_wide_kernel<C>.*?\} else \{\s*downscale_label_kernel<<<', st, flags=re.S)
    assert L.DOWNSCALE_FAST_SCALE == 16 and L.DOWNSCALE_FAST_CLASSES == 7
    # label_refine
    assert _const(r'constexpr int REFINE_ROWS = (\d+);') == L.REFINE_ROWS
    assert re.search(r'static constexpr int refine_slices\(int C\) \{ return C <= 14 \? 16 : 8; \}', SRC)
    assert [L.refine_slices(c) for c in (6, 14, 15, 16)] == [16, 16, 8, 8]
    assert re.search(r'static size_t refine_lds\(int C, int k\) \{ return \(\(size_t\)C \* k \+ \(size_t\)refine_slices\(C\) '
                     r'\* 32 \* \(C \+ 1\)\) \* 4; \}', SRC)
    m = re.search(r'constexpr int PX = (\d+), SL = refine_slices\(C\);', SRC)
    assert m and int(m.group(1)) == L.REFINE_PX
    assert re.search(r'const int kper = \(K \+ SL - 1\) / SL;', SRC)
    assert re.search(r'k < 2 \|\| k > 4096 \|\| \(k & 3\)', SRC) and L.REFINE_K_MAX == 4096
    assert re.search(r'if \(pview && refine_lds\(c, k\) > RGDA_LDS_MAX\) return RGDA_ERR_UNSUPPORTED;', SRC)
    assert re.search(r'if \(lds > 64 \* 1024 &&', SRC) and L.LDS_ATTR == 64 * 1024
    assert re.search(r'dim3 g2\(cdiv\(W, 256\), cdiv\(H, REFINE_ROWS\), b\);', SRC) and L.REFINE_COLS == 256
    assert re.search(r'#define RGDA_LDS_MAX \(\(size_t\)160 \* 1024\)', COMMON) and L.LDS_MAX == 160 * 1024
    assert _const(r'#define RGDA_MIN_CLASSES (\d+)', COMMON) == L.MIN_CLASSES
    assert _const(r'#define RGDA_MAX_CLASSES (\d+)', COMMON) == L.MAX_CLASSES
    for name, v in (('OK', L.OK), ('ERR_ARG', L.ERR_ARG), ('ERR_WORKSPACE', L.ERR_WORKSPACE), ('ERR_UNSUPPORTED', L.ERR_UNSUPPORTED)):
        assert int(re.search(r'RGDA_%s = (-?\d+)' % name, HDR).group(1)) == v
    # what the restatement says about the refusals of the table
    for name, entry, k, C, views, short, status in L.REFINE_REFUSALS:
        if not short and 1 <= views <= 3:
            assert L.refine_status(C, k, views) == status, name
    assert L.refine_status(16, 2048, 3) == L.OK and L.refine_slices(16) == 8


def test_pseudo_and_lrh_references_agree_with_the_oracle_on_the_goldens(gold):
    n = 0
    for fname, prefixes in (('pseudo.npz', ['']), ('c7.npz', ['ps_']), ('cn.npz', ['c8_ps_', 'c11_ps_', 'c16_ps_'])):
        g = gold(fname)
        for p in prefixes:
            for i in range(int(g[p + 'n'])):
                x = g[f'{p}in{i}']
                lab, flag, cm = L.pseudo_ref(x, 0.8, 0.6, -1)
                assert flag == 0 and np.array_equal(lab, g[f'{p}out{i}'].astype(np.int64)), (fname, p, i)
                assert np.array_equal(lab, olab.pseudo_selection(x, 0.8, 0.6, -1))
                n += 1
    for fname, prefixes in (('lrh.npz', [('', 6)]), ('c7.npz', [('lrh_', 7)]), ('cn.npz', [('c8_lrh_', 8), ('c11_lrh_', 11), ('c16_lrh_', 16)])):
        g = gold(fname)
        for p, C in prefixes:
            cnt = int(g[p + 'n']) if (p + 'n') in g.files else int(g['n'])
            for i in range(cnt):
                lab, reg, pct = g[f'{p}lab{i}'].astype(np.int64), g[f'{p}reg{i}'].astype(np.int64), float(g[f'{p}pct{i}'])
                out, flag = L.lrh_ref(lab, reg, pct, C, -1, 4096)
                assert flag == 0 and np.array_equal(out, g[f'{p}out{i}'].astype(np.int64)), (fname, p, i)
                assert np.array_equal(out, olab.homogenize(lab, reg, pct, C, -1))
                n += 1
    assert n > 30
    # and on every clean case of the table (the oracle sizes its table by the largest id: the ids must fit R)
    for fused, cases in ((False, L.LRH_CASES), (True, L.FUSED_CASES)):
        for c in cases:
            lab, reg = L.lrh_inputs(c, fused)
            out, flag = L.lrh_ref(lab, reg, c.percent, c.C, c.ignore, c.R)
            assert flag == (1 if c.kind == 'bad_region' else 2 if c.kind == 'bad_label' else 0), c.name
            if not flag:
                assert np.array_equal(out, olab.homogenize(lab, reg, c.percent, c.C, c.ignore)), c.name
                assert np.array_equal(out[reg == 0], lab[reg == 0])
            if c.kind == 'built' and 0 < c.percent < 1:
                assert (out != lab).any() and (out == lab).any()
    for c in L.PSEUDO_CASES:
        soft, cm = L.pseudo_inputs(c)
        lab, flag, _ = L.pseudo_ref(soft, 0.8, 0.6, -1, cm)
        assert flag == 0
        if cm is None:
            assert np.array_equal(lab, olab.pseudo_selection(soft, 0.8, 0.6, -1)), c.name
        if lab.size >= 63:
            assert (lab >= 0).any() and (lab < 0).any(), c.name
    for c in L.PSEUDO_FLAG_CASES:
        soft, _ = L.pseudo_inputs(c)
        assert L.pseudo_ref(soft)[1] == 1
        with pytest.raises(AssertionError):          # the reference's own assert fails on each of them, the NaN included
            olab.pseudo_selection(soft, 0.8, 0.6, -1)


def test_fused_inputs_select_the_planned_labels():
    for c in L.FUSED_CASES:
        lab, reg = L.lrh_inputs(c, True)
        soft = L.soft_from_labels(lab, c.C, c.ignore, c.name)
        sel, flag, _ = L.pseudo_ref(soft, 0.8, 0.6, c.ignore)
        assert flag == 0 and np.array_equal(sel, lab), c.name


def test_downscale_reference_against_the_oracle_and_torch(gold):
    g = gold('downscale.npz')
    ds, cnt, flag, clean = L.downscale_ref(g['lab'].astype(np.int64), 16, 6, -1, 0.75)
    assert flag == 0 and clean.all() and np.array_equal(ds, g['out'].astype(np.int64))
    g = gold('refine.npz')
    assert np.array_equal(L.downscale_ref(g['lab_s'].astype(np.int64), 16, 6)[0], g['ds'].astype(np.int64))
    seen = set()
    for c in L.DS_CASES:
        label, feat, protos, names = L.ds_inputs(c)
        ds, cnt, flag, clean = L.downscale_ref(label, c.scale, c.C, -1, c.min_ratio)
        assert flag == 0 and clean.all()
        # torch's own pooling, bit for bit, at every scale; the oracle where it applies; exact integers (no decision
        # of the table hangs on an fp32 rounding)
        assert np.array_equal(ds, L.downscale_torch(label, c.scale, c.C, -1, c.min_ratio)), c.name
        assert np.array_equal(ds, olab.downscale_label(label, c.scale, c.C, -1, c.min_ratio)), c.name
        assert np.array_equal(ds, L.downscale_exact(label, c.scale, c.C, -1, c.min_ratio)), c.name
        assert cnt[L.DS_ABSENT] == 0 and cnt.sum() > 0, c.name
        # the constructed cells decide as planned
        d = ds[:, 0]
        for (i, y, x), kind in np.ndenumerate(names):
            cell = label[i, y * c.scale:(y + 1) * c.scale, x * c.scale:(x + 1) * c.scale]
            vals = [v for v in np.unique(cell) if v >= 0]
            if kind == 'exact':
                assert d[i, y, x] == vals[0]
            elif kind in ('below', 'all_ign'):
                assert d[i, y, x] == -1
            elif kind == 'last':
                assert d[i, y, x] == c.C - 1
            elif kind == 'tie_ign':
                assert d[i, y, x] == (vals[0] if c.min_ratio <= 0.5 else -1)
            elif kind == 'tie_classes':
                assert len(vals) == 2 and d[i, y, x] == (min(vals) if c.min_ratio <= 0.5 else -1)
            seen.add((L.downscale_route(c.scale, c.w, c.C), kind))
        # the same cells as one column: the generic route, the same decisions
        col = L.cells_as_column(label, c.scale)
        assert L.downscale_route(c.scale, 1, c.C) == 'generic'
        assert np.array_equal(L.downscale_ref(col, c.scale, c.C, -1, c.min_ratio)[0].reshape(-1), ds.reshape(-1))
        # a label outside the range: flagged, the other cells unchanged
        for bad in (c.C, -2):
            lb = L.ds_inputs(c, bad)[0]
            ds2, _, f2, clean2 = L.downscale_ref(lb, c.scale, c.C, -1, c.min_ratio)
            assert f2 == 2 and (~clean2).sum() == 1 and np.array_equal(ds2[:, 0][clean2], ds[:, 0][clean2])
    for route in ('generic', 'fast', 'wide'):
        for kind in ('exact', 'below', 'all_ign', 'last', 'tie_ign', 'tie_classes'):
            assert (route, kind) in seen, (route, kind)


def test_prototype_references_agree_with_the_oracle(gold):
    g = gold('refine.npz')
    feat, lab, protos = torch.from_numpy(g['feat_s']), torch.from_numpy(g['lab_s'].astype(np.int64)), torch.from_numpy(g['protos'])
    ds = torch.from_numpy(L.downscale_ref(lab.numpy(), 16, 6)[0])
    sums, cnt = L.proto_sums_ref(feat, ds, 6)
    new = L.proto_apply_ref(protos, sums, cnt, 0.996)
    np.testing.assert_allclose(new.numpy(), g['protos_new'], rtol=1e-5, atol=1e-6)
    osum, ocnt = opath.prototype_statistics(feat, ds, 6, -1)
    assert torch.equal(ocnt.double(), cnt)
    np.testing.assert_allclose(osum.numpy(), sums.numpy(), rtol=1e-5, atol=1e-5)


def test_refine_references_agree_with_the_oracle_on_the_goldens(gold):
    g, gs = gold('refine.npz'), gold('refine_sup.npz')
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    feat, protos, p1, p2, soft = t(g['feat_t']), t(g['protos']), t(g['p1']), t(g['p2']), t(g['soft'])
    sup = t(gs['sup'].astype(np.int64)).reshape(2, 1, 64, 64)
    # the golden tolerance of tests/test_label_gpu.py (the inputs hold the one pixel with 1 / dist ~ 1e7)
    for key, views, temp, s, gg in (('out', 3, 2.0, None, g), ('out_p', 1, 2.0, None, g), ('out_l', 2, 1.5, None, g),
                                    ('out_all', 3, 2.0, sup, gs), ('out_s', 0, 1.5, sup, gs)):
        ref = L.refine_ref(feat, protos, p1, p2, soft, s, temp, views)
        np.testing.assert_allclose(ref.numpy(), gg[key], rtol=2e-4, atol=2e-6, err_msg=key)
        # the fp32 form the tolerances are derived from IS the oracle wherever the oracle has the mode
        mode = {3: 'all', 1: 'p', 2: 'l', 0: 's'}[views]
        o32 = L.refine_oracle32(feat, protos, p1, p2, soft, s, temp, views)
        assert torch.equal(o32, opath.label_refine(feat, protos, [p1, p2], soft, True, mode, temp, label_t_sup=s)), key
    np.testing.assert_allclose(L.feat_dist(feat, protos).numpy(), g['dist'], rtol=1e-4, atol=2e-7)
    cn = gold('cn.npz')
    for C in (8, 11, 16):
        q = {k[len(f'c{C}_'):]: cn[k] for k in cn.files if k.startswith(f'c{C}_rf_')}
        H = q['rf_sup'].shape[-1]
        s = t(q['rf_sup'].astype(np.int64)).reshape(-1, 1, H, H)
        a = (t(q['rf_feat']), t(q['rf_protos']), t(q['rf_p1']), t(q['rf_p2']), t(q['rf_soft']))
        np.testing.assert_allclose(L.refine_ref(*a).numpy(), q['rf_out'], rtol=5e-4, atol=1e-6)
        np.testing.assert_allclose(L.refine_ref(*a, s).numpy(), q['rf_out_sup'], rtol=5e-4, atol=1e-6)
    for i in range(len(L.TEACHER_CASES)):
        p1, p2, size = L.teacher_inputs(i)
        np.testing.assert_allclose(L.teacher_ref(p1, p2, size).numpy(), opath.teacher_probs(p1, p2, size).numpy(), rtol=1e-4, atol=1e-6)


def test_refine_inputs_keep_their_conditions():
    for c in L.REFINE_CASES:
        x = L.refine_inputs(c)
        assert L.refine_status(c.C, c.k, c.views) == L.OK, c.name
        if c.views & 1:
            d = L.feat_dist(x['feat'], x['protos'])
            assert float(d.min()) >= L.DIST_FLOOR, (c.name, float(d.min()))
        if c.sup:
            sup, soft = x['sup'], x['soft']
            b = sup.shape[0]
            top = int(sup.max())
            assert (soft == 0).any()
            assert all(int(sup[i].max()) < top for i in range(b - 1)) or b == 1       # the largest id: the last image only
            ids0 = set(sup[0].unique().tolist())
            if b > 1:
                assert ids0 - set(sup[1:].unique().tolist())                          # an id used in one image only
            assert (torch.bincount(sup[0].reshape(-1)) == 1).any()                    # single-pixel superpixels
    # C = 16 at k = 2048 takes the 8-slice route and fits; k = 4096 does not
    assert L.refine_lds(16, 2048) <= L.LDS_MAX < L.refine_lds(16, 4096)
    assert any(L.refine_lds(c.C, c.k) > L.LDS_ATTR and (c.shape[0] * c.shape[1]) % 32 for c in L.REFINE_CASES if c.views & 1)


def test_counts_and_regions_references_agree_with_the_oracle(gold):
    g = gold('regions.npz')
    for i in range(int(g['n'])):
        assert np.array_equal(L.regions_ref(g[f'masks{i}'], g[f'areas{i}'], int(g[f'thr{i}'])), g[f'regions{i}']), i
    for name, K, HW, kind in L.REGION_CASES:
        masks, areas, thr = L.region_inputs(name, K, HW, kind)
        ref = L.regions_ref(masks, areas, thr)
        assert np.array_equal(ref, oreg.regions_from_masks(masks, areas, thr)), name
        if kind == 'under' or K == 0:
            assert not ref.any()
        if kind == 'last':
            assert (ref[0, HW // 2:] == K).all() and (ref[0, :HW // 2] >= K - 1).all() and (ref == K - 1).any()
    for n, C in L.COUNT_CASES:
        lab = L.count_inputs(n, C)
        ref = L.class_count_ref(lab, C)
        assert ref.sum() == ((lab >= 0) & (lab < C)).sum()
        if n > 100:
            assert ref.sum() < n
            f = opath.class_balance_local_freq(torch.from_numpy(np.where((lab < 0) | (lab >= C), -1, lab)), C, -1)
            np.testing.assert_allclose(f.numpy(), ref / (ref.sum() + 1e-7), rtol=1e-6)


def test_tolerance_file_is_the_derivation():
    """tests/golden/label_tolerances.json holds, per family, the measured deviation of the fp32 oracle from the fp64
    reference and the margin; every bound is margin * measured and positive."""
    tol = json.load(open(os.path.join(ROOT, 'tests', 'golden', 'label_tolerances.json')))
    assert tol['margin'] == 3.0
    for fam in ('refine', 'refine_sup', 'teacher', 'proto_sums', 'protos'):
        assert tol['bounds'][fam] == tol['margin'] * tol['observed'][fam] > 0, fam
