"""CPU: the case table of tests/loss_cases.py reaches every path it names, its restatement of the host-side decisions
still matches loss_kernels.hip, the simulated radix select keeps what the float64 reference keeps, the reference agrees
with tests/loss_ref.py and with the reference's own classes (tests/golden/losses.npz), the committed bounds
(tests/golden/loss_tolerances.json) are current, the inputs keep the conditions the bounds rest on, and the bounds catch
six wrong lines put into the fp32 restatement."""
import json
import os
import re

import numpy as np
import pytest
import torch

import loss_cases as L
import loss_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = open(os.path.join(ROOT, 'regda_amd', 'csrc', 'loss_kernels.hip')).read()
COMMON = open(os.path.join(ROOT, 'regda_amd', 'csrc', 'common.h')).read()
TOL = json.load(open(os.path.join(ROOT, 'tests', 'golden', 'loss_tolerances.json')))


def _const(pattern, src=SRC):
    m = re.search(pattern, src)
    assert m, pattern
    return int(m.group(1))


def test_every_named_path_is_reached():
    reached = L.paths_reached()
    print('\n'.join('%-24s %s' % (p, ', '.join(sorted(set(reached.get(p, []))))[:160]) for p in L.REQUIRED))
    missing = [p for p in L.REQUIRED if not reached.get(p)]
    assert not missing, missing
    for c in L.CASES:
        got = {p for p, names in reached.items() if c.name in names}
        assert set(c.paths) <= got, (c.name, set(c.paths) - got)
    # every kind on every geometry of the table, with and without class weights where the entry point takes them
    for geo in L.TABLE_GEOS:
        for kind in L.KINDS:
            assert '%s-%s' % (geo, kind) in L.BY_NAME
            assert (('%s-%s-cw' % (geo, kind)) in L.BY_NAME) == (kind in L.TAKES_CW)


def test_restatement_matches_the_source():
    assert _const(r'constexpr int SEL_PASSES = (\d+);') == L.SEL_PASSES == len(L.SEL_SHIFT) == len(L.SEL_WIDTH)
    assert _const(r'constexpr int SEL_BINS = (\d+);') == L.SEL_BINS == 1 << max(L.SEL_WIDTH)
    assert _const(r'constexpr int CNT_REPL = (\d+);') == L.CNT_REPL
    assert _const(r'constexpr int GHM_BINS = (\d+);') == L.GHM_BINS
    m = re.search(r'kSelShift\[SEL_PASSES\] = \{([^}]*)\};\s*__constant__ int kSelWidth\[SEL_PASSES\] = \{([^}]*)\};', SRC)
    assert m and tuple(int(v) for v in m.group(1).split(',')) == L.SEL_SHIFT
    assert tuple(int(v) for v in m.group(2).split(',')) == L.SEL_WIDTH
    # the digits tile the 64-bit key from the top: 32 bits of loss, 32 bits of inverted index
    assert L.SEL_SHIFT[0] + L.SEL_WIDTH[0] == 64 and L.SEL_SHIFT[-1] == 0 and L.SEL_SHIFT[2] == 32
    assert all(L.SEL_SHIFT[i] == L.SEL_SHIFT[i + 1] + L.SEL_WIDTH[i + 1] for i in range(L.SEL_PASSES - 1))
    assert re.search(r'const int blocks = \(int\)min\(\(long long\)cdiv\(n, 256 \* 8\), 512ll\);', SRC)
    assert (L.SEL_CHUNK, L.SEL_MAX_WG) == (256 * 8, 512)
    assert [L.select_grid(n) for n in (1, 2048, 2049, 8192, 1 << 21)] == [1, 1, 2, 4, 512]
    assert re.search(r'return \(\(size_t\)2 \* c \* 2 \* w \+ \(want \? \(size_t\)2 \* c \* W : 0\) \+ \(size_t\)2 \* W\) \* 4;', SRC)
    assert re.search(r'if \(lds <= 64 \* 1024\) return RGDA_OK;', SRC) and L.LDS_ATTR == 64 * 1024
    assert re.search(r'constexpr size_t MAX_ROW_LDS = RGDA_LOSS_ROW_LDS_MAX;', SRC)
    assert _const(r'#define RGDA_LOSS_ROW_LDS_MAX \(\(size_t\)(\d+) \* 1024\)', COMMON) * 1024 == L.ROW_LDS_MAX
    assert len(re.findall(r'if \(grad_lds\(c, w, W, g1 != nullptr\) > MAX_ROW_LDS\) return RGDA_ERR_UNSUPPORTED;', SRC)) == 4
    assert len(re.findall(r'for \(int X = threadIdx\.x; X < W; X \+= 256\)', SRC)) >= 2 and L.ROW_THREADS == 256
    assert re.search(r'const int rep = \(blockIdx\.y \* gridDim\.x \+ blockIdx\.x\) % CNT_REPL;', SRC)
    assert _const(r'#define RGDA_MIN_CLASSES (\d+)', COMMON) == L.MIN_CLASSES
    assert _const(r'#define RGDA_MAX_CLASSES (\d+)', COMMON) == L.MAX_CLASSES
    # the figures the issue's table states
    assert L.grad_lds(7, 64, 1024) == 72704 and L.row_route(7, 64, 1024) == 'attr'
    assert L.grad_lds(16, 32, 512) == 77824 and L.row_route(16, 32, 512) == 'attr'
    assert L.grad_lds(16, 64, 1024) == 155648 and L.row_route(16, 64, 1024) == 'refuse'
    assert L.grad_lds(16, 64, 1024, False) == 24576 and L.row_route(16, 64, 1024, False) == 'default'
    assert L.row_iters(300) == 2 and L.row_iters(1024) == 4 and L.row_iters(3) == 1
    # lerp_ac as common.h states it
    assert re.search(r'float scale = \(out > 1\) \? __fdiv_rn\(\(float\)\(in - 1\), \(float\)\(out - 1\)\) : 0\.f;\s*'
                     r'float src = __fmul_rn\(scale, \(float\)dst\);', COMMON)
    assert not L.covered(7, 3).all() and L.covered(5, 300).all() and L.covered(1, 7).all()


def _sims(x):
    lab = x['lab'].reshape(-1)
    n_min = int((lab != x['ignore']).sum()) // 5
    return [L.select_sim(L.decision_values(x, hd, torch.float32).numpy(), n_min, x['thresh']) for hd in range(2)], n_min


def test_simulated_select_keeps_what_the_reference_keeps():
    """The radix select on the restatement's fp32 losses, digit by digit as ohem_select_kernel walks them, keeps the
    pixels the float64 reference keeps (stable descending sort: the lowest index of equal losses first)."""
    n = 0
    for c in L.CASES:
        if c.kind != 'ohem':
            continue
        x = L.inputs(c.name)
        sims, n_min = _sims(x)
        r = L.ref64(x)
        for hd in range(2):
            assert sims[hd]['branch'] == r['branch'][hd], c.name
            # (among exact zeros the keep set holds ignored pixels too: they carry neither loss nor gradient)
            assert torch.equal(torch.from_numpy(sims[hd]['keep']), r['keep'][hd]), c.name
            if sims[hd]['branch'] == 'topk':
                assert int(r['keep'][hd].sum()) == n_min
            n += 1
    assert n > 50


def test_tie_cases_are_what_they_claim():
    # tie_cut: fewer than n_min pixels above the tie group, more pixels than still needed inside it, the group below
    # the threshold; all six passes
    x = L.inputs('id64-ohem-tie_cut')
    v = L.decision_values(x, 0, torch.float64)
    tie = x['tie']
    n_min = int((x['lab'] != -1).sum()) // 5
    tv = v[tie[0]]
    assert (v[tie] == tv).all() and int((v == tv).sum()) == tie.numel() == 1000
    assert 0.2 < float(tv) < L.OHEM_THRESH and abs(float(tv) - 0.2223) < 1e-3
    above = int((v > tv).sum())
    assert above == 1000 < n_min == 1638 and tie.numel() > n_min - above == 638
    assert int((v > L.OHEM_THRESH).sum()) == above              # nothing between the threshold and the group
    sims, _ = _sims(x)
    assert all(s['resolved'] == L.SEL_PASSES - 1 and s['straddle'] for s in sims)
    # the kept part of the group is its lowest indices
    keep = L.ref64(x)['keep'][0]
    srt = torch.sort(tie).values
    assert keep[srt[:638]].all() and not keep[srt[638:]].any()
    # zeros_cut: fewer than n_min positive losses; ignored pixels lie in the tie of zeros and below the cut index
    x = L.inputs('id64-ohem-zeros_cut')
    v, lab = L.decision_values(x, 0, torch.float64), x['lab'].reshape(-1)
    n_min = int((lab != -1).sum()) // 5
    keep = L.ref64(x)['keep'][0]
    n_pos = int((v > 0).sum())
    assert 400 < n_pos <= 500 < n_min and (keep & (lab == -1)).any() and int((keep & (v > 0)).sum()) == n_pos
    # n_min == 0 with valid pixels; kept == n_min exactly; every label ignored; one head on each branch
    x = L.inputs('id64-ohem-nmin0')
    assert int((x['lab'] != -1).sum()) == 4
    x = L.inputs('id64-ohem-kept_eq')
    sims, n_min = _sims(x)
    assert all(s['kept'] == n_min == 1638 and s['branch'] == 'thresh' for s in sims)
    assert np.isnan(L.ref64(L.inputs('id64-ohem-all_ignored'))['loss'])
    assert L.ref64(L.inputs('id64-ohem-head_split'))['branch'] == ['topk', 'thresh']
    # the far case: the first index digit decides, rows 0 and 1 of the three tie rows are kept
    x = L.inputs('far-ohem-tie_p3')
    keep = L.ref64(x)['keep'][0]
    assert x['lab'].numel() == (1 << 21) + 2048 and keep[:2048].all() and not keep[2048:3072].any()
    # no tie case excuses a pixel of its tie group
    for c in L.CASES:
        x = L.inputs(c.name)
        if x['tie'] is not None:
            assert (x['lab'].reshape(-1)[x['tie']] != x['ignore']).all(), c.name


def test_inputs_keep_the_conditions_the_bounds_rest_on():
    for c in L.CASES:
        x = L.inputs(c.name)
        n = x['lab'].numel()
        assert x['excused'] <= L.EXCUSED_SHARE * n, (c.name, x['excused'], n)
        if n < L.SMALL_CASE:
            assert x['excused'] == 0, c.name
        assert x['eps'] == max(1e-5, 3 * x['noise'])
        assert x['eps'] < 5e-4, (c.name, x['eps'])
        geo = x['geo']
        assert L.MIN_CLASSES <= geo.C <= L.MAX_CLASSES
        assert (L.row_route(geo.C, geo.w, geo.W, x['want_grad']) != 'refuse'), c.name
        if c.kind == 'ghm':
            assert float(x['acc0'].min()) > 0                       # a non-zero state
        if x['ignore'] == 255:
            assert (x['lab'] == 255).any() and not (x['lab'] == -1).any()
    # saturated blocks: a CE of exactly 0 in fp32 at valid pixels, in every focal case and the saturated GHM cases
    for c in L.CASES:
        if c.build == 'sat':
            x = L.inputs(c.name)
            ce = loss_ref._ce(loss_ref.up(x['p1'], tuple(x['lab'].shape[-2:])), x['lab'], -1)
            assert int(((ce == 0) & (x['lab'].reshape(-1) != -1)).sum()) >= 16, c.name


def test_reference_agrees_with_the_restatement_on_every_case():
    """float64 reference against tests/loss_ref.py within the bounds of tests/test_losses_gpu.py (loss 1e-5 relative,
    gradients rtol 1e-3 with a floor of 1e-4 of the largest)."""
    for c in L.CASES:
        x = L.inputs(c.name)
        r64, r32 = L.ref64(x), L.ref32(x)
        if np.isnan(r64['loss']):
            assert np.isnan(r32['loss'])
        else:
            assert r32['loss'] == pytest.approx(r64['loss'], rel=1e-5, abs=0), c.name
        if x['want_grad']:
            for a, b in zip(r32['g'], r64['g']):
                np.testing.assert_allclose(a.numpy(), b.numpy(), rtol=1e-3, atol=1e-4 * float(b.abs().max()), err_msg=c.name)
        if r64['acc'] is not None:
            np.testing.assert_allclose(r32['acc'].numpy(), r64['acc'].numpy(), rtol=1e-5, err_msg=c.name)
    # gamma = 0: the mean CE and its gradient
    x = L.inputs('id32-focal-g0')
    a, b = L.ref64(x), L.ref64(dict(x, kind='ce'))
    assert a['loss'] == pytest.approx(b['loss'], rel=1e-12) and all(torch.allclose(p, q, rtol=1e-12, atol=0) for p, q in zip(a['g'], b['g']))


GOLDEN = ['ohem', 'ohem_topk', 'ohem_ignored', 'focal', 'ghm', 'ups', 'uvem', 'uvem_zeros', 'ups_zeros', 'uvem_onehot']


@pytest.mark.parametrize('name', GOLDEN)
def test_reference_agrees_with_the_reference_classes(gold, name):
    """float64 reference against tests/golden/losses.npz (minted from the reference's own classes in fp32), within the
    bounds tests/test_losses_gpu.py holds the kernels to on the same file: loss 2e-6 relative, gradients rtol 2e-4 (1e-3
    where the one-hot soft label divides by 1e-7) with a floor of 1e-8, GHM's state 1e-6.  (The `_bal` goldens go through
    the class balancer's EMA, which is not part of these kernels.)"""
    g = gold('losses.npz')
    c = {k.split('/', 1)[1]: g[k] for k in g.files if k.startswith(name + '/')}
    kind = name.split('_')[0]
    acc = torch.zeros(30)
    for k in range(2 if kind == 'ghm' else 1):
        sfx = '' if k == 0 else str(k)
        x = L.make_x(kind, torch.from_numpy(c['p1']), torch.from_numpy(c['p2']), torch.from_numpy(c['lab'].astype(np.int64)),
                     torch.from_numpy(c['soft']) if 'soft' in c else None, acc0=acc)
        r = L.ref64(x)
        if np.isnan(float(c['loss' + sfx])):
            assert np.isnan(r['loss'])
        else:
            assert r['loss'] == pytest.approx(float(c['loss' + sfx]), rel=2e-6)
        for got, key in zip(r['g'], ('g1', 'g2')):
            np.testing.assert_allclose(got.numpy(), c[key + sfx], rtol=1e-3 if name == 'uvem_onehot' else 2e-4, atol=1e-8)
        if kind == 'ghm':
            np.testing.assert_allclose(r['acc'].numpy(), c['acc' + sfx], rtol=1e-6)
            acc = r['acc'].float()


def test_tolerance_file_is_current():
    """tests/golden/loss_tolerances.json is what tests/golden/derive_loss_tolerances.py writes for the table as it is:
    the same cases and outputs, bound = margin * observed + floor.  The floors come from the float64 reference and
    reproduce to rounding on any machine, so they pin the inputs and the reference.  The observed deviation of the fp32
    restatement is one draw of rounding noise that depends on how torch vectorises fp32 on the machine at hand: recomputed
    here, it must lie within the committed bound (the restatement passes the test the kernels take)."""
    assert TOL['margin'] == L.MARGIN == 3.0
    assert set(TOL['cases']) == set(L.BY_NAME)
    for c in L.CASES:
        t = TOL['cases'][c.name]
        obs, floor = L.deviations(L.inputs(c.name))
        assert set(t['bound']) == set(obs) == set(floor), c.name
        for k in obs:
            assert t['bound'][k] == pytest.approx(L.MARGIN * t['observed'][k] + t['floor'][k], rel=1e-12), (c.name, k)
            assert t['floor'][k] == pytest.approx(floor[k], rel=1e-6, abs=1e-300), (c.name, k)
            assert obs[k] <= t['bound'][k], (c.name, k, obs[k], t['bound'][k])
            assert t['bound'][k] > 0 or floor[k] == 0, (c.name, k)


def _breaks(name, r):
    """the outputs of a (mutated) restatement that miss the committed bounds of the case"""
    x = L.inputs(name)
    r64 = L.ref64(x)
    t = TOL['cases'][name]['bound']
    bad = []
    if 'loss' in t and not abs(r['loss'] - r64['loss']) <= t['loss'] * abs(r64['loss']):
        bad.append('loss')
    for k, (a, b) in enumerate(zip(r['g'], r64['g'])):
        if not bool(((a.double() - b).abs() <= t['g%d' % (k + 1)]).all()):
            bad.append('g%d' % (k + 1))
    return bad


MUTANTS = [('footprint_short', ['ragged_row-ce', 'odd_ratio-ce', 'narrow_down-focal']),
           ('tie_highest_index', ['id64-ohem-tie_cut', 'id64-ohem-tie_p4']),
           ('ghm_denominator_ignore_label', ['id32-ghm-ig255', 'ragged_row-ghm-ig255']),
           ('ghm_bucket_off_by_one', ['id32-ghm-m0', 'ragged_row-ghm']),
           ('ohem_denominator_kept', ['id64-ohem-topk', 'ragged_row-ohem-gap']),
           ('uvem_right_at_m_eq_t', ['id32-uvem-m_eq_t', 'ragged_row-uvem-m_eq_t'])]


@pytest.mark.parametrize('mutation,names', MUTANTS, ids=[m for m, _ in MUTANTS])
def test_bounds_catch_a_wrong_line_in_the_restatement(mutation, names):
    """Each named case passes its committed bounds with tests/loss_ref.py as it is and misses them with one line wrong."""
    for name in names:
        assert _breaks(name, L.ref32(L.inputs(name))) == [], name
        with L.mutated(mutation):
            bad = _breaks(name, L.ref32(L.inputs(name)))
        print(mutation, name, bad)
        assert bad, (mutation, name)
    # and the restatement is itself again
    assert _breaks(names[0], L.ref32(L.inputs(names[0]))) == []
