"""CPU: the case table of tests/superpixel_cases.py holds what every case is named for, computed from the numpy
restatement alone (tests/superpixel_ref.py); its copy of the host-side geometry still matches superpixel_kernels.hip; the
restatement's components agree with an independent flood fill on every small case; and the restatement's int32 bound is
asserted over the candidates that exist, no more and no less."""
import os
import re

import numpy as np
import pytest

import superpixel_cases as C
import superpixel_ref as R
from test_superpixels_cpu import _flood

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = open(os.path.join(ROOT, 'regda_amd', 'csrc', 'superpixel_kernels.hip')).read()


def _shape(c):
    H, W, _ = C.images(c.name)[0].shape
    return len(c.gens), H, W


def _areas(o):
    a = np.bincount(o.roots.reshape(-1))
    return a[a > 0]


def _trace(c):
    return C.assign_trace(C.images(c.name)[0], c.S, c.m, c.iters)


def _min_ties(d):
    big = np.where(d < 0, np.iinfo(np.int64).max, d)
    return int(((big == big.min(0)).sum(0) > 1).sum())


def _any_ties(d):
    """Pixels at which two existing candidates are equally far (whether or not they are the nearest)."""
    s = np.sort(np.where(d < 0, -np.arange(1, 10)[:, None, None], d), 0)          # absent slots: distinct negatives
    return int((s[1:] == s[:-1]).any(0).sum())


def _drop_keep(c):
    return all((_areas(o) < c.min_area).sum() >= 1 and (_areas(o) >= c.min_area).sum() >= 8 and o.count >= 8
               and (o.regs == 0).any() for o in C.oracle(c.name))


def _tile(n):
    return lambda c: C.cell_block(c.S)[1] == n and n <= C.SPX_MAX_T


def _grid(c):
    N, H, W = _shape(c)
    return H // c.S, W // c.S


# claim -> predicate on the case.  d_large: the issue asks for a candidate d above 2^30 on the black / white case.  No
# input of that shape has one: |y - cy| <= 127 and |x - cx| <= 191 in a 128 x 192 image, so d <= 3 * 255^2 * 64^2 +
# 64^2 * (127^2 + 191^2) = 1 014 521 856 < 2^30 = 1 073 741 824 (the restatement gives 0.41 .. 0.42 * 2^31 here, the
# figure the issue itself records).  Asserted instead: d exceeds the whole colour term 3 * 255^2 * S^2 = 0.372 * 2^31,
# that is, some pixel is at the largest colour distance from a candidate AND away from it -- the largest d an image gives.
CLAIMS = {
    'bc_8': lambda c: C.cell_block(c.S)[0] == 8, 'bc_2': lambda c: C.cell_block(c.S)[0] == 2,
    'bc_1': lambda c: C.cell_block(c.S)[0] == 1,
    'cand_full': lambda c: C.cell_block(c.S)[2] == C.SPX_MAX_CAND,
    'tile_20': _tile(20), 'tile_24': _tile(24), 'tile_30': _tile(30), 'tile_33': _tile(33), 'tile_48': _tile(48),
    'tile_64': lambda c: C.cell_block(c.S)[1] == C.SPX_MAX_T,
    'part_block': lambda c: any(g % C.cell_block(c.S)[0] for g in _grid(c)),
    'head': lambda c: bool(C.heads(*_shape(c), c.S) - {0}),
    'tail': lambda c: int(np.prod(_shape(c))) * 3 % 4 != 0,
    'm_1': lambda c: c.m == 1, 'm_64': lambda c: c.m == 64,
    'drop_keep': _drop_keep,
    'd_large': lambda c: max(int(d.max()) for _, d in _trace(c)) > 3 * 255 * 255 * c.S * c.S and c.S == c.m == 64,
    'min_area_1': lambda c: all(o.count == _areas(o).size and (o.regs > 0).all() for o in C.oracle(c.name)),
    'min_area_all': lambda c: all(c.min_area > _areas(o).max() and o.count == 0 and not o.regs.any() and _areas(o).size > 100
                                  for o in C.oracle(c.name)),
    'dim_max': lambda c: max(_shape(c)[1:]) == 16384,
    'chunks_gt_256': lambda c: C.chunk_count(*_shape(c)[1:]) > C.SCAN_THREADS,
    'one_cell_wide': lambda c: min(_grid(c)) == 1,
    'span_4': lambda c: all(C.tiles_crossed(o.roots, o.regs) >= 4 for o in C.oracle(c.name)),
    'ties_min': lambda c: all(_min_ties(d) > 0 for _, d in _trace(c)),
    'ties_any': lambda c: all(_any_ties(d) > 0 for _, d in _trace(c)),
    'grid_kept': lambda c: np.array_equal(C.oracle(c.name)[0].labels, R.grid_labels(*_shape(c)[1:], c.S)),
    'batch': lambda c: len(c.gens) > 1,
    'image_off_dword': lambda c: len(c.gens) > 1 and _shape(c)[1] * _shape(c)[2] * 3 % 4 != 0,
    'hw_ragged': lambda c: len(c.gens) > 1 and _shape(c)[1] * _shape(c)[2] % 256 != 0,
}
CLAIMS.update({'rotation_%d' % r: (lambda c, r=r: c.iters % 6 == r) for r in range(6)})


@pytest.mark.parametrize('name', [c.name for c in C.CASES])
def test_case_holds_what_it_is_named_for(name):
    c = C.BY_NAME[name]
    assert c.claims
    for claim in c.claims:
        assert CLAIMS[claim](c), (name, claim)
    N, H, W = _shape(c)
    assert all(img.shape == (H, W, 3) and img.dtype == np.uint8 for img in C.images(name))
    assert H % c.S == 0 and W % c.S == 0 and 4 <= c.S <= 64 and 1 <= c.m <= 64 and c.iters >= 1 and c.min_area >= 1
    for o in C.oracle(name):
        assert o.regs.dtype == np.int32 and o.count == int(o.regs.max())
    if name in C.RECORDED:
        count, dropped = C.RECORDED[name]
        o = C.oracle(name)[0]
        assert o.count == count and (dropped is None or int((o.regs == 0).sum()) == dropped)


def test_every_claim_is_made_by_a_case():
    made = {claim for c in C.CASES for claim in c.claims}
    assert made == set(CLAIMS), (made ^ set(CLAIMS))
    # the sweep runs the shortest INIT -> MID -> LAST chains and every residue of the buffer rotation
    assert {c.iters for c in C.CASES if c.name.startswith('iters')} == set(range(1, 8))
    # both 16384 cases, both orientations
    assert {_shape(c)[1:] for c in C.CASES if 'dim_max' in c.claims} == {(16384, 64), (64, 16384)}
    # every S the geometry treats differently: bc = 8, a tile narrower than 32 at bc > 1 and bc = 1, an odd S >= 32, 64
    assert {4, 5, 12, 20, 33, 48, 64} <= {c.S for c in C.CASES}
    # the images of a batch differ, and so do their region counts
    for name in C.BATCH_CASES:
        assert len({o.count for o in C.oracle(name)}) > 1, name
    # all four heads, and every tail, occur
    assert set().union(*(C.heads(*_shape(c), c.S) for c in C.CASES)) == {0, 1, 2, 3}
    assert {int(np.prod(_shape(c))) * 3 % 4 for c in C.CASES} == {0, 1, 2, 3}


def _restate(imgs, c):
    out = []
    for img in imgs:
        labels, centres = R.slic_labels(np.ascontiguousarray(img), c.S, c.m, c.iters)
        out.append((centres, R.number(R.components(labels), c.min_area)[0]))
    return out


def _differs(imgs, c):
    """Images of the restatement's result on `imgs` that differ from the case's oracle in the centres or the map."""
    return [i for i, ((centres, regs), o) in enumerate(zip(_restate(imgs, c), C.oracle(c.name)))
            if not (np.array_equal(centres, o.centres) and np.array_equal(regs, o.regs))]


def _decoded_without_head(imgs, S):
    """The pixels slic_iter_kernel would decode if it left `head` out: every staged tile row read from the start of the
    dword that holds its first byte."""
    a = np.stack(imgs)
    N, H, W, _ = a.shape
    flat, out, tile = a.reshape(-1), a.copy(), C.cell_block(S)[1]
    for n in range(N):
        for y in range(H):
            for x0 in range(0, W, tile):
                tw = min(tile, W - x0)
                s = (((n * H + y) * W + x0) * 3) & ~3
                out[n, y, x0:x0 + tw] = flat[s:s + 3 * tw].reshape(tw, 3)
    return out


def test_the_mistakes_the_cases_are_there_for_would_show():
    """Three mistakes restated in numpy, each on the cases named for the path: the restatement's result on what the
    kernel would then see differs from the oracle the GPU test compares with, so the case would fail."""
    # `head` left out of the LDS read: every image of every non-constant `head` case changes
    for name in ('s5', 's33_m1', 'batch3_s5', 'batch2_s33'):
        c = C.BY_NAME[name]
        assert 'head' in c.claims
        assert _differs(_decoded_without_head(C.images(name), c.S), c) == list(range(len(c.gens))), name
    # the buffer's last dword not assembled from its bytes but dropped (read as 0): the last pixel loses 1 .. 3 bytes
    for name, tail in (('s5', 1), ('s33_m1', 2), ('batch3_s5', 3)):
        c = C.BY_NAME[name]
        a = np.stack(C.images(name))
        assert 'tail' in c.claims and a.size % 4 == tail and a.reshape(-1)[-tail:].any()
        a.reshape(-1)[-tail:] = 0
        assert _differs(a, c) == [len(c.gens) - 1], name
    # `running` not carried between the passes of root_scan_kernel: the numbering restarts every 256 chunks, so a kept
    # root beyond the first pass gets another id -- there are such roots in every later pass
    for name in ('tall', 'wide'):
        o = C.oracle(name)[0]
        roots = np.flatnonzero((o.roots.reshape(-1) == np.arange(o.roots.size)) & (o.regs.reshape(-1) > 0))
        per_pass = np.bincount(roots // (C.SCAN_CHUNK * C.SCAN_THREADS), minlength=4)
        assert per_pass.size == 4 and (per_pass > 0).all(), (name, per_pass)
    # and per-image chunk offsets with `p < HW` guards: the images of a batch end inside a chunk and a 256-pixel block
    for name in C.BATCH_CASES:
        hw = C.images(name)[0].shape[0] * C.images(name)[0].shape[1]
        assert hw % C.SCAN_CHUNK and hw % C.SCAN_THREADS and C.chunk_count(*C.images(name)[0].shape[:2]) > 1


def test_restatement_matches_the_source():
    def const(name):
        return int(re.search(r'constexpr int (?:\w+ = \d+, )*%s = (\d+)[;,]' % name, SRC).group(1))
    assert const('SPX_TILE') == C.SPX_TILE and const('SPX_MAX_T') == C.SPX_MAX_T and const('CCL_T') == C.CCL_T
    assert const('SCAN_CHUNK') == C.SCAN_CHUNK and const('SPX_THREADS') == C.SCAN_THREADS
    assert const('SHR_T') == C.SHR_T and const('SHR_MAX_WIN') == C.SHR_MAX_WIN
    assert 'constexpr int SPX_MAX_CAND = (SPX_TILE / 4 + 2) * (SPX_TILE / 4 + 2);' in SRC
    assert (C.SPX_TILE // 4 + 2) ** 2 == C.SPX_MAX_CAND == C.cell_block(4)[2]
    assert 'const int bc = S >= SPX_TILE ? 1 : SPX_TILE / S;' in SRC
    assert 'for (int b0 = 0; b0 < chunks; b0 += SPX_THREADS) {' in SRC
    assert 'const int head = (int)(((((long long)n * H + y) * W + x0) * 3) & 3);' in SRC
    assert 'if (S < 4 || S > 64 || H > 16384 || W > 16384 || N > 65535) return RGDA_ERR_UNSUPPORTED;' in SRC
    assert [C.cell_block(s)[:2] for s in (4, 5, 8, 12, 16, 20, 32, 33, 64)] == [
        (8, 32), (6, 30), (4, 32), (2, 24), (2, 32), (1, 20), (1, 32), (1, 33), (1, 64)]
    assert max(C.SHRINK_WINS) == C.SHR_MAX_WIN


@pytest.mark.parametrize('name', [c.name for c in C.CASES if 'ties_any' in c.claims or 'd_large' in c.claims or c.name == 's5'])
def test_candidate_distances_agree_with_assign(name):
    """candidate_d (which the tie and size claims read) picks the labels superpixel_ref.assign picks: the first least d."""
    c = C.BY_NAME[name]
    img = C.images(name)[0]
    H, W, _ = img.shape
    gy, gx = np.mgrid[0:H, 0:W] // c.S
    trace = _trace(c)
    for centres, d in trace:
        slot = np.where(d < 0, np.iinfo(np.int64).max, d).argmin(0)            # argmin: the first, i.e. the smallest k
        k = (gy + slot // 3 - 1) * (W // c.S) + gx + slot % 3 - 1
        assert np.array_equal(k, R.assign(img, centres, c.S, c.m))
    o = C.oracle(name)[0]
    assert np.array_equal(trace[-1][0], o.centres) and np.array_equal(k, o.labels)


def test_constant_images_follow_the_tie_rule_at_even_and_odd_s():
    """Even S: Update's round-half-up puts the first centres at S g + S / 2, so the rows / columns S g + S are equally far
    from the cells g and g + 1 and go to the smaller k: the grid moved by one pixel.  Odd S: the centres sit on the
    middle pixel S g + (S - 1) / 2, no pixel is equally far from two nearest centres (equal d exists among the farther
    candidates only), and Assign returns the grid itself."""
    o = C.oracle('const_s4_i1')[0]
    cell = np.maximum(np.arange(32) - 1, 0) // 4
    assert np.array_equal(o.labels, cell[:, None] * 8 + cell[None, :])
    assert np.array_equal(o.regs, cell[:, None] * 8 + cell[None, :] + 1) and o.count == 64
    assert _min_ties(_trace(C.BY_NAME['const_s5_i1'])[0][1]) == 0
    for name in ('const_s5_i1', 'const_s5_i4'):
        o = C.oracle(name)[0]
        assert np.array_equal(o.regs, R.grid_labels(35, 35, 5) + 1) and o.count == 49


@pytest.mark.parametrize('name', [c.name for c in C.CASES
                                  if C.images(c.name)[0].shape[0] * C.images(c.name)[0].shape[1] < C.FLOOD_MAX_PIXELS])
def test_components_agree_with_the_flood_fill(name):
    c = C.BY_NAME[name]
    for o in C.oracle(name):
        comp, first, area = _flood(o.labels)
        assert np.array_equal(first[comp], o.roots)
        kept = area >= c.min_area
        want = np.zeros(len(first), np.int64)
        want[kept] = np.arange(1, int(kept.sum()) + 1)
        assert o.count == int(kept.sum()) and np.array_equal(o.regs, want[comp])


def test_int32_bound_is_asserted_over_the_existing_candidates_only():
    """A tall image one cell wide: the slots left and right of the only column do not exist, stand in as centre 0 and are
    as far as 4096 * 991^2 > 2^31 from the lower pixels.  They are no candidates; the call passes.  A centre that IS a
    candidate and too far still trips the assertion, in a grid one cell wide as in any other."""
    img = R.rectangle_scene(1024, 64, 2, count=8)
    centres = R.update(img, R.grid_labels(1024, 64, 64), 64)
    assert 64 * 64 * (1023 - int(centres[0, 0])) ** 2 >= 2 ** 31                    # what the slots outside would give
    labels, _ = R.slic_labels(img, 64, 64, 2)
    assert labels.shape == (1024, 64) and set(np.unique(labels)) <= set(range(16))
    labels, _ = R.slic_labels(np.ascontiguousarray(img.transpose(1, 0, 2)), 64, 64, 2)
    assert labels.shape == (64, 1024)
    for shape in ((128, 64), (64, 128), (128, 128)):
        H, W = shape
        img = C.constant_image(H, W)
        centres = R.update(img, R.grid_labels(H, W, 64), 64)
        R.assign(img, centres, 64, 64)                                              # in range: passes
        far = centres.copy()
        far[-1, :2] += 800                                  # the last cell's centre, a neighbour of every other cell
        assert 64 * 64 * 800 ** 2 >= 2 ** 31
        with pytest.raises(AssertionError):
            R.assign(img, far, 64, 64)


def test_shrink_cases():
    """The restatement on the shrink table: win = 0 is the identity; a window that covers the whole image leaves a map
    that is not constant all `fill`; the larger maps keep and drop pixels at every window, the largest included; every
    id of the palette occurs and the third `fill` is one of them."""
    assert {int(v) for s in C.SHRINK_SHAPES for v in np.unique(C.shrink_map(s))} == set(C.SHRINK_IDS)
    assert min(C.SHRINK_IDS) < 0 and max(C.SHRINK_IDS) == C.INT32_MAX
    for shape in C.SHRINK_SHAPES:
        regs = C.shrink_map(shape)
        assert regs.dtype == np.int32 and regs.shape == shape
        fills = C.shrink_fills(regs)
        assert fills[:2] == (0, -7) and fills[2] in regs and fills[3] == C.INT32_MIN
        for fill in fills:
            assert np.array_equal(C.shrink_oracle(shape, 0, fill), regs)
            for win in C.SHRINK_WINS[1:]:
                out = C.shrink_oracle(shape, win, fill)
                assert ((out == regs) | (out == fill)).all()
                N, H, W = shape
                for n in range(N):
                    if win >= max(H, W) - 1 and len(np.unique(regs[n])) > 1:
                        assert (out[n] == fill).all(), (shape, win)
                if H >= 64 and fill == C.INT32_MIN:
                    assert (out == regs).any() and (out == fill).any(), (shape, win)
    assert len(np.unique(C.shrink_map((1, 5, 7)))) > 1 and len(np.unique(C.shrink_map((1, 1, 70)))) > 1
