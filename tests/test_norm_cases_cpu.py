"""CPU: the case table of tests/norm_cases.py reaches every layout path it names, its restatement of the host-side layout
arithmetic still matches norm_kernels.hip, and the fixed-point accumulators of common.h, modelled in integers, turn an
out-of-range total into NaN instead of wrapping (the worked example: one channel of 2^18 rows of +-1024)."""
import math
import os
import re

import norm_cases as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = open(os.path.join(ROOT, 'regda_amd', 'csrc', 'norm_kernels.hip')).read()
COMMON = open(os.path.join(ROOT, 'regda_amd', 'csrc', 'common.h')).read()
HDR = open(os.path.join(ROOT, 'include', 'rgda_hip.h')).read()


def test_every_named_path_is_reached():
    reached = N.paths_reached()
    lines = ['%-28s %s' % (p, ', '.join(sorted(set(reached.get(p, []))))) for p in N.REQUIRED]
    print('\n'.join(lines))
    missing = [p for p in N.REQUIRED if not reached.get(p)]
    assert not missing, missing
    # and every case reaches what it claims to be there for
    for c in N.BN_CASES:
        got = {p for p, names in reached.items() if c.name in names}
        assert set(c.paths) <= got, (c.name, set(c.paths) - got)


def test_cases_are_valid_calls():
    for c in N.BN_CASES:
        assert c.C % 8 == 0 and c.pad % 8 == 0 and c.Mg % c.rpi == 0 and 1 <= c.G <= N.GROUPS_MAX and c.Mg >= 2, c
    for C, G, Mg, relu in N.SMALL:
        assert C % 8 == 0 and 1 <= G <= N.GROUPS_MAX and 2 <= Mg <= N.BN_SMALL_ROWS
    assert len(N.SMALL) > N.BN_SMALL_MAX


def _const(pattern, src=SRC):
    m = re.search(pattern, src)
    assert m, pattern
    return int(m.group(1))


def test_restatement_matches_the_source():
    assert _const(r'#define\s+RGDA_STAT_REPLICAS\s+(\d+)', HDR) == N.NREP
    assert _const(r'#define\s+RGDA_STAT_FRAC_FWD\s+(\d+)', HDR) == N.FRAC_FWD
    assert _const(r'#define\s+RGDA_STAT_FRAC_BWD\s+(\d+)', HDR) == N.FRAC_BWD
    # row_layout
    assert re.search(r'L\.vpr = C / 8;\s*int v = 1;\s*while \(v < L\.vpr && v < 256\) v <<= 1;\s*L\.vpb = v;\s*'
                     r'L\.rpb = 256 / v;', SRC)
    # the vpb cap in rgda_bn_stats, elementwise_grid and rgda_bn_bwd_reduce
    caps = re.findall(r'if \(L\.vpb > (\d+)\) \{ L\.vpb = (\d+); L\.rpb = (\d+); \}', SRC)
    assert len(caps) == 3 and all(tuple(map(int, c)) == (N.VPB_CAP,) * 3 for c in caps), caps
    # reduce_rows_per_block
    assert _const(r'long long want = (\d+) / ny;') == N.RED_WANT
    assert _const(r'long long minrows = \(long long\)L\.rpb \* (\d+);') == N.RED_MIN_ROWS_PER_LANE
    assert re.search(r'rows = \(rows \+ L\.rpb - 1\) / L\.rpb \* L\.rpb;', SRC)
    # the Mg clamp of rgda_bn_bwd_reduce: rows per block of the whole call, clamped to one group
    assert re.search(r'reduce_rows_per_block\(Mg \* groups, L\);\s*if \(rows_per_block > Mg\) rows_per_block = '
                     r'\(int\)\(\(Mg \+ L\.rpb - 1\) / L\.rpb \* L\.rpb\);', SRC)
    # elementwise_grid
    assert _const(r'int& bpg, dim3& grid,\s*int rows_mult = (\d+)\)') == N.EW_ROWS_MULT
    assert re.search(r'rows_per_block = L\.rpb \* rows_mult;', SRC)
    assert _const(r'cdiv\(M, rows_per_block\) \* groups \* cdiv\(L\.vpr, L\.vpb\) > (\d+)\) rows_per_block \*= 2;') == \
        N.EW_MAX_BLOCKS
    # the replica a reduction workgroup adds to (bn_stats, bn_bwd_reduce)
    assert len(re.findall(r'\(\(blockIdx\.x \+ blockIdx\.y \* gridDim\.x\) & \(NREP - 1\)\)', SRC)) == 2
    # the small-map kernels
    for name in ('BN_SMALL_RPT', 'BN_SMALL_LANES', 'BN_SMALL_CV', 'BN_SMALL_GP', 'BN_SMALL_MAX'):
        assert _const(r'constexpr int %s = (\d+);' % name) == getattr(N, name), name
    assert re.search(r'constexpr int BN_SMALL_ROWS = BN_SMALL_LANES \* BN_SMALL_RPT;', SRC)
    assert re.search(r'd\.groups > 8', SRC) and N.GROUPS_MAX == 8
    # the fixed-point accumulators: poison, range, and a total summed without wrapping, read as NaN out of range
    assert re.search(r'#define RGDA_STAT_POISON \(3ll << 60\)', COMMON) and N.STAT_POISON == 3 << 60
    assert re.search(r'if \(!\(fabsf\(x\) < 0x1p59f\)\) return RGDA_STAT_POISON;', COMMON)
    body = re.search(r'double stat_total\(.*?\n\}', COMMON, flags=re.S).group(0)
    assert '__int128 t = 0;' in body and '__builtin_nan' in body and '(1ll << 59)' in body


def _worked_example(total):
    """One channel of one group of 2^18 rows alternating +1024 / -1024, reduced as rgda_bn_stats reduces it:
    -> (mean, var) from `total` (stat_total or the 64-bit form)."""
    M, C = 1 << 18, 64
    rows, gx, gy = N.stats_grid(M, C)
    assert (rows, gx, gy) == (512, 512, 1)
    part_s, part_q = 0.0, float(rows) * 1024.0 ** 2        # every partial: 256 (+1024) and 256 (-1024) rows
    assert N.stat_fix(part_q, N.FRAC_FWD) == 1 << 55 < N.STAT_LIMIT   # each partial is in range
    reps_s, reps_q = [0] * N.NREP, [0] * N.NREP
    for b in range(gx):
        r = b & (N.NREP - 1)
        reps_s[r] = N.stat_add(reps_s[r], part_s, N.FRAC_FWD)
        reps_q[r] = N.stat_add(reps_q[r], part_q, N.FRAC_FWD)
    assert reps_q == [1 << 61] * N.NREP                     # no replica wraps: 64 partials of 2^55 each
    S, Q = total(reps_s, N.FRAC_FWD), total(reps_q, N.FRAC_FWD)
    mean = S / M
    return mean, Q / M - mean * mean


def test_fixed_point_totals_do_not_wrap():
    # the 64-bit sum of the eight replicas wraps 2^64 to exactly 0: var = 0, invstd = 1 / sqrt(eps) -- finite and wrong
    mean, var = _worked_example(N.stat_total_64)
    assert mean == 0.0 and var == 0.0
    # the library's form (128-bit sum of the replicas, NaN out of range): the channel's statistics are NaN
    mean, var = _worked_example(N.stat_total)
    assert mean == 0.0 and math.isnan(var)
    # in range, the totals are exact
    assert N.stat_total([N.stat_fix(1.5, N.FRAC_FWD)] * 8, N.FRAC_FWD) == 12.0
    # a single out-of-range or non-finite partial poisons; one poison reads out of range
    for v in (2.0 ** 33, float('inf'), float('nan')):
        assert N.stat_fix(v, N.FRAC_FWD) == N.STAT_POISON
        assert math.isnan(N.stat_total([N.stat_fix(v, N.FRAC_FWD)] + [0] * 7, N.FRAC_FWD))
    # k poisons in one replica wrap in 64 bits, but read out of range for every k that is not a multiple of 16
    for k in range(1, 40):
        r = 0
        for _ in range(k):
            r = N.stat_add(r, float('inf'), N.FRAC_FWD)
        assert math.isnan(N.stat_total([r] + [0] * 7, N.FRAC_FWD)) == (k % 16 != 0), k
    # the backward worked example (tests/test_norm_passes_gpu.py): 2^18 rows of g' xhat = 128, partials of 512 rows (2^56
    # fixed-point units each), replicas of 2^62 (no replica wraps), a total of 2^65
    rows, bpg, gx, gy = N.bwd_reduce_grid(1 << 18, 64, 1)
    assert rows == 512 and gx == 512
    reps = [0] * N.NREP
    for b in range(gx):
        reps[b & 7] = N.stat_add(reps[b & 7], 512 * 128.0, N.FRAC_BWD)
    assert reps == [1 << 62] * N.NREP
    assert N.stat_total_64(reps, N.FRAC_BWD) == 0.0 and math.isnan(N.stat_total(reps, N.FRAC_BWD))


def test_linear_pass_cases_are_valid_calls():
    """The spatial-map, group, sparse and classifier cases are calls the library accepts, and they reach what the tables
    say: both spatial_mix kernels, every spatial_mix_multi block width and several channel passes, the LDS limit of
    group_mix, ragged channel blocks."""
    assert {J >= 256 for (_, _, J, *_) in N.SPATIAL} == {True, False}
    assert any(acc and f32 for *_, acc, f32 in N.SPATIAL) and any(acc and not f32 for *_, acc, f32 in N.SPATIAL)
    widths = set()
    for Nn, I, Js, C, pad in N.SPATIAL_MULTI:
        assert 1 <= len(Js) <= 4 and sum(Js) <= N.SPATIAL_MULTI_MAX_J and C % 8 == 0
        cvb = 256 if C // 8 >= 256 else 128 if C // 8 >= 128 else 64 if C // 8 >= 64 else 32
        widths.add(cvb)
        if C // 8 > cvb:
            widths.add('passes')
    assert widths == {256, 128, 64, 32, 'passes'}, widths
    for G, I, J, C, pad, in32, out32 in N.GROUP:
        assert J * 64 * 8 * (4 if in32 else 2) <= 150 * 1024      # launch_group_mix: the staged slab
    assert {(c[5], c[6]) for c in N.GROUP} == {(False, False), (True, True), (True, False), (False, True)}
    assert any(c[1] % 2 for c in N.GROUP) and any((c[3] // 8) % 64 for c in N.GROUP)
    for Nn, Js, rows, C, *_ in N.SPARSE:
        assert 1 <= len(Js) <= 4 and 1 <= len(rows) <= 4 and C % 8 == 0 and sum(rows) > 13      # a row of 13 entries: the 8-, 4- and 1-entry loops
    for Nn, HW, C, nc, pad in N.CLASSIFIER:
        assert 6 <= nc <= 16 and C % 8 == 0
    assert any((Nn * HW) % 64 for Nn, HW, *_ in N.CLASSIFIER)
