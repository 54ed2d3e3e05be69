"""The HBM-bound passes of regda_amd/csrc/norm_kernels.hip (BatchNorm, the small-map BatchNorm, max-pool, InstanceNorm;
the spatial maps and the classifier are not in the table yet): a Python restatement of the host-side layout arithmetic that decides how a call is cut
into workgroups, a table of cases that each name the layout path they are there to reach, and the fp64 references and
per-element bounds the GPU tests check them with.

The restatement mirrors norm_kernels.hip; tests/test_norm_cases_cpu.py parses the constants it copies out of the source,
so a change there that is not made here fails on a machine without a GPU.  The checks reuse U, U32 and
stat_violations of tests/conv_routes.py; stat_violations gets the partial size of THESE kernels (PARTIAL_ROWS there was
derived for convolution tiles).
"""
from collections import namedtuple

from conv_routes import U, U32, stat_violations  # noqa: F401  (re-exported for the tests)

# ---------------------------------------------------------------- the restatement (norm_kernels.hip, common.h)
NREP = 8                    # RGDA_STAT_REPLICAS (include/rgda_hip.h); a workgroup adds to replica (bx + by * gx) & 7
VPB_CAP = 16                # `if (L.vpb > 16) { L.vpb = 16; L.rpb = 16; }`: rgda_bn_stats, elementwise_grid, rgda_bn_bwd_reduce
RED_WANT = 512              # reduce_rows_per_block: `long long want = 512 / ny`
RED_MIN_ROWS_PER_LANE = 4   # reduce_rows_per_block: `minrows = (long long)L.rpb * 4`
EW_ROWS_MULT = 8            # elementwise_grid: `int rows_mult = 8`, rows_per_block = rpb * 8
EW_MAX_BLOCKS = 8192        # elementwise_grid: rows_per_block doubles while a launch would exceed 8192 workgroups
GROUPS_MAX = 8              # rgda_bn_train_apply, rgda_bn_train_small, rgda_bn_bwd_small: groups <= 8
BN_SMALL_RPT = 5            # rows per thread
BN_SMALL_LANES = 64         # row lanes
BN_SMALL_CV = 8             # channel vectors (of 8 channels) per workgroup
BN_SMALL_GP = 2             # groups resident at a time
BN_SMALL_MAX = 8            # descriptors per launch
BN_SMALL_ROWS = BN_SMALL_LANES * BN_SMALL_RPT       # 320: the most rows of one group the small kernels take
FRAC_FWD, FRAC_BWD = 26, 40
STAT_POISON = 3 << 60       # RGDA_STAT_POISON (common.h)
STAT_LIMIT = 1 << 59        # |partial| and |total| must stay below 2^59 fixed-point units

Layout = namedtuple('Layout', 'vpr vpb rpb')


def cdiv(a, b):
    return -(-a // b)


def row_layout(C, cap=True):
    """row_layout(): vpr = C / 8 vectors per row, vpb = the next power of two (<= 256), rpb = 256 / vpb row lanes; the
    statistics, apply and backward passes cap vpb at 16 (128 channels per workgroup)."""
    vpr = C // 8
    v = 1
    while v < vpr and v < 256:
        v <<= 1
    if cap and v > VPB_CAP:
        return Layout(vpr, VPB_CAP, VPB_CAP)
    return Layout(vpr, v, 256 // v)


def reduce_rows_per_block(M, L):
    """reduce_rows_per_block(): ~512 workgroups per channel block column, at least 4 rows per row lane, a multiple of rpb."""
    ny = cdiv(L.vpr, L.vpb)
    want = max(RED_WANT // ny, 1)
    rows = cdiv(M, want)
    rows = max(rows, L.rpb * RED_MIN_ROWS_PER_LANE)
    return cdiv(rows, L.rpb) * L.rpb


def stats_grid(M, C):
    """rgda_bn_stats -> (rows_per_block, gx, gy)."""
    L = row_layout(C)
    rpb = reduce_rows_per_block(M, L)
    return rpb, cdiv(M, rpb), cdiv(L.vpr, L.vpb)


def bwd_reduce_grid(M, C, groups):
    """rgda_bn_bwd_reduce -> (rows_per_block, blocks per group, gx, gy): the rows per block of the WHOLE call, clamped to
    one group's rows (`if (rows_per_block > Mg) rows_per_block = round_up(Mg, rpb)`)."""
    L = row_layout(C)
    Mg = M // groups
    rpb = reduce_rows_per_block(Mg * groups, L)
    if rpb > Mg:
        rpb = cdiv(Mg, L.rpb) * L.rpb
    bpg = cdiv(Mg, rpb)
    return rpb, bpg, bpg * groups, cdiv(L.vpr, L.vpb)


def elementwise_grid(Mg, C, groups):
    """elementwise_grid() (rgda_bn_apply, rgda_bn_train_apply, rgda_bn_bwd_apply) -> (rows_per_block, blocks per group,
    gx, gy, doubled)."""
    L = row_layout(C)
    rows = L.rpb * EW_ROWS_MULT
    base = rows
    while cdiv(Mg, rows) * groups * cdiv(L.vpr, L.vpb) > EW_MAX_BLOCKS:
        rows *= 2
    bpg = cdiv(Mg, rows)
    return rows, bpg, bpg * groups, cdiv(L.vpr, L.vpb), rows > base


def replicas(gx, gy):
    """Partials per replica of a reduction grid (bn_stats, bn_bwd_reduce): workgroup (bx, by) adds to (bx + by gx) & 7."""
    n = [0] * NREP
    for by in range(gy):
        for bx in range(gx):
            n[(bx + by * gx) & (NREP - 1)] += 1
    return n


def straddles(Mg, rows_per_block, rows_per_image):
    """The Dropout2d scale index r / rows_per_image changes inside some chunk of a group: an image boundary (a multiple of
    rows_per_image) lies strictly inside a chunk (b, b + rows_per_block)."""
    for b in range(0, Mg, rows_per_block):
        e = min(b + rows_per_block, Mg)
        if (b // rows_per_image + 1) * rows_per_image < e:
            return True
    return False


def small_launches(n):
    """rgda_bn_train_small / one gate kind of rgda_bn_bwd_small: descriptors per launch."""
    return [min(BN_SMALL_MAX, n - i) for i in range(0, n, BN_SMALL_MAX)]


# ---------------------------------------------------------------- fixed-point accumulators, as integers (common.h)
def wrap64(v):
    v &= (1 << 64) - 1
    return v - (1 << 64) if v >> 63 else v


def stat_fix(v, frac):
    """stat_fix(): round(v * 2^frac), or the poison where that is out of range or not finite (v a Python float that is
    already an fp32 value; the scaling by a power of two is exact)."""
    x = v * 2.0 ** frac
    if not abs(x) < 2.0 ** 59:
        return STAT_POISON
    return int(round(x))


def stat_add(replica, v, frac):
    """stat_add(): the 64-bit integer atomic (wraps)."""
    return wrap64(replica + stat_fix(v, frac))


def stat_total(reps, frac):
    """stat_total(): the replicas summed WITHOUT wrapping (128-bit), a total of magnitude >= 2^59 read as NaN."""
    t = sum(reps)
    return float('nan') if abs(t) >= STAT_LIMIT else t * 2.0 ** -frac


def stat_total_64(reps, frac):
    """The form before the fix: the replicas summed in 64 bits (wrapping), then the range check."""
    t = 0
    for r in reps:
        t = wrap64(t + r)
    return float('inf') if abs(t) >= STAT_LIMIT else t * 2.0 ** -frac


# ---------------------------------------------------------------- the cases
# BatchNorm (general kernels): Mg rows per group, groups G, images of `rpi` rows (Mg % rpi == 0, the Dropout2d scale is
# per image), `pad` added to the row stride of EVERY operand (x, res, y, g, dx, gmask, act_out), relu / res / nscale of the
# forward apply, `modes` the backward ReLU gates: 0 (none), 'y' (relu 1, sign from y), 'mask' (relu 1, the sign mask),
# 2 (recomputed from x, with act_out).  `paths`: what the case is there to reach (tests/test_norm_cases_cpu.py checks it).
BnCase = namedtuple('BnCase', 'name C G Mg rpi pad relu res nscale modes paths')
BN_CASES = [
    BnCase('replicas8', 64, 1, 1 << 18, 128 * 128, 0, 1, False, True, ('mask',),
           ('all_replicas', 'groups_1')),
    BnCase('doubling', 2048, 2, 33280, 1040, 0, 0, True, False, (0,),
           ('doubling', 'C_2048', 'groups_2')),
    BnCase('c8', 8, 3, 2652, 221, 8, 1, True, True, ('y', 'mask', 2),
           ('C_8', 'vpr_1', 'straddle', 'groups_3', 'strided', 'ragged_chunk', 'relu_1_y', 'relu_1_mask',
            'relu_2')),
    BnCase('c24', 24, 8, 663, 221, 8, 1, True, True, (0, 'y', 'mask', 2),
           ('C_24', 'vpr_npot', 'straddle', 'groups_8', 'strided', 'ragged_chunk', 'relu_0', 'relu_1_y', 'relu_1_mask',
            'relu_2')),
    BnCase('c72', 72, 2, 884, 221, 16, 1, True, True, (0, 'y', 2),
           ('C_72', 'straddle', 'ragged_chunk', 'groups_2', 'strided', 'relu_2')),
    BnCase('c264', 264, 1, 1768, 221, 8, 1, False, True, ('mask', 2),
           ('C_264', 'ragged_cblock', 'straddle', 'ragged_chunk', 'strided', 'groups_1')),
]

# Small-map BatchNorm: descriptors (C, G, rows per group, relu).  One forward call takes all of them (more than
# BN_SMALL_MAX: two launches); the backward call takes every relu-1 descriptor twice, gated by y and by the sign mask,
# and the relu-0 ones once (they go with the mask launch): more than BN_SMALL_MAX of each gate kind.
SMALL = [
    (512, 2, 36, 1), (512, 8, 2, 1), (64, 3, 320, 1), (72, 1, 319, 0), (8, 5, 4, 1), (512, 2, 288, 1),
    (136, 3, 319, 1), (64, 8, 320, 0), (24, 1, 2, 1), (256, 4, 9, 1), (72, 7, 64, 1),
]

# max-pool 3x3 / 2 / pad 1: (N, H, W, C); with BatchNorm + ReLU on the operand path: (N, H, W, C, groups)
POOL = [(3, 17, 13, 72), (2, 16, 16, 8), (1, 9, 33, 264)]
POOL_BNIN = [(4, 17, 13, 64, 2), (2, 16, 15, 24, 1)]
# InstanceNorm: (N, HW, C, pad)
INORM = [(3, 221, 72, 8), (2, 4096, 64, 0), (1, 33, 8, 16)]


def paths_reached():
    """{path: [case names]} according to the restatement -- what tests/test_norm_cases_cpu.py lists and checks."""
    out = {}

    def add(p, name):
        out.setdefault(p, []).append(name)
    for c in BN_CASES:
        M = c.Mg * c.G
        rows, gx, gy = stats_grid(M, c.C)
        if min(replicas(gx, gy)) >= 2:
            add('all_replicas', c.name)
        rb, bpg, gx2, gy2 = bwd_reduce_grid(M, c.C, c.G)
        if min(replicas(gx2, gy2)) >= 2:
            add('all_replicas_bwd', c.name)
        erows, ebpg, _, egy, doubled = elementwise_grid(c.Mg, c.C, c.G)
        if doubled:
            add('doubling', c.name)
        if c.Mg % erows:
            add('ragged_chunk', c.name)
        L = row_layout(c.C)
        if L.vpr > L.vpb and L.vpr % L.vpb:
            add('ragged_cblock', c.name)
        if L.vpr == 1:
            add('vpr_1', c.name)
        if L.vpr < 16 and L.vpr & (L.vpr - 1):
            add('vpr_npot', c.name)
        if c.nscale and straddles(c.Mg, erows, c.rpi):
            add('straddle', c.name)
        add('C_%d' % c.C, c.name)
        add('groups_%d' % c.G, c.name)
        if c.pad:
            add('strided', c.name)
        for m in c.modes:
            add({0: 'relu_0', 'y': 'relu_1_y', 'mask': 'relu_1_mask', 2: 'relu_2'}[m], c.name)
    for C, G, Mg, relu in SMALL:
        add('small_rows_%d' % Mg, 'small')
        if G % 2:
            add('small_odd_groups', 'small')
        if C % (BN_SMALL_CV * 8):
            add('small_ragged_cblock', 'small')
        if not relu:
            add('small_bwd_relu_0', 'small')
    if len(small_launches(len(SMALL))) > 1:
        add('small_fwd_multi_launch', 'small')
    n1 = sum(1 for d in SMALL if d[3])
    if n1 > BN_SMALL_MAX:
        add('small_bwd_y_multi_launch', 'small')
    if n1 + sum(1 for d in SMALL if not d[3]) > BN_SMALL_MAX:
        add('small_bwd_mask_multi_launch', 'small')
    return out


# every path the table has to reach
REQUIRED = ['all_replicas', 'all_replicas_bwd', 'doubling', 'ragged_chunk', 'ragged_cblock', 'C_8', 'C_24', 'C_72',
            'C_264', 'C_2048', 'vpr_1', 'vpr_npot', 'straddle', 'groups_1', 'groups_2', 'groups_3', 'groups_8', 'strided',
            'relu_0', 'relu_1_y', 'relu_1_mask', 'relu_2', 'small_rows_2', 'small_rows_319', 'small_rows_320',
            'small_odd_groups', 'small_ragged_cblock', 'small_bwd_relu_0', 'small_fwd_multi_launch',
            'small_bwd_y_multi_launch', 'small_bwd_mask_multi_launch']


# ---------------------------------------------------------------- bounds (torch tensors, float64)
def moment_bounds(S, Q, n, dS, dQ, eps=1e-5):
    """Error bounds of (mean, var, invstd) formed from sums S, Q of n rows that err by at most dS, dQ:
        mean = S / n                    |d mean| <= dS / n
        var  = Q / n - mean^2           |d var|  <= dQ / n + (2 |mean| + |d mean|) |d mean|
        invstd = (var + eps)^-1/2       |d invstd| / invstd <= |d var| / (2 (var + eps - |d var|))  (where positive)
    plus the final fp32 roundings of each (a few 2^-24 relative), and the fp32 cancellation of E[x^2] - mean^2 when it
    is formed in fp32 (4 2^-24 (Q / n + mean^2))."""
    mean = S / n
    var = (Q / n - mean * mean).clamp_min(0)
    dm = dS / n + 2 * U32 * mean.abs()
    dv = dQ / n + (2 * mean.abs() + dm) * dm + 4 * U32 * (Q.abs() / n + mean * mean)
    den = (var + eps - dv).clamp_min(eps / 2)
    rel = dv / (2 * den) + 4 * U32
    return mean, var, (var + eps).rsqrt(), dm, dv, rel


# ---------------------------------------------------------------- the linear passes: spatial maps and the classifier
# rgda_spatial_mix: (N, I, J, C, pad, accumulate, out_f32).  J >= 256 takes the 8-vector x 32-slice kernel that walks a
# row's nonzero span, J < 256 the 32-vector x 8-slice one; C = 72 and 264 leave a ragged last channel block of both.
SPATIAL_MIX_SLICES = {True: 32, False: 8}               # J >= 256: 256 / 8 slices; else 256 / 32
SPATIAL = [(2, 6, 1024, 72, 8, False, False), (3, 36, 256, 264, 0, True, False), (2, 33, 36, 264, 16, False, True),
           (1, 17, 9, 72, 8, True, True), (2, 2, 255, 8, 8, True, False)]
# rgda_spatial_mix_multi: (N, I, [J of each source], C, pad): 1..4 sources, total J <= 1024, every channel-vector block
# width (C / 8 >= 256, 128, 64, else 32) and several passes over the channel blocks (C = 4160: 520 vectors, 3 passes)
SPATIAL_MULTI_MAX_J = 1024
SPATIAL_MULTI = [(2, 12, [1, 4, 9, 36], 512, 8), (1, 7, [450], 4160, 0), (3, 5, [36, 9], 72, 16), (2, 3, [1000, 24], 1024, 8)]
# rgda_group_mix: (G, I, J, C, pad, in_f32, out_f32): odd I (the last row of a row pair alone), C = 520 (65 vectors: a
# second block of one vector); J <= 75 for fp32 inputs (the staged slab must fit 150 KB of LDS)
GROUP = [(3, 9, 36, 520, 8, False, False), (2, 36, 9, 512, 0, True, True), (4, 5, 75, 72, 16, True, False),
         (1, 64, 144, 264, 8, False, True)]
# rgda_sparse_mix: (N, [J of each source], [rows per image of each output], C, pad, in_f32, out_f32); rows get 0 .. 20
# entries (the 8-, 4- and 1-entry loops and their tails)
SPARSE = [(2, [36, 9, 4, 1], [6, 6, 12, 6], 520, 8, False, False), (3, [64], [17], 72, 0, True, True),
          (1, [20, 13], [9, 4, 3], 264, 16, False, True)]
# rgda_classifier_fwd / _bwd: (N, HW, C, ncls, pad): ragged row counts (not multiples of 64), C from 8 to 2048
CLASSIFIER = [(3, 221, 72, 6, 8), (2, 4096, 2048, 7, 0), (1, 77, 8, 16, 8), (2, 130, 264, 6, 16)]
