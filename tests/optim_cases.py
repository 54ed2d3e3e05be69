"""The optimizer, weight-layout and step-chore kernels of regda_amd/csrc/optim_kernels.hip: a Python restatement of the
host-side grid arithmetic of every entry point, a table of cases that each name the path they are there to reach, and the
references the GPU tests (tests/test_optim_passes_gpu.py) check them with.

The restatement mirrors optim_kernels.hip; tests/test_optim_cases_cpu.py parses the constants it copies out of the source,
so a change there that is not made here fails on a machine without a GPU.

References.  Everything but the SGD step and the gradient norm is EXACT and compared bit for bit: bf16 round-to-nearest-
even (written here in integers), permutes / slices / zero padding, ONE fp32 add (IEEE, as torch does it), the sequential
fp32 sum in rank order, SplitMix64 in 64-bit integers.  The SGD step is computed in fp64 from its definition (torch's
clip_grad_norm_ and SGD, regda/utils/ema.py) with a bound per element that counts fp32 roundings; the one modelled
rounding point is `coef`, formed in fp32 on the host from the norm word the kernel read (coef_fp32).  Works on CPU and
GPU tensors alike (the cap cases are too large for a CPU reference to be quick).
"""
import math
from collections import namedtuple

import numpy as np
import torch

U32 = 2.0 ** -24            # unit roundoff of fp32 (round to nearest)


def gamma(k):
    """k fp32 roundings, first order and all higher ones: k u / (1 - k u) (Higham, Accuracy and Stability, lemma 3.1)."""
    return k * U32 / (1 - k * U32)


def cdiv(a, b):
    return -(-a // b)


# ---------------------------------------------------------------- the restatement (optim_kernels.hip, rgda_hip.h)
THREADS = 256
SUMSQ_PER_BLOCK, SUMSQ_CAP = 256 * 16, 1024          # rgda_sumsq: min(cdiv(n, 256 * 16), 1024)
SGD_VEC_PER_BLOCK, SGD_CAP = 256 * 4, 4096           # rgda_sgd_step: min(cdiv(n >> 2, 256 * 4), 4096)
CAST_PER_BLOCK, CAST_CAP = 256 * 16, 4096            # rgda_cast_bf16: min(cdiv(n, 256 * 16), 4096)
CASTF32_PER_BLOCK, CASTF32_CAP = 256 * 8, 4096       # rgda_cast_f32: min(cdiv(n, 256 * 8), 4096)
DDP_VEC, DDP_CAP = 8, 2048                           # rgda_ddp_accumulate_bf16: min(cdiv(shard >> 3, 256), 2048)
FILL_VEC_PER_BLOCK, FILL_CAP = 256 * 4, 4096         # rgda_fill_zero: min(cdiv(max(n16, 1), 256 * 4), 4096)
COPY_VEC_PER_BLOCK, COPY_CAP, COPY_MAX_JOBS = 256 * 4, 2048, 4      # rgda_copy_multi, per job
DROPOUT_CAP = 1024                                   # rgda_dropout_mask: min(cdiv(n, 256), 1024)
ADD_CAP = 8192                                       # rgda_add_bf16: min(cdiv(M * (C / 8), 256), 8192)
LAYOUT_TILE = 64                                     # RGDA_LAYOUT_TILE (include/rgda_hip.h)
LAYOUT_LDS_ROWS = 1024                               # NFB: tables of more rows search first_block in global memory
LAYOUT_SRC16 = 16                                    # mode bit 4: the source is bf16


def sumsq_blocks(n):
    return min(cdiv(n, SUMSQ_PER_BLOCK), SUMSQ_CAP)


def sgd_blocks(n):
    return min(cdiv(n >> 2, SGD_VEC_PER_BLOCK), SGD_CAP)


def cast_bf16_blocks(n):
    return min(cdiv(n, CAST_PER_BLOCK), CAST_CAP)


def cast_f32_blocks(n):
    return min(cdiv(n, CASTF32_PER_BLOCK), CASTF32_CAP)


def ddp_blocks(shard):
    return min(cdiv(shard >> 3, THREADS), DDP_CAP)


def fill_blocks(nbytes):
    return min(cdiv(max(nbytes >> 4, 1), FILL_VEC_PER_BLOCK), FILL_CAP)


def copy_first(sizes):
    """rgda_copy_multi: first[k] = the first workgroup of job k, first[n..4] = the grid size."""
    first, blocks = [], 0
    for b in sizes:
        first.append(blocks)
        blocks += min(cdiv(max(b >> 4, 1), COPY_VEC_PER_BLOCK), COPY_CAP)
    return first + [blocks] * (COPY_MAX_JOBS + 1 - len(sizes))


def dropout_blocks(n):
    return min(cdiv(n, THREADS), DROPOUT_CAP)


def add_blocks(M, C):
    return min(cdiv(M * (C // 8), THREADS), ADD_CAP)


def pad_blocks(R, K, Kp):
    """(rgda_pad_cast_bf16, rgda_unpad_acc_f32): one thread per destination element, no cap."""
    return cdiv(R * Kp, THREADS), cdiv(R * K, THREADS)


def loops(work, per_block_pass, blocks):
    """A grid-stride loop goes round more than once for some lane."""
    return work > blocks * per_block_pass


def layout_blocks(Co, Ci, T):
    """Blocks a table row owns: ceil(Ci / 64) ceil(Co / 64) T."""
    return cdiv(Ci, LAYOUT_TILE) * cdiv(Co, LAYOUT_TILE) * T


# a row of a layout table: the source is a [Co][T][ld] tensor (fp32, or bf16 with src16) read from element `off` of its
# rows, the destination a bf16 tensor in `mode` order placed `dst_off` elements past a 16-byte boundary
LayoutRow = namedtuple('LayoutRow', 'Co T Ci ld off mode src16 dst_off')


def layout_fallback_reasons(r):
    """Why a row leaves the vectorised path (the `vec` predicate of weight_transpose_batched_kernel); sources and
    destinations are placed on 16-byte boundaries before `off` / `dst_off` are applied."""
    why = []
    if r.Ci & 3:
        why.append('Ci')
    if r.ld & 3:
        why.append('ld')
    if (r.off * (2 if r.src16 else 4)) & (7 if r.src16 else 15):
        why.append('srcalign')
    if (r.dst_off * 2) & 7:
        why.append('dstalign')
    if r.mode == 0 and r.Co & 3:
        why.append('Co_mode0')
    return why


def layout_dst_shape(r):
    return {0: (r.Ci, r.T, r.Co), 1: (r.T, r.Co, r.Ci), 2: (r.Co, r.T, r.Ci)}[r.mode]


def layout_first_blocks(rows):
    first, blk = [], 0
    for r in rows:
        first.append(blk)
        blk += layout_blocks(r.Co, r.Ci, r.T)
    return first, blk


# ---------------------------------------------------------------- the cases
K = 1029                                     # 4 K + t: two workgroups of rgda_sumsq, the second ragged
SUMSQ_N = [1, 2, 3, 4, 4 * K + 1, 4 * K + 2, 4 * K + 3, SUMSQ_PER_BLOCK * SUMSQ_CAP + 3 * SUMSQ_PER_BLOCK + 7]

# rgda_sgd_step.  `first`: first_step; the gradient is gsig * N(0, 1) per element (0: all zero), so its norm is about
# gsig sqrt(n) and `clip` says which side of max_norm the AVERAGED norm gscale gsig sqrt(n) lies on; `bufs`: which of the
# optional buffers are present: 'all' (shadow, p_bf16, shadow_bf16), 'noshadow' (p_bf16 only), 'nosb' (shadow and p_bf16),
# 'nopb' (shadow and shadow_bf16).  lr and momentum are the training recipe's.
SgdCase = namedtuple('SgdCase', 'name n first gscale wd ema max_norm gsig clip bufs paths')
SGD_LR, SGD_MOMENTUM = 0.01, 0.9
RAGGED = 4 * (2 * SGD_VEC_PER_BLOCK + 37)
SGD_CASES = [
    SgdCase('n4', 4, True, 1.0, 5e-4, 0.99, 32.0, 1.0, 'inactive', 'all', ('sgd_one_block', 'sgd_first')),
    SgdCase('block', 1024, False, 0.5, 5e-4, 0.999, 1.0, 3.0, 'active', 'all',
            ('sgd_one_block', 'sgd_full_block', 'sgd_not_first', 'sgd_clip_active', 'sgd_gscale_0.5', 'sgd_ema_0.999')),
    SgdCase('block_first', 1024, True, 0.125, 5e-4, 0.99, 1e4, 3.0, 'inactive', 'all',
            ('sgd_first', 'sgd_clip_inactive', 'sgd_gscale_0.125', 'sgd_wd')),
    SgdCase('ragged_first', RAGGED, True, 0.125, 0.0, 0.0, 2.0, 3.0, 'active', 'all',
            ('sgd_ragged', 'sgd_first', 'sgd_clip_active', 'sgd_gscale_0.125', 'sgd_wd_0', 'sgd_ema_0')),
    SgdCase('ragged', RAGGED, False, 0.5, 5e-4, 0.99, 1e4, 3.0, 'inactive', 'noshadow',
            ('sgd_ragged', 'sgd_not_first', 'sgd_clip_inactive', 'sgd_no_shadow')),
    SgdCase('zero_grad', 1200, False, 1.0, 5e-4, 0.99, 32.0, 0.0, 'zero', 'nosb',
            ('sgd_zero_grad', 'sgd_no_sb', 'sgd_one_block')),
    SgdCase('tiny_norm', 1200, True, 1.0, 0.0, 0.999, 1e-5, 2e-5 / math.sqrt(1200), 'tiny', 'nopb',
            ('sgd_tiny_norm', 'sgd_no_pb')),
    SgdCase('ema0', 4 * (SGD_VEC_PER_BLOCK + 3), False, 1.0, 0.0, 0.0, 32.0, 3.0, 'active', 'all',
            ('sgd_ema_0', 'sgd_ragged', 'sgd_gscale_1')),
    SgdCase('cap', 4 * (SGD_VEC_PER_BLOCK * SGD_CAP + SGD_VEC_PER_BLOCK + 5), False, 0.5, 5e-4, 0.99, 32.0, 3.0, 'active',
            'all', ('sgd_cap', 'sgd_not_first', 'sgd_clip_active', 'sgd_wd')),
]

CAST_N = [1, 2, 3, 4, 4 * K + 1, 4 * K + 2, 4 * K + 3, CAST_PER_BLOCK * CAST_CAP + CAST_PER_BLOCK + 3]
CASTF32_N = [1, 7, 2 * CASTF32_PER_BLOCK + 5, CASTF32_PER_BLOCK * CASTF32_CAP + CASTF32_PER_BLOCK + 3]

# rgda_ddp_accumulate_bf16: (world, shard elements, order-dependent triples planted)
DDP_CASES = [(1, 8, False), (2, 8, False), (3, 8, True), (8, 8, True), (3, 8 * 259, True), (8, 8 * 1031, True),
             (2, 8 * (THREADS * DDP_CAP + THREADS + 3), False), (1, 8 * 300, False)]
ORDER_TRIPLE = (256.0, -256.0, 2.0 ** -20)      # ascending: 2^-20; descending: 0 (2^-20 is below half an ulp of 256)

# rgda_weight_transpose_batched: tables of rows (Co, T, Ci, ld, off, mode, src16, dst_off)
_VEC_ROWS = [
    LayoutRow(64, 1, 64, 64, 0, 0, False, 0), LayoutRow(96, 9, 64, 200, 4, 1, False, 0),
    LayoutRow(130, 1, 96, 104, 4, 2, True, 0), LayoutRow(4, 9, 4, 4, 0, 0, True, 0),
    LayoutRow(7, 1, 64, 64, 0, 1, False, 0), LayoutRow(65, 9, 4, 12, 4, 2, False, 0),
    LayoutRow(1, 1, 4, 4, 0, 1, True, 0), LayoutRow(64, 9, 96, 96, 0, 0, True, 0),
    LayoutRow(63, 1, 64, 68, 4, 1, True, 0), LayoutRow(96, 1, 132, 132, 0, 0, False, 0),
    LayoutRow(130, 9, 4, 4, 0, 2, False, 4), LayoutRow(6, 9, 64, 64, 0, 2, True, 0),
]
_FALLBACK_ROWS = [
    LayoutRow(64, 1, 63, 63, 0, 0, False, 0), LayoutRow(65, 9, 7, 8, 0, 1, True, 0),
    LayoutRow(96, 1, 130, 132, 0, 2, False, 0), LayoutRow(64, 1, 64, 66, 0, 1, False, 0),
    LayoutRow(4, 9, 4, 6, 0, 0, True, 0), LayoutRow(64, 1, 64, 72, 1, 2, False, 0),
    LayoutRow(96, 1, 64, 72, 2, 0, False, 0), LayoutRow(64, 9, 4, 8, 1, 1, True, 0),
    LayoutRow(63, 1, 64, 72, 2, 2, True, 0), LayoutRow(64, 1, 64, 64, 0, 2, False, 1),
    LayoutRow(4, 1, 64, 64, 0, 1, True, 2), LayoutRow(96, 1, 64, 64, 0, 0, False, 3),
    LayoutRow(7, 1, 64, 64, 0, 0, False, 0), LayoutRow(6, 9, 64, 64, 0, 0, True, 0),
    LayoutRow(130, 1, 4, 4, 0, 0, False, 0), LayoutRow(1, 1, 1, 1, 0, 0, False, 0),
    LayoutRow(1, 1, 1, 1, 0, 1, True, 0), LayoutRow(1, 9, 1, 3, 1, 2, False, 0),
    LayoutRow(130, 9, 65, 65, 0, 1, False, 0), LayoutRow(7, 9, 7, 7, 0, 0, True, 0),
]
LAYOUT_TABLES = {
    'vec': _VEC_ROWS,
    'fallback': _FALLBACK_ROWS,
    'mixed': [r for pair in zip(_VEC_ROWS, _FALLBACK_ROWS) for r in pair] + _FALLBACK_ROWS[len(_VEC_ROWS):],
    'rows1025': [LayoutRow(4, 1, 4, 4, 0, i % 3, bool((i // 3) & 1), 0) for i in range(LAYOUT_LDS_ROWS + 1)],
}

# rgda_pad_cast_bf16 / rgda_unpad_acc_f32: (R, K, Kp): the stem's, a ragged one, one without padding
PAD_CASES = [(64, 147, 192), (5, 13, 24), (3, 37, 37)]

FILL_BYTES = [0, 1, 15, 16, 16 * K + 5, 16 * (FILL_VEC_PER_BLOCK * FILL_CAP + FILL_VEC_PER_BLOCK + 3) + 6]
FILL_DTYPES = ['uint8', 'bfloat16', 'int64']

# rgda_copy_multi: byte sizes of the jobs of one call
COPY_BIG = 16 * (COPY_VEC_PER_BLOCK * COPY_CAP + COPY_VEC_PER_BLOCK + 9)
COPY_CASES = [[16], [16 * 1030, 16], [16, 16 * 2051, 16 * 5], [16 * 1025, 16, 16 * 4097, 16 * 3], [COPY_BIG, 16],
              [16, 0, 32]]

DROPOUT_P = [0.0, 0.1, 0.5, 0.999]
DROPOUT_SEEDS = [0, 2 ** 62 - 1, 2 ** 64 - 1]
DROPOUT_N = [1, 255, 3 * THREADS * DROPOUT_CAP + 17]
DROPOUT_CASES = [(p, s, n) for p in DROPOUT_P for s in DROPOUT_SEEDS for n in DROPOUT_N[:2]] + \
                [(p, DROPOUT_SEEDS[i % 3], DROPOUT_N[2]) for i, p in enumerate(DROPOUT_P)]

# rgda_add_bf16: (M, C, row strides of a, b and the output)
ADD_CASES = [(37, 8, (8, 16, 24)), (301, 72, (72, 80, 136)), (9, 520, (528, 520, 1040)),
             (THREADS * ADD_CAP + 1000, 8, (8, 8, 8))]


def paths_reached():
    """{path: [case names]} according to the restatement -- what tests/test_optim_cases_cpu.py lists and checks."""
    out = {}

    def add(p, name):
        out.setdefault(p, []).append(str(name))
    for n in SUMSQ_N:
        if n < 4:
            add('sumsq_only_tail', n)
        elif n & 3:
            add('sumsq_tail_%d' % (n & 3), n)
        if cdiv(n, SUMSQ_PER_BLOCK) > SUMSQ_CAP:
            add('sumsq_cap', n)
    for c in SGD_CASES:
        n4, b = c.n >> 2, sgd_blocks(c.n)
        if b == 1:
            add('sgd_one_block', c.name)
            if n4 == THREADS:
                add('sgd_full_block', c.name)
        if b > 1 and n4 % SGD_VEC_PER_BLOCK and cdiv(n4, SGD_VEC_PER_BLOCK) <= SGD_CAP:
            add('sgd_ragged', c.name)
        if cdiv(n4, SGD_VEC_PER_BLOCK) > SGD_CAP:
            add('sgd_cap', c.name)
        add('sgd_first' if c.first else 'sgd_not_first', c.name)
        total = c.gscale * c.gsig * math.sqrt(c.n)
        if c.gsig == 0:
            add('sgd_zero_grad', c.name)
        elif total > 2 * c.max_norm and c.max_norm > 1e-3:
            add('sgd_clip_active', c.name)
        elif total < c.max_norm / 2:
            add('sgd_clip_inactive', c.name)
        elif abs(c.max_norm / total - c.max_norm / (total + 1e-6)) > 0.01 * c.max_norm / total:
            add('sgd_tiny_norm', c.name)
        add('sgd_gscale_%g' % c.gscale, c.name)
        add('sgd_wd' if c.wd else 'sgd_wd_0', c.name)
        add('sgd_ema_%g' % c.ema, c.name)
        add({'all': 'sgd_all_buffers', 'noshadow': 'sgd_no_shadow', 'nosb': 'sgd_no_sb', 'nopb': 'sgd_no_pb'}[c.bufs], c.name)
    for n in CAST_N:
        if n & 3:
            add('cast_tail', n)
        if cdiv(n, CAST_PER_BLOCK) > CAST_CAP:
            add('cast_cap', n)
    for n in CASTF32_N:
        if cdiv(n, CASTF32_PER_BLOCK) > CASTF32_CAP:
            add('castf32_cap', n)
    for w, s, order in DDP_CASES:
        add('ddp_world_%d' % w, (w, s))
        if cdiv(s >> 3, THREADS) > DDP_CAP:
            add('ddp_cap', (w, s))
        if (s >> 3) % THREADS and s > 8:
            add('ddp_ragged', (w, s))
        if order:
            add('ddp_order', (w, s))
    for tname, rows in LAYOUT_TABLES.items():
        kinds = set()
        for r in rows:
            why = layout_fallback_reasons(r)
            kinds.add(bool(why))
            path = 'fallback' if why else 'vec'
            if not why:
                add('layout_vec', tname)
            for w in why:
                add('layout_fallback_' + w, tname)
            add('layout_mode%d_%s' % (r.mode, path), tname)
            if r.src16:
                add('layout_src16', tname)
                add('layout_src16_' + path, tname)
            else:
                add('layout_src32_' + path, tname)
            for d in (r.Co, r.Ci):
                if d > LAYOUT_TILE and d % LAYOUT_TILE:
                    add('layout_partial_tile', tname)
                if d < LAYOUT_TILE:
                    add('layout_lt_tile', tname)
            add('layout_T%d' % r.T, tname)
            add('layout_off%d' % r.off, tname)
            add('layout_Co%d' % r.Co, tname)
            add('layout_Ci%d' % r.Ci, tname)
        if kinds == {True, False}:
            add('layout_mixed', tname)
        if len(rows) > LAYOUT_LDS_ROWS:
            add('layout_rows_gt_1024', tname)
    for b in FILL_BYTES:
        if 0 < b < 16:
            add('fill_tail_only', b)
        if b >= 16 and b & 15:
            add('fill_tail', b)
        if cdiv(b >> 4, FILL_VEC_PER_BLOCK) > FILL_CAP:
            add('fill_cap', b)
    for sizes in COPY_CASES:
        first = copy_first(sizes)
        if len(sizes) == COPY_MAX_JOBS:
            add('copy_4_jobs', sizes)
        if any(cdiv(b >> 4, COPY_VEC_PER_BLOCK) > COPY_CAP for b in sizes):
            add('copy_cap', sizes)
        # a job of several workgroups followed by another job: the search for the owner of a block crosses first[k + 1]
        if any(first[k + 1] - first[k] > 1 for k in range(len(sizes) - 1)):
            add('copy_job_boundary', sizes)
        if any(b == 0 for b in sizes):
            add('copy_zero_length', sizes)
    for p, s, n in DROPOUT_CASES:
        if loops(n, THREADS, dropout_blocks(n)):
            add('dropout_stride', (p, s, n))
    for M, C, lds in ADD_CASES:
        if cdiv(M * (C // 8), THREADS) > ADD_CAP:
            add('add_cap', (M, C))
        if any(ld != C for ld in lds):
            add('add_strided', (M, C))
        add('add_C%d' % C, (M, C))
    return out


# every path the tables have to reach
REQUIRED = ['sumsq_tail_1', 'sumsq_tail_2', 'sumsq_tail_3', 'sumsq_only_tail', 'sumsq_cap',
            'sgd_one_block', 'sgd_full_block', 'sgd_ragged', 'sgd_cap', 'sgd_first', 'sgd_not_first', 'sgd_clip_active',
            'sgd_clip_inactive', 'sgd_zero_grad', 'sgd_tiny_norm', 'sgd_gscale_1', 'sgd_gscale_0.5', 'sgd_gscale_0.125',
            'sgd_wd', 'sgd_wd_0', 'sgd_ema_0', 'sgd_ema_0.99', 'sgd_ema_0.999', 'sgd_all_buffers', 'sgd_no_shadow',
            'sgd_no_sb', 'sgd_no_pb',
            'cast_tail', 'cast_cap', 'castf32_cap',
            'ddp_world_1', 'ddp_world_2', 'ddp_world_3', 'ddp_world_8', 'ddp_cap', 'ddp_ragged', 'ddp_order',
            'layout_vec', 'layout_fallback_Ci', 'layout_fallback_ld', 'layout_fallback_srcalign',
            'layout_fallback_dstalign', 'layout_fallback_Co_mode0', 'layout_src16', 'layout_src16_vec',
            'layout_src16_fallback', 'layout_src32_vec', 'layout_src32_fallback',
            'layout_mode0_vec', 'layout_mode1_vec', 'layout_mode2_vec', 'layout_mode0_fallback', 'layout_mode1_fallback',
            'layout_mode2_fallback', 'layout_partial_tile', 'layout_lt_tile', 'layout_rows_gt_1024', 'layout_mixed',
            'layout_T1', 'layout_T9', 'layout_off0', 'layout_off1', 'layout_off2', 'layout_off4'] + \
           ['layout_C%s%d' % (x, d) for x in 'oi' for d in (1, 4, 7, 63, 64, 65, 96, 130)] + \
           ['fill_tail_only', 'fill_tail', 'fill_cap', 'copy_4_jobs', 'copy_cap', 'copy_job_boundary', 'copy_zero_length',
            'dropout_stride', 'add_cap', 'add_strided', 'add_C8', 'add_C72', 'add_C520']


# ---------------------------------------------------------------- exact references
BF16_NAN = 0x7FC0


def bf16_bits(x):
    """fp32 tensor -> the bits (int32 in [0, 65536)) of its bf16 rounding, round to nearest, ties to even, from the
    definition: add half an ulp of the result (0x7FFF) plus the lowest kept bit, drop the low 16 bits; the carry moves
    the exponent (and the largest finite values to infinity) by itself.  Every NaN becomes BF16_NAN."""
    b = x.contiguous().view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    r = ((b + 0x7FFF + ((b >> 16) & 1)) >> 16) & 0xFFFF
    return torch.where(torch.isnan(x), torch.full_like(r, BF16_NAN), r).to(torch.int32)


def bf16_canon(t):
    """bf16 tensor -> its bits as int32 with every NaN mapped to BF16_NAN (a NaN stays a NaN; which one is free)."""
    b = t.contiguous().view(torch.int16).to(torch.int32) & 0xFFFF
    return torch.where(((b & 0x7F80) == 0x7F80) & ((b & 0x7F) != 0), torch.full_like(b, BF16_NAN), b)


def bf16_from_bits(bits):
    """Bits (int32 in [0, 65536)) -> bf16 tensor."""
    return (((bits.to(torch.int32) + 0x8000) & 0xFFFF) - 0x8000).to(torch.int16).view(torch.bfloat16)


def f32_canon(t):
    """fp32 tensor -> bits (int32), every NaN mapped to one pattern."""
    b = t.contiguous().view(torch.int32)
    return torch.where(torch.isnan(t), torch.full_like(b, 0x7FC00000), b)


CAST_SPECIALS_BITS = [
    0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x7FC00000, 0xFFC00001, 0x7F800001,     # +-0, +-inf, NaNs
    0x3F808000, 0x3F818000, 0xBF808000, 0xBF818000,     # exact ties: down to an even 0x3F80, up to an even 0x3F82
    0x3F808001, 0x3F807FFF, 0x3F818001, 0x3F817FFF,     # one bit either side of a tie
    0x7F7FFFFF, 0xFF7FFFFF, 0x7F7F7FFF, 0x7F7F8000,     # largest finite fp32 (-> inf), and around the last bf16
    0x00800000, 0x3F800000,
]


def cast_specials(device='cpu'):
    return torch.tensor(np.array(CAST_SPECIALS_BITS, dtype=np.uint32).view(np.float32), device=device)


def ddp_reference_bits(recv, world, descending=False):
    """recv [world][s] bf16 -> bf16 bits of the fp32 sum taken one rank after the other, starting from zero, rounded
    once (every partial sum is one IEEE fp32 add, as torch performs it)."""
    acc = torch.zeros(recv.shape[1], dtype=torch.float32, device=recv.device)
    for r in (range(world - 1, -1, -1) if descending else range(world)):
        acc = acc + recv[r].float()
    return bf16_bits(acc)


def ddp_input(world, s, order, device):
    """recv [world][s] bf16: random values, with the order-dependent triple planted in ranks (0, 1, world - 1) of every
    seventh element (the ranks between hold zero there)."""
    gen = torch.Generator().manual_seed(world * 1000003 + s)
    recv = torch.randn(world, s, generator=gen).to(torch.bfloat16)
    if order:
        recv[:, ::7] = 0
        for r, val in zip((0, 1, world - 1), ORDER_TRIPLE):
            recv[r, ::7] = val
    return recv.to(device)


def layout_reference_bits(src, r):
    """src: the [Co][T][ld] source tensor of row r (fp32 or bf16) -> bf16 bits of the destination, in its own shape."""
    sl = src[:, :, r.off:r.off + r.Ci].float()
    ref = {0: sl.permute(2, 1, 0), 1: sl.permute(1, 0, 2), 2: sl}[r.mode].contiguous()
    return bf16_bits(ref)


_GOLDEN, _M1, _M2 = 0x9E3779B97F4A7C15, 0xBF58476D1CE4E5B9, 0x94D049BB133111EB


def splitmix64(seed, n):
    """Outputs 0 .. n-1 of SplitMix64 (Steele, Lea, Flood 2014) seeded with `seed`: the state advances by the golden
    gamma BEFORE each output, z = state; z = (z ^ z >> 30) M1; z = (z ^ z >> 27) M2; z ^ z >> 31; all modulo 2^64."""
    with np.errstate(over='ignore'):
        state = np.uint64(seed) + np.uint64(_GOLDEN) * np.arange(1, n + 1, dtype=np.uint64)
        z = (state ^ (state >> np.uint64(30))) * np.uint64(_M1)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(_M2)
        return z ^ (z >> np.uint64(31))


def dropout_reference(n, p, seed):
    """-> fp32 numpy mask: u_i = (top 24 bits of output i) 2^-24, keep = fp32(1) / (fp32(1) - fp32(p)) where u_i >= p."""
    u = (splitmix64(seed, n) >> np.uint64(40)).astype(np.float32) * np.float32(2.0 ** -24)
    p32 = np.float32(p)
    keep = np.float32(1) / (np.float32(1) - p32)
    return np.where(u >= p32, keep, np.float32(0)).astype(np.float32)


# ---------------------------------------------------------------- the SGD step
# regda_amd/csrc/Makefile compiles with `-O3 -std=c++17 -munsafe-fp-atomics`: no -ffast-math, no
# -fno-hip-fp32-correctly-rounded-divide-sqrt, no denormal flushing.  hipcc's default is then IEEE fp32 with a correctly
# rounded sqrtf and division (0 ulp each), and -ffp-contract=fast, which lets the compiler fuse
# `sqrtf(gn) * gscale + 1e-6f` into one fma.  coef_fp32 forms coef unfused; against the fused form its denominator
# carries one more rounding (2^-24 relative), which the correctly rounded quotient passes on and may re-round by one ulp
# (2^-23 relative at worst); min() and the final product by gscale (a power of two in every case) are exact.
# Allowance: 2^-24 + 2^-23 = 3 * 2^-24 relative.  Where the clamp is taken coef is gscale exactly (the clamp is only
# accepted as taken when the unclamped quotient clears 1 by more than that allowance).
COEF_REL = 3 * U32


def coef_fp32(gnorm_sq, gscale, max_norm):
    """(coef, relative allowance) from the fp32 word the kernel read: torch's clip_grad_norm_ on the averaged gradient,
    coef = min(max_norm / (total + 1e-6), 1) * gscale with total = sqrt(gnorm_sq) * gscale, every step in fp32."""
    f = np.float32
    with np.errstate(divide='ignore'):
        total = np.sqrt(f(gnorm_sq)) * f(gscale)
        q = f(max_norm) / (total + f(1e-6))
    if q > 1 + 4 * COEF_REL:
        return float(f(gscale)), 0.0
    return float(f(min(q, f(1)) * f(gscale))), COEF_REL


def sgd_reference(p, g, v, shadow, coef, coef_rel, lr, momentum, wd, ema, first):
    """One step in fp64 on the fp32 values the kernel read (tensors of any device; v is ignored when `first`).
        d = g coef + wd p                 torch SGD: weight decay added to the (clipped, averaged) gradient
        v' = d | momentum v + d           buf = d_p on the first step
        p' = p - lr v'
        s' = (1 - ema) p' + ema s         regda/utils/ema.py
    lr, momentum, wd, ema are the fp32 values the kernel received.  -> (v', p', s', Ev, Ep, Es), the E per-element bounds.

    Bounds: every fp32 operation, fused or not, rounds once and errs by at most 2^-24 of its result, which is at most the
    sum of the magnitudes of the terms it combines; k roundings on the way to a value give gamma(k) = k u / (1 - k u)
    times that sum (contraction only removes roundings).
        d:  g*coef, wd*p, their sum                      3 roundings of |g coef| + |wd p|, plus |g coef| coef_rel
        v': momentum*v, its sum with d                   2 more, of |momentum v| + |g coef| + |wd p|   (not first)
        p': lr*v', the subtraction                       2 roundings of |p| + lr |v'|, plus lr Ev
        s': 1 - ema (exact for ema = 0 and ema >= 0.5 -- Sterbenz -- counted anyway), a*p', ema*s, their sum
                                                         4 roundings of |(1 - ema) p'| + |ema s|, plus (1 - ema) Ep
    """
    f64 = torch.float64
    p, g = p.to(f64), g.to(f64)
    gc, wp = g * coef, wd * p
    d = gc + wp
    Ad = gc.abs() + wp.abs()
    Ed = gamma(3) * Ad + gc.abs() * coef_rel
    if first:
        vn, Ev = d, Ed
    else:
        mv = momentum * v.to(f64)
        vn = mv + d
        Ev = gamma(5) * (mv.abs() + Ad) + gc.abs() * coef_rel
    pn = p - lr * vn
    Ep = gamma(2) * (p.abs() + lr * (vn.abs() + Ev)) + lr * Ev
    if shadow is None:
        return vn, pn, None, Ev, Ep, None
    a = 1.0 - ema
    s = shadow.to(f64)
    sn = a * pn + ema * s
    Es = gamma(4) * (a * (pn.abs() + Ep) + (ema * s).abs()) + a * Ep
    return vn, pn, sn, Ev, Ep, Es


def sumsq_bound(n):
    """Relative bound of rgda_sumsq (every term positive, so it is a bound on the sum): x^2 + y^2 of a pair in fp32 (2
    roundings, one when fused), the partial and the total each rounded to fp32 once (2 more): gamma(4); the fp64
    accumulation in between adds at most n 2^-53."""
    return gamma(4) + n * 2.0 ** -53
