"""The teacher / evaluation kernels of regda_amd/csrc/teacher_kernels.hip (dihedral views, window crop / accumulate /
normalise, the align-corners resize, row padding, argmax, the confusion matrix): a Python restatement of the host-side
decisions, a table of small cases that each name the path they are there to reach, and plain numpy / torch-CPU references.

The restatement mirrors teacher_kernels.hip; tests/test_teacher_cases_cpu.py parses the constants it copies out of the
source, so a change there that is not made here fails on a machine without a GPU.

References: permutations, crops, pads, argmax and counts are exact (np.rot90 / np.flip, slicing, torch's pad on the CPU,
np.add.at); window_normalise is numpy's fp32 division, bit for bit; the dihedral scale-and-accumulate and the resize are
fp64 from the fp32 inputs, the bilinear source index from the fp32 product scale * dst as tests/label_cases.py argues.

Inputs are built on the CPU from fixed seeds; nothing here needs a GPU or the library.
"""
import zlib
from collections import namedtuple

import numpy as np
import torch
import torch.nn.functional as F

from label_cases import bilinear64

# ---------------------------------------------------------------- the restatement (teacher_kernels.hip)
THREADS = 256
GRID_CAP = 65535                     # grid_for() and rgda_dihedral_nchw
CONFUSION_GRID_CAP = 1024            # rgda_confusion_accumulate: each workgroup counts < 2^32 elements in 32-bit cells
CONFUSION_MAX_CLASSES = 64           # 64 * 64 * 4 B = the 16 KB histogram
OK, ERR_ARG = 0, -1


def cdiv(a, b):
    return -(-a // b)


def grid_for(total, cap=GRID_CAP):
    return min(max(cdiv(total, THREADS), 1), cap)


def trips(total, cap=GRID_CAP):
    """Trips of the grid-stride loop of the busiest thread."""
    return cdiv(total, grid_for(total, cap) * THREADS)


def dihedral_shape(n, c, h, w, k):
    return (n, c, w, h) if k & 1 else (n, c, h, w)


def confusion_status(n, C):
    return ERR_ARG if n < 0 or C <= 0 or C > CONFUSION_MAX_CLASSES else OK


def _rng(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


# ---------------------------------------------------------------- dihedral
VIEWS = [(f, k, ff) for ff in (1, 0) for f in (0, 1) for k in range(4)]          # all 16 (hflip, k, flip_first)
DIHEDRAL_SHAPES = [(1, 1, 1, 1), (1, 1, 1, 7), (1, 2, 7, 1), (2, 3, 5, 9)]
DIHEDRAL_BIG = (1, 1, 4099, 4093)    # > 65535 * 256 elements, H != W: the second trip of an odd rotation
DIHEDRAL_BIG_VIEWS = [(1, 1, 1), (0, 3, 0)]
DIHEDRAL_SCALE = 0.3                 # scale + accumulate, on the last small shape


def dihedral_ref(src, hflip, k, flip_first):
    """flip_first = 1: R^k(F^f(src)) (augment); 0: F^f(R^k(src)) (de-augment).  R = rot90 over (H, W), F = flip of W."""
    src = np.asarray(src)
    if flip_first:
        x = np.flip(src, 3) if hflip else src
        return np.ascontiguousarray(np.rot90(x, k, (2, 3)))
    x = np.rot90(src, k, (2, 3))
    return np.ascontiguousarray(np.flip(x, 3) if hflip else x)


def index_image(shape):
    """Every element its own flat index: exact in fp32 below 2^24, so a permutation is checked element by element."""
    n = int(np.prod(shape))
    assert n <= 1 << 24
    return np.arange(n, dtype=np.float32).reshape(shape)


def dihedral_acc_inputs(shape, view):
    r = _rng('dihedral_acc', shape, view)
    src = r.standard_normal(shape).astype(np.float32)
    old = r.standard_normal(dihedral_shape(*shape, view[1])).astype(np.float32)
    return src, old


def dihedral_acc_ref(src, old, view, scale):
    """-> (fp64 result, per-element bound): two fp32 roundings, of scale * src and of the sum (one, of the sum alone, where
    the compiler fuses them): 2^-24 (|scale * src| + |result|)."""
    v = float(np.float32(scale)) * dihedral_ref(src, *view).astype(np.float64)
    out = old.astype(np.float64) + v
    return out, 2.0 ** -24 * (np.abs(v) + np.abs(out))


# ---------------------------------------------------------------- windows
# name, (N, C, Hf, Wf), y1, x1, h, w, Th, Tw, paths
CropCase = namedtuple('CropCase', 'name shape y1 x1 h w Th Tw paths')
CROP_CASES = [
    CropCase('pad_both', (1, 1, 9, 11), 2, 3, 4, 5, 6, 8, ('pad_rows', 'pad_cols')),
    CropCase('far_corner', (1, 1, 9, 11), 4, 5, 5, 6, 5, 6, ('far_corner',)),
    CropCase('one_pixel', (1, 1, 3, 3), 2, 2, 1, 1, 2, 3, ('one_pixel', 'far_corner')),
    CropCase('planes', (2, 3, 7, 6), 1, 0, 5, 4, 6, 4, ('planes', 'pad_rows')),
]


def crop_ref(full, c):
    t = np.zeros(full.shape[:2] + (c.Th, c.Tw), np.float32)
    t[:, :, :c.h, :c.w] = full[:, :, c.y1:c.y1 + c.h, c.x1:c.x1 + c.w]
    return t


# name, (N, C, Hf, Wf), (Th, Tw), windows [(y1, x1, h, w)], paths
AccCase = namedtuple('AccCase', 'name shape tile windows paths')
ACC_CASES = [
    AccCase('tile_larger_nan_padding', (1, 2, 7, 9), (5, 6), [(1, 2, 3, 4)], ('nan_padding', 'prefilled')),
    AccCase('two_overlapping', (2, 3, 8, 8), (4, 4), [(1, 1, 4, 4), (3, 2, 4, 4)], ('overlap', 'planes', 'prefilled')),
    AccCase('far_corner_one_pixel', (1, 1, 3, 4), (2, 2), [(2, 3, 1, 1)], ('one_pixel', 'nan_padding', 'prefilled')),
]


def acc_inputs(c):
    """-> (tiles [one per window; NaN in the padding the kernel must not read], full, count), all pre-filled."""
    r = _rng('acc', c.name)
    N, C, Hf, Wf = c.shape
    full = r.standard_normal(c.shape).astype(np.float32)
    count = r.integers(0, 4, (N, 1, Hf, Wf)).astype(np.float32)
    tiles = []
    for (_, _, h, w) in c.windows:
        t = np.full((N, C) + c.tile, np.nan, np.float32)
        t[:, :, :h, :w] = r.standard_normal((N, C, h, w)).astype(np.float32)
        tiles.append(t)
    return tiles, full, count


def acc_ref(tiles, full, count, c):
    full, count = full.copy(), count.copy()
    for t, (y1, x1, h, w) in zip(tiles, c.windows):
        full[:, :, y1:y1 + h, x1:x1 + w] += t[:, :, :h, :w]      # fp32 + fp32: one rounding, one right answer
        count[:, :, y1:y1 + h, x1:x1 + w] += np.float32(1)
    return full, count


NORM_SHAPES = [(1, 1, 1, 1), (2, 3, 5, 7)]
NORM_BIG = (2, 3, 1673, 1672)        # N * C * HW > 65535 * 256: the n / p split on the second trip


def norm_inputs(shape):
    """Counts 0 .. 8 (zero included: x / 0 = +-inf, 0 / 0 = NaN); a plane of `full` holds zeros where the count is 0."""
    r = _rng('norm', shape)
    N, C, H, W = shape
    full = r.standard_normal(shape).astype(np.float32)
    count = r.integers(0, 9, (N, 1, H, W)).astype(np.float32)
    full[:, 0][count[:, 0] == 0] = 0.0
    return full, count


def norm_ref(full, count):
    with np.errstate(all='ignore'):
        return (full / count).astype(np.float32)                 # IEEE fp32 division, as __fdiv_rn


# ---------------------------------------------------------------- resize, pad
RESIZE_CASES = [((2, 3, 7, 9), (7, 9)), ((2, 3, 7, 9), (1, 1)), ((2, 3, 7, 9), (13, 4)), ((2, 3, 7, 9), (20, 31)),
                ((2, 3, 1, 5), (4, 9)), ((2, 3, 5, 1), (3, 3)), ((2, 3, 6, 6), (1, 7)), ((1, 2, 33, 33), (513, 513)),
                ((1, 5, 64, 48), (40, 24))]


def resize_name(shape, size):
    return '%dx%d_to_%dx%d' % (shape[2], shape[3], size[0], size[1])


def resize_inputs(shape, size):
    return torch.from_numpy(_rng('resize', shape, size).standard_normal(shape).astype(np.float32))


def resize_ref(x, size):
    return bilinear64(x, size[0], size[1])


def resize_oracle32(x, size):
    return F.interpolate(x, size, mode='bilinear', align_corners=True)


PAD_SHAPE = (2, 3, 5, 4)
PAD_CASES = [(2, 3), (0, 0), (-1, -2), (-3, 5), (4, -2)]


def pad_ref(x, top, bottom):
    return F.pad(torch.as_tensor(x), (0, 0, top, bottom), 'constant', 0).numpy()


# ---------------------------------------------------------------- argmax, confusion matrix
def argmax_cases():
    """-> [(name, probs f32 (N, C, H, W))]: first maximum wins."""
    r = _rng('argmax')
    out = [('c1', r.standard_normal((2, 1, 3, 5)).astype(np.float32)),
           ('hw1', r.standard_normal((3, 6, 1, 1)).astype(np.float32)),
           ('hw257', r.standard_normal((2, 7, 1, 257)).astype(np.float32))]
    x = r.standard_normal((1, 6, 1, 257)).astype(np.float32) - 3.0                # negatives and -inf
    x[0, :, 0, ::5] = -np.inf
    x[0, 2, 0, ::5] = -7.0
    x[0, :, 0, 3] = -np.inf                                                      # every class -inf: class 0
    out.append(('neg_inf', x))
    t = r.standard_normal((1, 5, 3, 11)).astype(np.float32)
    t[0, 1, 0] = t[0, 0, 0] = 4.0                                                # tie of the first pair -> 0
    t[0, 4, 1] = t[0, 3, 1] = 4.0                                                # tie of the last pair -> 3
    t[0, :, 2] = 0.25                                                            # all classes tie -> 0
    out.append(('ties', t))
    return out


def argmax_ref(x):
    x = np.asarray(x)
    best, arg = x[:, 0].copy(), np.zeros(x[:, 0].shape, np.int64)
    for c in range(1, x.shape[1]):
        m = x[:, c] > best
        best, arg = np.where(m, x[:, c], best), np.where(m, c, arg)
    return arg


# name, n, C, special, paths
ConfCase = namedtuple('ConfCase', 'name n C special paths')
CONF_CASES = [
    ConfCase('c1', 300, 1, None, ('c1',)),
    ConfCase('c64', 5000, 64, None, ('c64',)),
    ConfCase('n0', 0, 6, None, ('n0',)),
    ConfCase('n1', 1, 6, None, ('n1',)),
    ConfCase('second_trip', CONFUSION_GRID_CAP * THREADS + 77, 7, None, ('second_trip',)),
    ConfCase('negative_truth_skipped', 600, 6, 'negative', ('skipped',)),
    ConfCase('out_of_range_flagged', 600, 6, 'bad', ('flagged',)),
]
CONF_CM0, CONF_FLAG0 = 5, 0          # cm is pre-filled with 5 everywhere: the kernel accumulates


def conf_inputs(c):
    r = _rng('conf', c.name)
    yt = r.integers(0, c.C, c.n).astype(np.int64)
    yp = r.integers(0, c.C, c.n).astype(np.int64)
    if c.special == 'negative':
        yt[::7], yt[3::11] = -1, -5
        yp[::14] = c.C                                           # under a skipped truth: not looked at, no flag
    elif c.special == 'bad':
        yt[::7], yt[5] = -1, c.C
        yp[1], yp[2] = -1, c.C
        yt[1], yt[2] = 0, 1
    return yt, yp


def conf_ref(yt, yp, C, cm0=CONF_CM0):
    """-> (cm int64 (C, C), flag): truth < 0 skipped; truth >= C or a prediction outside [0, C): flag 1, not counted."""
    cm = np.full((C, C), cm0, np.int64)
    live = yt >= 0
    bad = live & ((yt >= C) | (yp < 0) | (yp >= C))
    ok = live & ~bad
    np.add.at(cm, (yt[ok], yp[ok]), 1)
    return cm, int(bad.any())


# ---------------------------------------------------------------- which case reaches which path
REQUIRED = ['dihedral:second_trip', 'dihedral:one_pixel', 'dihedral:one_row', 'dihedral:one_col', 'dihedral:planes',
            'crop:pad_rows', 'crop:pad_cols', 'crop:far_corner', 'crop:one_pixel', 'crop:planes',
            'acc:nan_padding', 'acc:prefilled', 'acc:overlap', 'acc:planes', 'acc:one_pixel', 'norm:zero_count', 'norm:second_trip',
            'resize:identity', 'resize:one_out', 'resize:one_row_src', 'resize:one_col_src', 'resize:one_row_dst',
            'resize:up', 'resize:down', 'pad:both', 'pad:none', 'pad:crop_both', 'pad:crop_top', 'pad:crop_bottom',
            'argmax:c1', 'argmax:hw1', 'argmax:two_blocks', 'argmax:neg_inf', 'argmax:ties',
            'conf:c1', 'conf:c64', 'conf:n0', 'conf:n1', 'conf:second_trip', 'conf:skipped', 'conf:flagged']


def paths_reached():
    r = {}

    def hit(path, name):
        r.setdefault(path, []).append(name)

    for s in DIHEDRAL_SHAPES + [DIHEDRAL_BIG]:
        n, c, h, w = s
        if trips(n * c * h * w) >= 2 and h != w and all(k & 1 for _, k, _ in DIHEDRAL_BIG_VIEWS):
            hit('dihedral:second_trip', s)
        if h == w == 1:
            hit('dihedral:one_pixel', s)
        elif h == 1:
            hit('dihedral:one_row', s)
        elif w == 1:
            hit('dihedral:one_col', s)
        if n > 1 and c > 1:
            hit('dihedral:planes', s)
    for c in CROP_CASES:
        N, C, Hf, Wf = c.shape
        if c.h < c.Th:
            hit('crop:pad_rows', c.name)
        if c.w < c.Tw:
            hit('crop:pad_cols', c.name)
        if c.y1 + c.h == Hf and c.x1 + c.w == Wf:
            hit('crop:far_corner', c.name)
        if c.h == c.w == 1:
            hit('crop:one_pixel', c.name)
        if N > 1 and C > 1:
            hit('crop:planes', c.name)
    for c in ACC_CASES:
        if any(h < c.tile[0] or w < c.tile[1] for _, _, h, w in c.windows):
            hit('acc:nan_padding', c.name)
        hit('acc:prefilled', c.name)
        if len(c.windows) > 1:
            (a, b, h, w), (a2, b2, h2, w2) = c.windows[:2]
            if a < a2 + h2 and a2 < a + h and b < b2 + w2 and b2 < b + w:
                hit('acc:overlap', c.name)
        if c.shape[0] > 1 and c.shape[1] > 1:
            hit('acc:planes', c.name)
        if any(h == w == 1 for _, _, h, w in c.windows):
            hit('acc:one_pixel', c.name)
    for s in NORM_SHAPES + [NORM_BIG]:
        if s != NORM_BIG and (norm_inputs(s)[1] == 0).any():
            hit('norm:zero_count', s)
        if trips(int(np.prod(s))) >= 2 and s[0] > 1 and s[1] > 1:
            hit('norm:second_trip', s)
    for shape, size in RESIZE_CASES:
        name = resize_name(shape, size)
        h, w = shape[2:]
        if (h, w) == size:
            hit('resize:identity', name)
        if size == (1, 1):
            hit('resize:one_out', name)
        if h == 1:
            hit('resize:one_row_src', name)
        if w == 1:
            hit('resize:one_col_src', name)
        if size[0] == 1 and size[1] > 1:
            hit('resize:one_row_dst', name)
        if size[0] > h and size[1] > w:
            hit('resize:up', name)
        if size[0] < h and size[1] < w and size != (1, 1):
            hit('resize:down', name)
    for top, bottom in PAD_CASES:
        key = ('both' if top > 0 and bottom > 0 else 'none' if top == bottom == 0 else
               'crop_both' if top < 0 and bottom < 0 else 'crop_top' if top < 0 else 'crop_bottom')
        hit('pad:' + key, (top, bottom))
    for name, x in argmax_cases():
        N, C, H, W = x.shape
        if C == 1:
            hit('argmax:c1', name)
        if H * W == 1:
            hit('argmax:hw1', name)
        if N * H * W > THREADS:
            hit('argmax:two_blocks', name)
        if np.isinf(x).any() and (x < 0).any() and (argmax_ref(x) == 0).any():
            hit('argmax:neg_inf', name)
        if name == 'ties' and (x[0, 0, 0] == x[0, 1, 0]).all() and (x[0, 3, 1] == x[0, 4, 1]).all():
            hit('argmax:ties', name)
    for c in CONF_CASES:
        yt, yp = conf_inputs(c)
        if c.C == 1:
            hit('conf:c1', c.name)
        if c.C == CONFUSION_MAX_CLASSES:
            hit('conf:c64', c.name)
        if c.n in (0, 1):
            hit('conf:n%d' % c.n, c.name)
        if trips(c.n, CONFUSION_GRID_CAP) >= 2:
            hit('conf:second_trip', c.name)
        if (yt == -1).any() and (yt == -5).any() and conf_ref(yt, yp, c.C)[1] == 0:
            hit('conf:skipped', c.name)
        if (yt == c.C).any() and (yp == -1).any() and (yp == c.C).any() and conf_ref(yt, yp, c.C)[1] == 1:
            hit('conf:flagged', c.name)
    return r
