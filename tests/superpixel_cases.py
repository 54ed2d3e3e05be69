"""The region-map kernels of regda_amd/csrc/superpixel_kernels.hip (the integer SLIC, the components, the root numbering,
region_shrink): a Python restatement of the host-side geometry that cuts a call into workgroups, a table of small cases
that each name the path they are there to reach, and the memoised output of the numpy restatement of the specification
(tests/superpixel_ref.py) for each of them.

Everything is integer and specified bit for bit, so every comparison made with this table is an exact array_equal.
tests/test_superpixel_cases_cpu.py proves, from the restatement alone, that each case holds what its claims say (and
parses the constants copied out of the source); tests/test_superpixel_passes_gpu.py runs the kernels on the cases.

Inputs are built on the CPU from fixed seeds; nothing here needs a GPU or the library.
"""
import functools
from collections import namedtuple

import numpy as np

import superpixel_ref as R

# ---------------------------------------------------------------- the restatement (superpixel_kernels.hip)
SPX_TILE = 32            # a SLIC workgroup covers bc x bc cells, bc = S >= 32 ? 1 : 32 / S
SPX_MAX_T = 64           # the largest tile edge, max(32, S)
SPX_MAX_CAND = 100       # (32 / 4 + 2)^2 candidate centres in LDS
CCL_T = 32               # component tile edge
SCAN_CHUNK = 1024        # pixels per workgroup of the root numbering passes
SCAN_THREADS = 256       # chunk counts root_scan_kernel takes per pass of its loop
SHR_T, SHR_MAX_WIN = 32, 8
INT32_MAX, INT32_MIN = 2 ** 31 - 1, -2 ** 31


def cdiv(a, b):
    return -(-a // b)


def cell_block(S):
    """-> (bc, tile edge in pixels, candidate slots cw * cw)."""
    bc = 1 if S >= SPX_TILE else SPX_TILE // S
    return bc, bc * S, (bc + 2) ** 2


def heads(N, H, W, S):
    """The byte offset inside its dword at which every staged tile row starts (slic_iter_kernel's `head`), as a set."""
    bc = cell_block(S)[0]
    x0 = np.arange(0, W // S, bc) * S
    rows = np.arange(N * H)
    return set((((rows[:, None] * W + x0[None, :]) * 3) & 3).reshape(-1).tolist())


def chunk_count(H, W):
    return cdiv(H * W, SCAN_CHUNK)


# ---------------------------------------------------------------- generators added to those of superpixel_ref
def constant_image(H, W, value=77):
    return np.full((H, W, 3), value, np.uint8)


def black_white(H, W, seed, white=0.5):
    """Every pixel pure black or pure white at random; `white` is the probability of white in the left half of the
    image and of black in the right half.  A small value gives centres that are black (white) to the last bit with a
    few pixels of the opposite extreme among them: the colour term of d at its maximum 3 * 255^2 * S^2."""
    rng = np.random.default_rng(seed)
    u = rng.random((H, W))
    on = np.where(np.arange(W)[None, :] < W // 2, u < white, u >= white)
    return np.repeat(np.where(on, 255, 0).astype(np.uint8)[..., None], 3, -1)


_GEN = dict(noise=R.blurred_noise, scene=R.rectangle_scene, diagonal=R.diagonal_image, constant=constant_image,
            bw=black_white)

# ---------------------------------------------------------------- the cases
# gens: one (generator, args...) per image of the batch.  claims: what the case is there for, each proved on the CPU
# (tests/test_superpixel_cases_cpu.py: CLAIMS).
Case = namedtuple('Case', 'name gens S m iters min_area claims')


def _n(H, W, seed=3):
    return ('noise', H, W, seed)


CASES = [
    # cell-block geometry and unaligned staging
    Case('s4', (_n(40, 36),), 4, 10, 5, 4, ('bc_8', 'cand_full', 'part_block', 'drop_keep')),
    Case('s5', (_n(35, 45),), 5, 10, 5, 6, ('tile_30', 'head', 'tail', 'part_block', 'drop_keep')),
    Case('s12', (_n(36, 60),), 12, 10, 5, 6, ('bc_2', 'tile_24', 'part_block', 'drop_keep')),
    Case('s20', (_n(60, 100),), 20, 10, 5, 6, ('bc_1', 'tile_20', 'drop_keep')),
    Case('s33_m1', (_n(66, 99),), 33, 1, 4, 6, ('bc_1', 'tile_33', 'head', 'tail', 'm_1', 'drop_keep')),
    Case('s48', (_n(96, 144),), 48, 10, 5, 6, ('bc_1', 'tile_48', 'drop_keep')),
    Case('s64_m64', (_n(192, 128),), 64, 64, 4, 200, ('bc_1', 'tile_64', 'm_64')),
    Case('bw_s64', (('bw', 128, 192, 3, 1.0 / 1024),), 64, 64, 3, 1, ('tile_64', 'm_64', 'd_large', 'min_area_1')),
    # the dimension limit: 1024 chunks (4 passes of root_scan's loop), a grid one cell wide
    Case('tall', (('scene', 16384, 64, 11),), 64, 64, 2, 64, ('dim_max', 'chunks_gt_256', 'one_cell_wide', 'span_4', 'drop_keep')),
    Case('wide', (('scene', 64, 16384, 12),), 64, 64, 2, 64, ('dim_max', 'chunks_gt_256', 'one_cell_wide', 'span_4', 'drop_keep')),
    # the tie rule at even S (rows and columns equally far from two centres) and at odd S (no nearest tie: the grid stays)
    Case('const_s4_i1', (('constant', 32, 32),), 4, 10, 1, 4, ('ties_min', 'ties_any', 'cand_full')),
    Case('const_s4_i4', (('constant', 32, 32),), 4, 10, 4, 4, ('ties_min', 'ties_any', 'cand_full')),
    Case('const_s5_i1', (('constant', 35, 35),), 5, 10, 1, 6, ('ties_any', 'grid_kept', 'head', 'tail')),
    Case('const_s5_i4', (('constant', 35, 35),), 5, 10, 4, 6, ('ties_any', 'grid_kept', 'head', 'tail')),
] + [
    # the iteration sweep: every residue of the three sum buffers (it % 3) and the two centre buffers (it & 1)
    Case('iters%d' % it, (_n(64, 96, 1),), 8, 10, it, 16, ('rotation_%d' % (it % 6), 'drop_keep'))
    for it in range(1, 8)
] + [
    # batches: images 1 and 2 start off a dword boundary, HW is no multiple of 256 or 1024
    Case('batch3_s5', (_n(35, 45, 3), _n(35, 45, 4), ('scene', 35, 45, 5, 6)), 5, 10, 5, 6,
         ('batch', 'image_off_dword', 'hw_ragged', 'head', 'tail', 'drop_keep')),
    Case('batch2_s33', (_n(66, 99, 3), _n(66, 99, 8)), 33, 10, 4, 6,
         ('batch', 'image_off_dword', 'hw_ragged', 'head', 'drop_keep')),
    # min_area extremes on a fragmenting image
    Case('min_area_1', (_n(64, 96, 1),), 8, 10, 5, 1, ('min_area_1',)),
    Case('min_area_all', (_n(64, 96, 1),), 8, 10, 5, 64 * 96 + 1, ('min_area_all',)),
]
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
BATCH_CASES = [c.name for c in CASES if len(c.gens) > 1]
# small enough for the stack flood fill of tests/test_superpixels_cpu.py
FLOOD_MAX_PIXELS = 20000

# what the issue's own run of the restatement gave (blurred_noise, seed 3): (regions, dropped pixels)
RECORDED = dict(s4=(123, 398), s5=(85, 635), s64_m64=(6, None))


@functools.lru_cache(maxsize=None)
def images(name):
    """The case's images, read-only."""
    out = []
    for g in BY_NAME[name].gens:
        img = np.ascontiguousarray(_GEN[g[0]](*g[1:]))
        img.flags.writeable = False
        out.append(img)
    return tuple(out)


Oracle = namedtuple('Oracle', 'regs count centres labels roots')


@functools.lru_cache(maxsize=None)
def _oracle_image(gen, S, m, iters):
    img = np.ascontiguousarray(_GEN[gen[0]](*gen[1:]))
    labels, centres = R.slic_labels(img, S, m, iters)
    roots = R.components(labels)
    for a in (labels, centres, roots):
        a.flags.writeable = False
    return labels, centres, roots


@functools.lru_cache(maxsize=None)
def oracle(name):
    """Per image of the case: (regs, count, centres of the last Assign, labels, roots) of the restatement, computed once
    (cases that differ in min_area only share the SLIC and the components) and read-only."""
    c = BY_NAME[name]
    out = []
    for g in c.gens:
        labels, centres, roots = _oracle_image(g, c.S, c.m, c.iters)
        regs, count = R.number(roots, c.min_area)
        regs.flags.writeable = False
        out.append(Oracle(regs, count, centres, labels, roots))
    return tuple(out)


def candidate_d(img, centres, S, m):
    """d of every pixel to its nine candidate slots in ascending k, int64 [9][H][W]; -1 where the cell does not exist.
    Written apart from superpixel_ref.assign (which it is checked against) to look at ties and at the size of d."""
    H, W, _ = img.shape
    Gy, Gx = H // S, W // S
    yy, xx = np.mgrid[0:H, 0:W]
    px = img.astype(np.int64)
    out = np.full((9, H, W), -1, np.int64)
    for i, (a, b) in enumerate((a, b) for a in (-1, 0, 1) for b in (-1, 0, 1)):
        cy, cx = yy // S + a, xx // S + b
        ok = (cy >= 0) & (cy < Gy) & (cx >= 0) & (cx < Gx)
        c = centres[np.where(ok, cy * Gx + cx, 0)]
        d = ((px - c[..., 2:5]) ** 2).sum(-1) * (S * S) + (m * m) * ((yy - c[..., 0]) ** 2 + (xx - c[..., 1]) ** 2)
        out[i] = np.where(ok, d, -1)
    return out


def assign_trace(img, S, m, iters):
    """-> [(centres, d [9][H][W]) of Assign 1 .. iters]: slic_labels' loop with every iteration's candidates kept."""
    H, W, _ = img.shape
    centres = R.update(img, R.grid_labels(H, W, S), S)
    out = []
    for it in range(1, iters + 1):
        out.append((centres, candidate_d(img, centres, S, m)))
        if it < iters:
            centres = R.update(img, R.assign(img, centres, S, m), S, centres)
    return out


def tiles_crossed(roots, regs):
    """The largest number of 32 x 32 component tiles one kept component lies in."""
    H, W = roots.shape
    yy, xx = np.mgrid[0:H, 0:W]
    tile = (yy // CCL_T) * cdiv(W, CCL_T) + xx // CCL_T
    kept, T = regs > 0, int(tile.max()) + 1
    pairs = np.unique(roots[kept].astype(np.int64) * T + tile[kept])        # one entry per (component, tile)
    return int(np.unique(pairs // T, return_counts=True)[1].max()) if pairs.size else 0


# ---------------------------------------------------------------- region_shrink
SHRINK_WINS = (0, 1, 2, 3, 5, 8)
SHRINK_SHAPES = ((1, 1, 1), (1, 1, 70), (1, 70, 1), (1, 33, 31), (1, 5, 7), (1, 64, 64), (3, 70, 45))
SHRINK_IDS = (-3, -1, 0, 5, 9, INT32_MAX)


@functools.lru_cache(maxsize=None)
def shrink_map(shape):
    """int32 [N][H][W]: blocks of 12 x 9 pixels (2 x 3 along an edge shorter than 24) of ids that include negatives and
    INT32_MAX, and (from 33 rows on) one block of half the image that reaches the bottom edge, so that the largest
    window keeps something too."""
    N, H, W = shape
    rng = np.random.default_rng(N * 100003 + H * 257 + W)
    pal = np.array(SHRINK_IDS, np.int64)
    out = np.empty(shape, np.int32)
    for n in range(N):
        bh, bw = (12 if H >= 24 else 2), (9 if W >= 24 else 3)
        ids = pal[rng.integers(0, len(pal), (cdiv(H, bh), cdiv(W, bw)))]
        out[n] = ids[np.arange(H)[:, None] // bh, np.arange(W)[None, :] // bw]
        if H >= 33 and n != 1:
            out[n, H // 2:, W // 8:W // 8 + max(W // 2, 20)] = INT32_MAX if n == 0 else -3
    out.flags.writeable = False
    return out


def shrink_fills(regs):
    """0, -7, an id present in the map, INT32_MIN."""
    return (0, -7, int(regs.reshape(-1)[regs.size // 2]), INT32_MIN)


@functools.lru_cache(maxsize=None)
def shrink_oracle(shape, win, fill):
    regs = shrink_map(shape)
    out = np.stack([R.shrink(r, win, fill) for r in regs])
    out.flags.writeable = False
    return out
