"""The label-path kernels of regda_amd/csrc/label_kernels.hip (pseudo_selection, LRH, the fused pass, downscale +
prototypes, label_refine with and without superpixels, teacher probabilities, class counts, the SAM region map): a Python
restatement of the host-side decisions that pick a route or cut a call into workgroups, a table of small cases that each
name the path they are there to reach, and plain numpy / torch-CPU references.

The restatement mirrors label_kernels.hip; tests/test_label_cases_cpu.py parses the constants it copies out of the
source, so a change there that is not made here fails on a machine without a GPU.

References: integer decisions in exact integer arithmetic, fp32 only where the reference itself decides in fp32 (the
thresholds f32(max) * top, the ratios count / s^2, m / (n + 1e-5f)); float outputs in fp64 from the fp32 inputs.  The
bilinear source index comes from the fp32 product scale * dst, as torch forms it (an fp64 index may floor differently at
an integer boundary; the interpolated value is continuous there, so indices are never compared).

Inputs are built on the CPU from fixed seeds; nothing here needs a GPU or the library.
"""
from collections import namedtuple

import numpy as np
import torch
import torch.nn.functional as F

# ---------------------------------------------------------------- the restatement (label_kernels.hip, common.h)
MIN_CLASSES, MAX_CLASSES = 6, 16     # RGDA_MIN_CLASSES / RGDA_MAX_CLASSES (pseudo_select alone serves 1 .. 16)
PSEUDO_CHUNK = 16384                 # rgda_pseudo_select: `int chunk = 16384;`, float4 route where hw % 4 == 0
LRH_CHUNK, LRH_CHUNK_MIN, LRH_MIN_WG = 16384, 2048, 512      # rgda_lrh: halved while fewer than 512 workgroups
PICK_CHUNK, PICK_CHUNK_MIN, PICK_MIN_WG = 16384, 1024, 512   # rgda_pseudo_lrh
HIST_LDS_BYTES = 48 * 1024           # lds_regions = min(R, 48 KB / (C * 4))
FUSED_MAX_REGIONS = 65535            # rgda_pseudo_lrh: region ids travel as 16 bits, 0xffff = out of range
DOWNSCALE_FAST_SCALE = 16            # `scale == 16 && !(w & 1)`: the one-workgroup-per-row kernels
DOWNSCALE_FAST_CLASSES = 7           # C <= 7: one 64-bit word of 9-bit fields; above: the wide kernel
REFINE_ROWS, REFINE_COLS = 8, 256    # refine_apply_kernel: output rows per workgroup, columns per block
REFINE_PX = 32                       # pearson_sim_kernel: low-res pixels per workgroup
REFINE_K_MAX = 4096
LDS_MAX = 160 * 1024                 # RGDA_LDS_MAX
LDS_ATTR = 64 * 1024                 # above: hipFuncAttributeMaxDynamicSharedMemorySize is set before the launch
OK, ERR_ARG, ERR_WORKSPACE, ERR_LAUNCH, ERR_UNSUPPORTED = 0, -1, -2, -3, -4


def cdiv(a, b):
    return -(-a // b)


def pseudo_route(hw):
    """pseudo_max_kernel -> (route, chunks)."""
    return ('vec' if hw % 4 == 0 and PSEUDO_CHUNK % 4 == 0 else 'scalar'), cdiv(hw, PSEUDO_CHUNK)


def lrh_chunk(hw, b):
    c = LRH_CHUNK
    while c > LRH_CHUNK_MIN and cdiv(hw, c) * b < LRH_MIN_WG:
        c >>= 1
    return c


def pick_chunk(hw, b):
    c = PICK_CHUNK
    while c > PICK_CHUNK_MIN and cdiv(hw, c) * b < PICK_MIN_WG:
        c >>= 1
    return c


def lds_regions(R, C):
    return min(R, HIST_LDS_BYTES // (C * 4))


def downscale_route(scale, w, C):
    if scale == DOWNSCALE_FAST_SCALE and not (w & 1):
        return 'fast' if C <= DOWNSCALE_FAST_CLASSES else 'wide'
    return 'generic'


def refine_slices(C):
    return 16 if C <= 14 else 8


def refine_kper(C, k):
    return cdiv(k, refine_slices(C))


def refine_lds(C, k):
    return (C * k + refine_slices(C) * REFINE_PX * (C + 1)) * 4


def refine_status(C, k, views):
    """What refine_run answers for (C, k) before it looks at the workspace."""
    if not MIN_CLASSES <= C <= MAX_CLASSES:
        return ERR_UNSUPPORTED
    if views & 1:
        if k < 2 or k > REFINE_K_MAX or k & 3:
            return ERR_ARG
        if refine_lds(C, k) > LDS_MAX:
            return ERR_UNSUPPORTED
    return OK


def refine_grid(H, W, b):
    return cdiv(W, REFINE_COLS), cdiv(H, REFINE_ROWS), b


def slice_shapes(C, k):
    """Per k-slice of pearson_sim_kernel: (terms in the 4-way unrolled sum, terms in the scalar tail)."""
    SL, kper = refine_slices(C), refine_kper(C, k)
    out = []
    for s in range(SL):
        k0 = min(s * kper, k)
        n = min(k0 + kper, k) - k0
        out.append((n // 4 * 4, n % 4))
    return out


# ---------------------------------------------------------------- references: pseudo_selection, LRH
def f32(x):
    return np.float32(x)


def pseudo_ref(soft, top=0.8, low=0.6, ignore_label=-1, classmax=None):
    """soft (b, c, h, w) f32 -> (labels (b, h, w) int64, flag, classmax (b, c) f32).  flag = 1 where the reference's
    `assert mask.max() <= 1 and mask.min() >= 0` fails: a value outside [0, 1] or a NaN."""
    soft = np.asarray(soft, np.float32)
    b, c, h, w = soft.shape
    m = soft.reshape(b, c, -1)
    flag = int(not bool(np.all((m >= 0) & (m <= 1))))
    if classmax is None:
        classmax = np.fmax(m, 0).max(-1).astype(np.float32) if m.shape[-1] else np.zeros((b, c), np.float32)
    thr = np.maximum((classmax.astype(np.float32) * f32(top)).astype(np.float32), f32(low))[:, :, None]
    g = m > thr
    lab = g.argmax(1).astype(np.int64)
    lab[g.sum(1) != 1] = ignore_label
    return lab.reshape(b, h, w), flag, classmax


def lrh_ref(labels, regions, percent, C, ignore_label, R):
    """(b, n) labels / region ids -> (out, flag): the histogram over the pixels with a region in [0, R) and a label in
    [0, C); flag bit 1 (value 1) for a region outside, bit 2 (value 2) for a label outside that is not ignore_label; per
    region n, m, the first argmax, f32(m) / (f32(n) + 1e-5f) < f32(percent) -> ignore; pixels of regions 1 .. R - 1 with
    an id take it, every other pixel keeps its label."""
    labels, regions = np.asarray(labels, np.int64), np.asarray(regions, np.int64)
    b = labels.shape[0]
    lab, reg = labels.reshape(b, -1), regions.reshape(b, -1)
    rok, lok = (reg >= 0) & (reg < R), (lab >= 0) & (lab < C)
    flag = (1 if (~rok).any() else 0) | (2 if (~lok & (lab != ignore_label)).any() else 0)
    out = np.empty_like(lab)
    for i in range(b):
        hist = np.zeros((R, C), np.int64)
        v = rok[i] & lok[i]
        np.add.at(hist, (reg[i][v], lab[i][v]), 1)
        n, m, ids = hist.sum(-1), hist.max(-1), hist.argmax(-1).astype(np.int64)
        ratio = m.astype(np.float32) / (n.astype(np.float32) + f32(1e-5))
        ids[ratio < f32(percent)] = ignore_label
        o = np.full(lab[i].shape, ignore_label, np.int64)
        g = (reg[i] > 0) & (reg[i] < R)
        o[g] = ids[reg[i][g]]
        out[i] = np.where(o == ignore_label, lab[i], o)
    return out.reshape(labels.shape), flag


# ---------------------------------------------------------------- references: downscale + prototypes
def downscale_ref(label, scale, C, ignore_label=-1, min_ratio=0.75):
    """(b, H, W) int64 -> (ds (b, 1, h, w) int64, cnt (C,) int64, flag, clean (b, h, w) bool): per cell the counts over
    C + 1 classes (ignore last), ratio = f32(count) / f32(s^2), the first maximum, ignore where it is the ignore class or
    ratio < f32(min_ratio).  flag = 2 for a label outside [0, C) that is not ignore_label; such a label is counted
    nowhere (the generic kernel) or as ignore (the 16 x 16 kernels from 7 classes on), so `clean` marks the cells that
    hold none: only those are compared."""
    label = np.asarray(label, np.int64)
    b, H, W = label.shape
    s = scale
    h, w = H // s, W // s
    cells = lambda a: a.reshape(b, h, s, w, s).transpose(0, 1, 3, 2, 4).reshape(b, h, w, s * s)
    bad = cells((label != ignore_label) & ((label < 0) | (label >= C)))
    blocks = cells(np.where(label == ignore_label, C, np.where((label < 0) | (label >= C), C + 1, label)))
    cnt = np.stack([(blocks == c).sum(-1) for c in range(C + 1)], -1)
    ratio = cnt.astype(np.float32) / f32(s * s)
    out = ratio.argmax(-1).astype(np.int64)
    mx = ratio.max(-1)
    out[out == C] = ignore_label
    out[mx < f32(min_ratio)] = ignore_label
    n = np.array([(out == c).sum() for c in range(C)], np.int64)
    return out[:, None], n, (2 if bad.any() else 0), ~bad.any(-1)


def downscale_exact(label, scale, C, ignore_label=-1, min_ratio=0.75):
    """The same decision in exact integers (count * 2^24 against s^2 * round(min_ratio * 2^24); every min_ratio of the
    table is a multiple of 2^-24): a case on which this differs from downscale_ref would depend on an fp32 rounding."""
    label = np.asarray(label, np.int64)
    b, H, W = label.shape
    s = scale
    h, w = H // s, W // s
    lab = np.where(label == ignore_label, C, label)
    blocks = lab.reshape(b, h, s, w, s).transpose(0, 1, 3, 2, 4).reshape(b, h, w, s * s)
    cnt = np.stack([(blocks == c).sum(-1) for c in range(C + 1)], -1)
    out = cnt.argmax(-1).astype(np.int64)
    mr = int(round(min_ratio * 2 ** 24))
    assert mr == min_ratio * 2 ** 24
    low = cnt.max(-1) * 2 ** 24 < s * s * mr
    out[out == C] = ignore_label
    out[low] = ignore_label
    return out[:, None]


def downscale_torch(label, scale, C, ignore_label=-1, min_ratio=0.75):
    """torch's own one_hot -> avg_pool2d -> max on the CPU (regda/gast/alignment.py:466-481), any scale."""
    lab = torch.as_tensor(label).long().clone()
    lab[lab == ignore_label] = C
    oh = F.one_hot(lab, C + 1).permute(0, 3, 1, 2).float()
    r = F.avg_pool2d(oh, kernel_size=scale)
    mx, idx = torch.max(r, dim=1, keepdim=True)
    idx[idx == C] = ignore_label
    idx[mx < min_ratio] = ignore_label
    return idx.numpy()


def proto_sums_ref(feat, ds, C, dtype=torch.float64):
    """feat (b, k, h, w) f32, ds (b, 1, h, w) -> (sums (C, k), cnt (C,)) in `dtype` (fp64: the reference)."""
    b, k = feat.shape[:2]
    f = torch.as_tensor(feat).to(dtype).permute(0, 2, 3, 1).reshape(-1, k)
    lab = torch.as_tensor(ds).reshape(-1)
    oh = torch.stack([(lab == c) for c in range(C)], 1).to(dtype)
    return oh.t() @ f, oh.sum(0)


def proto_apply_ref(protos, sums, cnt, decay, dtype=torch.float64):
    """local = sums / (n + 1e-7), the old prototype where n < 1, then (1 - decay) local + decay old."""
    p = torch.as_tensor(protos).to(dtype)
    n = cnt.to(dtype).unsqueeze(1).expand_as(sums)
    local = torch.where(n < 1, p, sums.to(dtype) / (n + 1e-7))
    d = float(np.float32(decay)) if dtype == torch.float64 else decay
    return (1.0 - d) * local + d * p


# ---------------------------------------------------------------- references: bilinear, label_refine, teacher
def lerp_ac(n_in, n_out):
    """align_corners=True source positions -> (i0, i1, l1): index from the fp32 product, as torch and the kernels."""
    scale = f32(n_in - 1) / f32(n_out - 1) if n_out > 1 else f32(0)
    src = (scale * np.arange(n_out, dtype=np.float32)).astype(np.float32)
    i0 = src.astype(np.int64)
    i1 = i0 + (i0 < n_in - 1)
    l1 = (src - i0.astype(np.float32)).astype(np.float64)
    return torch.from_numpy(i0), torch.from_numpy(i1), torch.from_numpy(l1)


def bilinear64(x, H, W):
    x = x.double()
    h, w = x.shape[-2:]
    y0, y1, ly = lerp_ac(h, H)
    x0, x1, lx = lerp_ac(w, W)
    r0, r1 = x[:, :, y0], x[:, :, y1]
    top = r0[..., x0] * (1 - lx) + r0[..., x1] * lx
    bot = r1[..., x0] * (1 - lx) + r1[..., x1] * lx
    return top * (1 - ly)[:, None] + bot * ly[:, None]


def pearson64(f1, f2):
    """(n, k), (m, k) f32 -> (n, m) fp64 (regda/gast/alignment.py:396-423)."""
    f1, f2 = f1.double(), f2.double()
    k = f1.shape[-1]
    c1, c2 = f1 - f1.mean(-1, keepdim=True), f2 - f2.mean(-1, keepdim=True)
    cov = c1 @ c2.t() / (k - 1 + 1e-7)
    return (-cov / (f1.std(-1).unsqueeze(1) * f2.std(-1).unsqueeze(0) + 1e-7) + 1.0) * 0.5


def feat_dist(feat, protos):
    b, k, h, w = feat.shape
    return pearson64(feat.permute(0, 2, 3, 1).reshape(-1, k), protos)


def sup_weight64(sup, soft, temp):
    """-> (weight (b, c, H, W) fp64, ignored (b, 1, H, W)): per (image, id, class) the maximum of the soft labels (exact),
    softmax(. / temp) over the classes, divided by its maximum + 1e-7; the batch's largest id is `ignored`."""
    b, c, H, W = soft.shape
    ids = sup.reshape(b, -1).long()
    top = int(ids.max())
    src = soft.double().permute(0, 2, 3, 1).reshape(b, -1, c)
    idx = ids.unsqueeze(-1).expand(-1, -1, c)
    table = torch.full((b, top + 1, c), float('-inf'), dtype=torch.float64)
    table.scatter_reduce_(1, idx, src, reduce='amax')
    prob = torch.softmax(torch.gather(table, 1, idx).reshape(b, H, W, c).permute(0, 3, 1, 2) / temp, 1)
    return prob / (prob.max(1, keepdim=True)[0] + 1e-7), (ids == top).reshape(b, 1, H, W)


def refine_ref(feat, protos, p1, p2, soft, sup=None, temp=2.0, views=3):
    """label_refine in fp64.  views bit 0: the prototype view, bit 1: the prediction view; `sup`: the superpixel view on
    top (alignment.py:194-265).  No view at all with superpixels: weight ones (mode 's')."""
    H, W = soft.shape[-2:]
    weight = None
    if views & 1:
        b, k, h, w = feat.shape
        sim = (1.0 / feat_dist(feat, protos)).view(b, h, w, -1).permute(0, 3, 1, 2)
        pw = torch.softmax(bilinear64(sim, H, W), 1)
        weight = pw / (pw.max(1, keepdim=True)[0] + 1e-7)
    if views & 2:
        lw = (torch.softmax(bilinear64(p1, H, W) / temp, 1) + torch.softmax(bilinear64(p2, H, W) / temp, 1)) * 0.5
        lw = lw / (lw.max(1, keepdim=True)[0] + 1e-7)
        weight = lw if weight is None else weight + lw
    if sup is not None:
        sw, ign = sup_weight64(sup, soft, temp)
        weight = torch.where(ign, torch.ones_like(sw), sw) if weight is None else torch.where(ign, weight, weight * sw)
    out = weight * soft.double()
    return out / (out.sum(1, keepdim=True) + 1e-7)


def refine_oracle32(feat, protos, p1, p2, soft, sup=None, temp=2.0, views=3):
    """The same formula in torch fp32, from the pieces of oracle/labelpath.py (its label_refine has no mode for one view
    with superpixels; where it has a mode this equals it, see tests/test_label_cases_cpu.py)."""
    from oracle import labelpath as op
    H, W = soft.shape[-2:]
    weight = None
    if views & 1:
        b, k, h, w = feat.shape
        simi = 1.0 / op.pearson_dist(feat.permute(0, 2, 3, 1).reshape(-1, k), protos)
        simi = F.interpolate(simi.view(b, h, w, -1).permute(0, 3, 1, 2), (H, W), mode='bilinear', align_corners=True)
        pw = op.softmax_T(simi, 1, 1)
        weight = 0 + pw / (pw.max(dim=1, keepdim=True)[0] + 1e-7)
    if views & 2:
        x1 = F.interpolate(p1, (H, W), mode='bilinear', align_corners=True)
        x2 = F.interpolate(p2, (H, W), mode='bilinear', align_corners=True)
        lw = (op.softmax_T(x1, temp, 1) + op.softmax_T(x2, temp, 1)) * 0.5
        lw = lw / (lw.max(dim=1, keepdim=True)[0] + 1e-7)
        weight = 0 + lw if weight is None else weight + lw
    if sup is not None:
        sw, ign = op.superpixel_weight(sup, soft, temp)
        weight = torch.where(ign, torch.ones_like(sw), sw) if weight is None else torch.where(ign, weight, weight * sw)
    out = weight * soft
    return out / (out.sum(dim=1, keepdim=True) + op.EPS)


def teacher_ref(p1, p2, size):
    H, W = size
    return (torch.softmax(bilinear64(p1, H, W), 1) + torch.softmax(bilinear64(p2, H, W), 1)) / 2


# ---------------------------------------------------------------- references: class counts, SAM region map
def class_count_ref(label, C):
    lab = np.asarray(label, np.int64).reshape(-1)
    return np.array([(lab == c).sum() for c in range(C)], np.int32)


def regions_ref(masks, areas, thr):
    """1 + the LAST mask index with areas >= thr that covers the pixel, else 0."""
    masks = np.asarray(masks).astype(bool)
    K = masks.shape[0]
    out = np.zeros(masks.shape[1:], np.int32)
    for k in range(K):
        if areas[k] >= thr:
            out = np.where(masks[k], np.int32(k + 1), out)
    return out


# ================================================================ the cases
def _rng(*key):
    import zlib
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


# ---------------------------------------------------------------- pseudo_select
# kind: 'rand' (softmax noise), 'edge' (the constructed threshold pixels), 'ready' (classmax_ready = 1 with maxima of the
# caller's), 'above' / 'below' / 'nan' (one value outside [0, 1] in the LAST chunk: flag only)
PseudoCase = namedtuple('PseudoCase', 'name b c shape kind paths')
PSEUDO_CASES = [
    PseudoCase('hw1', 1, 1, (1, 1), 'rand', ('scalar', 'c_1')),
    PseudoCase('hw63', 2, 5, (1, 63), 'rand', ('scalar', 'c_5')),
    PseudoCase('hw255', 3, 6, (5, 51), 'rand', ('scalar', 'c_6')),
    PseudoCase('hw1000', 2, 7, (8, 125), 'rand', ('vec', 'c_7')),
    PseudoCase('tail4', 1, 16, (1, 16384 + 4), 'rand', ('vec', 'vec_tail_chunk', 'c_16')),
    PseudoCase('two_chunks', 2, 6, (129, 129), 'rand', ('scalar', 'scalar_two_chunks')),
    PseudoCase('edge', 2, 6, (3, 85), 'edge', ('threshold_equal', 'threshold_next', 'two_pass', 'low_dominates')),
    PseudoCase('ready', 2, 7, (8, 125), 'ready', ('classmax_ready',)),
]
PSEUDO_FLAG_CASES = [PseudoCase('%s_%s' % (kind, route), 2, 6, shape, kind, ('flag_%s_%s' % (kind, route),))
                     for route, shape in (('scalar', (129, 129)), ('vec', (1, 16384 + 4)))
                     for kind in ('above', 'below', 'nan')]
EDGE_TOP, EDGE_LOW = 0.8, 0.6


def pseudo_inputs(case):
    """-> (soft (b, c, h, w) f32, classmax (b, c) f32 or None)."""
    rng = _rng('pseudo', case.name)
    b, c, (h, w) = case.b, case.c, case.shape
    z = rng.standard_normal((b, c, h, w)).astype(np.float32) * 3
    soft = np.exp(z - z.max(1, keepdims=True))
    soft = (soft / soft.sum(1, keepdims=True)).astype(np.float32)
    if c == 1:
        soft = rng.random((b, c, h, w)).astype(np.float32) * f32(0.5) + f32(0.5)
    soft = np.clip(soft, 0, 1)
    cm = None
    if case.kind == 'edge':
        # nothing of the noise passes (all < 0.45 < low); image 0's first pixels are built around the thresholds
        soft = (soft * f32(0.45)).astype(np.float32)
        m = soft.reshape(b, c, -1)
        m[0, :, :8] = 0
        m[0, 0, 0] = 1.0                                            # class 0: max 1.0, threshold f32(1.0 * 0.8)
        m[0, 0, 1] = f32(EDGE_TOP)                                  # exactly the threshold: not above it
        m[0, 0, 2] = np.nextafter(f32(EDGE_TOP), f32(1))            # the next float: labelled
        m[0, 0, 3] = m[0, 1, 3] = 0.9                               # classes 0 and 1 both pass: ignore
        m[0, 2, 4] = 0.55                                           # class 2: max 0.55, 0.44 < low = 0.6 decides
        m[0, 1, 5] = 0.75                                           # class 1 (max 0.9 -> 0.72) alone: labelled 1
    elif case.kind == 'ready':
        cm = (rng.random((b, c)) * 0.5 + 0.5).astype(np.float32)    # NOT the maxima of soft: the route must use these
    elif case.kind in ('above', 'below', 'nan'):
        v = {'above': np.nextafter(f32(1), f32(2)), 'below': -np.finfo(np.float32).tiny, 'nan': f32('nan')}[case.kind]
        soft.reshape(b, c, -1)[b - 1, c - 1, h * w - 1] = v         # the last pixel of the last plane: the last chunk
    return soft, cm


# ---------------------------------------------------------------- LRH (two-call) and the fused pass
LrhCase = namedtuple('LrhCase', 'name b hw C R percent ignore kind paths')
LRH_CASES = [
    LrhCase('hw1', 1, 1, 6, 8, 0.5, -1, 'rand', ('hw_1',)),
    LrhCase('hw5', 2, 5, 7, 4096, 0.5, -1, 'rand', ('c_7',)),
    LrhCase('hw64', 2, 64, 16, 1024, 0.5, -1, 'rand', ('c_16', 'one_wave')),
    LrhCase('hw257', 2, 257, 6, 4096, 0.5, -1, 'built',
            ('run_across_waves', 'run_cut_by_ignore', 'alternating', 'run_ends_at_invalid_lane', 'global_hist',
             'ratio_both_sides', 'all_ignored_region', 'region_0')),
    LrhCase('hw2049', 2, 2049, 16, 1024, 0.5, 255, 'built',
            ('one_pixel_last_chunk', 'global_hist', 'ignore_255', 'run_across_waves', 'c_16')),
    LrhCase('hw4097', 1, 4097, 7, 4096, 0.5, -1, 'built', ('one_pixel_last_chunk', 'three_chunks', 'global_hist')),
    LrhCase('percent0', 1, 2049, 6, 4096, 0.0, -1, 'built', ('percent_0', 'all_ignored_region')),
    LrhCase('percent1', 1, 2049, 6, 4096, 1.0, -1, 'built', ('percent_1',)),
    LrhCase('flag_region', 1, 257, 6, 64, 0.5, -1, 'bad_region', ('flag_bit_1', 'run_cut_by_bad_region')),
    LrhCase('flag_label', 1, 257, 6, 64, 0.5, -1, 'bad_label', ('flag_bit_2',)),
]
FusedCase = namedtuple('FusedCase', 'name b hw C R percent ignore kind paths')
FUSED_CASES = [
    FusedCase('hw4', 1, 4, 6, 8, 0.5, -1, 'rand', ('one_lane', 'grid_1')),
    FusedCase('hw1020', 2, 1020, 7, 4096, 0.5, -1, 'built', ('grid_1', 'same_and_mixed_waves', 'global_hist')),
    FusedCase('hw1028', 2, 1028, 6, 65535, 0.5, -1, 'built', ('four_pixel_last_chunk', 'max_regions_65535', 'global_hist')),
    FusedCase('hw2052', 1, 2052, 16, 1024, 0.5, 255, 'built', ('three_chunks', 'ignore_255', 'global_hist', 'c_16')),
    FusedCase('hw4100', 2, 4100, 6, 4096, 0.5, -1, 'built', ('four_pixel_last_chunk', 'same_and_mixed_waves')),
    FusedCase('fp0', 1, 2052, 6, 4096, 0.0, -1, 'built', ('percent_0',)),
    FusedCase('fp1', 1, 2052, 6, 4096, 1.0, -1, 'built', ('percent_1',)),
    FusedCase('fflag', 1, 1028, 6, 64, 0.5, -1, 'bad_region', ('flag_bit_1',)),
]


def _runs(rng, n, values, lo, hi):
    out = np.empty(n, np.int64)
    i = 0
    while i < n:
        L = int(rng.integers(lo, hi + 1))
        out[i:i + L] = values[int(rng.integers(0, len(values)))]
        i += L
    return out


def special_regions(R, C):
    """The region ids the built cases place: the last LDS-resident region, the first global one, the last of the table."""
    L = lds_regions(R, C)
    return [max(1, L - 1), min(L, R - 1), R - 1]


def lrh_inputs(case, fused=False):
    """-> (labels (b, 1, hw) int64, regions (b, 1, hw) int64).  'built' lays these over piecewise-constant noise (image 0,
    from pixel 0; the lane of pixel i is i % 64 because every chunk is a multiple of 256):
       60 .. 67   one key across the lane 63 -> 0 boundary            (region A)
       70 .. 80   one key, pixel 75 ignored                           (region A)
       96 .. 99   [c0, c1, c1, c1]: one lane's four pixels differ     (region B: n 4, m 3 -> c1)
      104 .. 105  [c0, c1]: n 2, m 1, 1 / (2 + 1e-5) < 0.5 -> ignore  (region D)
      108 .. 110  only ignored pixels                                  (region E)
      128 .. 191  keys alternating lane by lane                        (region F)
    and in the fused form pixels 256 .. 511 in runs of 16 (every lane's four pixels share a key)."""
    rng = _rng('lrh', case.name, fused)
    b, n, C, R, ig = case.b, case.hw, case.C, case.R, case.ignore
    sp = special_regions(R, C)
    ids = [0, 1, 2, 3] + sp + [int(x) for x in rng.integers(1, R, 6)]
    lab = np.stack([_runs(rng, n, list(range(C)) + [ig], 1, 24) for _ in range(b)])
    reg = np.stack([_runs(rng, n, ids, 1, 40) for _ in range(b)])
    noise = rng.random((b, n)) < 0.1
    lab = np.where(noise, rng.integers(0, C, (b, n)), lab)
    if case.kind in ('built', 'bad_region', 'bad_label') and n >= 257:
        free = [r for r in range(4, R) if r not in ids][:5]
        A, B, D, E, Fr = free
        reg[0, :256] = np.where(np.isin(reg[0, :256], free), 1, reg[0, :256])
        lab[0, 60:68], reg[0, 60:68] = 2, A
        lab[0, 70:81], reg[0, 70:81] = 2, A
        lab[0, 75] = ig
        lab[0, 96:100], reg[0, 96:100] = [0, 1, 1, 1], B
        lab[0, 104:106], reg[0, 104:106] = [0, 1], D
        lab[0, 108:111], reg[0, 108:111] = ig, E
        lab[0, 128:192], reg[0, 128:192] = np.arange(64) % 2 + 3, Fr
        reg[0, 200:210], lab[0, 200:210] = sp[0], C - 1
        reg[0, 210:220], lab[0, 210:220] = sp[1], 0
        reg[0, 220:230], lab[0, 220:230] = sp[2], 1
        reg[0, 230:240] = 0
        if fused and n >= 512:
            lab[0, 256:512] = np.repeat(rng.integers(0, C, 16), 16)
            reg[0, 256:512] = np.repeat(rng.choice(ids, 16), 16)
        reg[:, n - 1], lab[:, n - 1] = sp[1], 2                     # the last pixel (a chunk of its own where hw = 2^k + 1)
    if case.kind == 'bad_region':
        lab[0, 64:80], reg[0, 64:80] = 1, 5
        reg[0, 72] = R                                              # cuts the run; left unchanged
        reg[0, 20] = -1
    if case.kind == 'bad_label':
        lab[0, 64:80], reg[0, 64:80] = 1, 5
        lab[0, 70], lab[0, 71] = C, -2
    return lab.reshape(b, 1, n), reg.reshape(b, 1, n)


def soft_from_labels(lab, C, ignore, seed):
    """Soft labels whose pseudo_selection (top 0.8, low 0.6) is `lab`: 0.9 + noise on the class, <= 0.05 elsewhere; an
    ignored pixel has two classes above the threshold or none."""
    rng = _rng('soft', seed)
    b, _, n = lab.shape
    soft = (rng.random((b, C, n)) * 0.05).astype(np.float32)
    for i in range(b):
        for p in range(n):
            l = lab[i, 0, p]
            if l != ignore:
                soft[i, l, p] = 0.9 + 0.1 * rng.random()
            elif p % 2:
                soft[i, 0, p] = soft[i, C - 1, p] = 0.95
    return soft.reshape(b, C, 1, n)


# ---------------------------------------------------------------- downscale + prototypes
# cells: a cycle of constructed compositions (see ds_inputs) over random ones.  k: feature channels.
DsCase = namedtuple('DsCase', 'name b h w scale C min_ratio k paths')
DS_CASES = [
    DsCase('s2', 3, 3, 5, 2, 6, 0.75, 4, ('generic', 'scale_2', 'hw_15', 'k_4')),
    DsCase('s2_300', 2, 10, 30, 2, 6, 0.5, 260, ('generic', 'hw_300', 'k_260', 'ties_visible')),
    DsCase('s3', 2, 2, 3, 3, 7, 0.75, 4, ('generic', 'scale_3')),
    DsCase('s8', 2, 3, 2, 8, 16, 0.5, 4, ('generic', 'scale_8', 'ties_visible')),
    DsCase('s16_w1', 1, 1, 1, 16, 6, 0.75, 1, ('generic', 'scale_16_odd_w', 'hw_1', 'k_1')),
    DsCase('s16_w3', 2, 1, 3, 16, 8, 0.5, 4, ('generic', 'scale_16_odd_w', 'ties_visible')),
    DsCase('s32', 1, 1, 2, 32, 7, 0.75, 4, ('generic', 'scale_32_loop')),
    DsCase('f6_w2', 3, 1, 2, 16, 6, 0.75, 4, ('fast', 'c_6', 'part_workgroup', 'h_1')),
    DsCase('f7_w34', 3, 3, 34, 16, 7, 0.75, 4, ('fast', 'c_7', 'second_x_block', 'h_3')),
    DsCase('f7_w2', 3, 3, 2, 16, 7, 0.5, 260, ('fast', 'c_7', 'ties_visible')),
    DsCase('f6_w34', 3, 1, 34, 16, 6, 0.5, 4, ('fast', 'c_6', 'second_x_block', 'ties_visible')),
    DsCase('w8_w34', 3, 3, 34, 16, 8, 0.75, 4, ('wide', 'c_8', 'second_x_block')),
    DsCase('w14_w2', 3, 1, 2, 16, 14, 0.75, 4, ('wide', 'c_14', 'part_workgroup')),
    DsCase('w15_w2', 3, 3, 2, 16, 15, 0.5, 4, ('wide', 'c_15', 'ties_visible')),
    DsCase('w16_w34', 3, 1, 34, 16, 16, 0.5, 260, ('wide', 'c_16', 'ties_visible')),
]
DS_ABSENT = 1        # the class no constructed or random cell ever wins: its prototype must stay


def ds_cell_kinds(s2, min_ratio):
    """The constructed cells as (name, [(class or 'ign' or 'last' or 'a' / 'b', count) ...]) for cells of s2 pixels."""
    q = next(n for n in range(s2 + 1) if f32(n) / f32(s2) >= f32(min_ratio))       # the smallest count that is kept
    kinds = [('exact', [('a', q), ('ign', s2 - q)]), ('below', [('a', q - 1), ('b', (s2 - q + 1) // 2), ('ign', s2 - q + 1 - (s2 - q + 1) // 2)]),
             ('all_ign', [('ign', s2)]), ('last', [('last', s2)])]
    if s2 % 2 == 0:
        kinds += [('tie_ign', [('a', s2 // 2), ('ign', s2 // 2)]), ('tie_classes', [('b', s2 // 2), ('a', s2 // 2)])]
    return kinds


def ds_inputs(case, bad=None):
    """-> (label (b, h * s, w * s) int64, feat (b, k, h, w) f32, protos (C, k) f32, kinds (b, h, w) of cell names).
    `bad`: a label outside [0, C) that is not ignore put into the LAST cell (flag only)."""
    rng = _rng('ds', case.name)
    b, h, w, s, C = case.b, case.h, case.w, case.scale, case.C
    s2 = s * s
    kinds = ds_cell_kinds(s2, case.min_ratio)
    classes = [c for c in range(C) if c != DS_ABSENT]
    label = np.empty((b, h, w, s2), np.int64)
    names = np.empty((b, h, w), object)
    for n, (i, y, x) in enumerate(np.ndindex(b, h, w)):
        a, bb = (int(v) for v in rng.choice(classes, 2, replace=False))
        a, bb = max(a, bb), min(a, bb)                              # 'b' < 'a': the FIRST of two tied classes is b
        sel = n % (len(kinds) + 2)
        if sel < len(kinds):
            names[i, y, x], comp = kinds[sel]
            cell = np.concatenate([np.full(cnt, {'a': a, 'b': bb, 'ign': -1, 'last': C - 1}[c]) for c, cnt in comp])
        else:
            names[i, y, x] = 'rand'
            cell = np.where(rng.random(s2) < 0.8, a, rng.choice(classes + [-1], s2))
        label[i, y, x] = rng.permutation(cell)
    if bad is not None:
        label[b - 1, h - 1, w - 1, s2 - 1] = bad
    label = label.reshape(b, h, w, s, s).transpose(0, 1, 3, 2, 4).reshape(b, h * s, w * s)
    feat = rng.standard_normal((b, case.k, h, w)).astype(np.float32)
    protos = rng.standard_normal((C, case.k)).astype(np.float32)
    return label, feat, protos, names


def cells_as_column(label, s):
    """The same cells stacked into one column (b' = 1, w' = 1: odd, so the generic kernel serves it at scale 16 too)."""
    b, H, W = label.shape
    h, w = H // s, W // s
    return label.reshape(b, h, s, w, s).transpose(0, 1, 3, 2, 4).reshape(1, b * h * w * s, s)


# ---------------------------------------------------------------- label_refine, teacher_probs
SHAPES = [(3, 5, 13, 300), (1, 4, 8, 257), (4, 1, 20, 7), (2, 2, 2, 2), (4, 4, 64, 64), (3, 3, 41, 513)]
RefineCase = namedtuple('RefineCase', 'name b C k shape views sup temp paths')
REFINE_CASES = [
    RefineCase('k4096_lds', 2, 6, 4096, SHAPES[0], 3, False, 2.0, ('lds_attr', 'ok_guard', 'W_ragged_2_blocks', 'H_not_8', 'k_4096', 'non_integer_scale')),
    RefineCase('k4_h1', 2, 7, 4, SHAPES[1], 3, False, 2.0, ('empty_slices', 'h_1', 'W_257', 'k_4', 'c_7')),
    RefineCase('k36_w1', 3, 15, 36, SHAPES[2], 1, False, 2.0, ('tail_4_plus_1', 'w_1', 'views_1', 'slices_8', 'c_15')),
    RefineCase('k68_same', 2, 14, 68, SHAPES[3], 3, False, 1.5, ('tail_4_plus_1', 'H_eq_h', 'k_68', 'c_14')),
    RefineCase('c16_k2048', 1, 16, 2048, SHAPES[4], 3, False, 2.0, ('slices_8', 'lds_attr', 'ok_guard', 'c_16', 'k_2048')),
    RefineCase('views2', 2, 7, 4, SHAPES[5], 2, False, 1.5, ('views_2', 'W_ragged_3_blocks', 'H_not_8')),
    RefineCase('k36_tail', 1, 6, 36, SHAPES[5], 3, False, 2.0, ('tail_only', 'W_ragged_3_blocks', 'row_pair_changes', 'k_36')),
    RefineCase('c15_k2048', 1, 15, 2048, SHAPES[0], 1, False, 2.0, ('slices_8', 'lds_attr', 'ok_guard', 'views_1')),
    RefineCase('sup_all', 2, 6, 36, SHAPES[4], 3, True, 2.0, ('sup_views_3', 'sup_whole_and_mixed_waves')),
    RefineCase('sup_s', 2, 7, 4, SHAPES[0], 0, True, 1.5, ('sup_views_0', 'sup_ragged')),
    RefineCase('sup_p', 1, 16, 4, SHAPES[5], 1, True, 2.0, ('sup_views_1', 'c_16')),
    RefineCase('sup_l', 2, 14, 4, SHAPES[1], 2, True, 2.0, ('sup_views_2',)),
]
TEACHER_CASES = [(2, (6, 7, 16, 6, 7, 16)[i], SHAPES[i]) for i in range(len(SHAPES))]
# Floor of pearson_dist in a float case.  sim = 1 / dist turns an error e of dist into e / dist^2: at dist >= 0.1 a
# rounding error is amplified at most 100-fold and sim <= 10, so the softmax over the classes stays unsaturated and the
# per-element bound means something.  (The golden test keeps the one pixel with dist ~ 1e-7, where every implementation
# saturates to one-hot.)  Short feature vectors correlate by chance (k = 4: dist is uniform in [0, 1]), so refine_inputs
# redraws a pixel whose distance to any prototype is below the floor.
DIST_FLOOR = 0.1


def sup_map(b, H, W, rng):
    """Superpixel ids: a coarse grid (waves of 64 pixels mixing ids), whole rows of one id where W allows 64-pixel waves
    inside one superpixel, single-pixel superpixels, an id used in image 0 only, and the batch's largest id (ignored) in
    the last image only."""
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing='ij')
    gw = cdiv(W, 8)
    base = (yy // 4) * gw + xx // 8
    sup = np.stack([base.copy() for _ in range(b)]).astype(np.int64)
    top = int(sup.max())
    flat = sup.reshape(b, -1)
    n = H * W
    if n >= 512:
        flat[:, 128:320] = top + 1                                  # three whole waves inside one superpixel
    for j, p in enumerate(rng.choice(n, min(5, n), replace=False)):
        flat[0, p] = top + 2 + j                                    # single pixels, image 0 only
    flat[b - 1, n // 2:n // 2 + max(1, n // 16)] = top + 10         # the batch's largest id: ignored
    return sup.reshape(b, 1, H, W)


def refine_inputs(case):
    """-> dict(feat, protos, p1, p2, soft, sup) of CPU tensors (those the views do not use are None)."""
    rng = _rng('refine', case.name)
    g = torch.Generator().manual_seed(int(rng.integers(1 << 30)))
    b, C, k, (h, w, H, W) = case.b, case.C, case.k, case.shape
    out = dict(feat=None, protos=None, p1=None, p2=None, sup=None)
    if case.views & 1:
        protos = torch.randn(C, k, generator=g)
        feat = torch.randn(b, k, h, w, generator=g)
        for _ in range(200):
            low = (feat_dist(feat, protos) < DIST_FLOOR * 1.2).any(1).view(b, h, w)
            if not low.any():
                break
            feat = torch.where(low[:, None], torch.randn(b, k, h, w, generator=g), feat)
        out.update(feat=feat, protos=protos)
    if case.views & 2:
        out.update(p1=torch.randn(b, C, h, w, generator=g) * 2, p2=torch.randn(b, C, h, w, generator=g) * 2)
    soft = torch.softmax(torch.randn(b, C, H, W, generator=g) * 3, 1)
    if case.sup:
        soft = torch.where(torch.rand(b, C, H, W, generator=g) < 0.1, torch.zeros(()), soft)     # exact zeros
        out['sup'] = torch.from_numpy(sup_map(b, H, W, rng))
    out['soft'] = soft.contiguous()
    return out


def teacher_inputs(i):
    b, C, (h, w, H, W) = TEACHER_CASES[i]
    g = torch.Generator().manual_seed(900 + i)
    return torch.randn(b, C, h, w, generator=g) * 3, torch.randn(b, C, h, w, generator=g) * 3, (H, W)


# the refusals refine_run states: (name, entry point, k, C, views, ws_short, status)
REFINE_REFUSALS = [
    ('k2', 'views', 2, 6, 3, False, ERR_ARG), ('k6', 'views', 6, 6, 3, False, ERR_ARG),
    ('k4100', 'views', 4100, 6, 3, False, ERR_ARG), ('c16_k4096', 'views', 4096, 16, 3, False, ERR_UNSUPPORTED),
    ('views0', 'views', 8, 6, 0, False, ERR_ARG), ('views4', 'views', 8, 6, 4, False, ERR_ARG),
    ('sup_views4', 'sup', 8, 6, 4, False, ERR_ARG), ('sup_views_neg', 'sup', 8, 6, -1, False, ERR_ARG),
    ('ws_small', 'views', 8, 6, 3, True, ERR_WORKSPACE), ('sup_ws_small', 'sup', 8, 6, 3, True, ERR_WORKSPACE),
]

# ---------------------------------------------------------------- class_count, masks_to_regions
COUNT_CASES = [(1, 6), (255, 16), (2049, 7)]


def count_inputs(n, C):
    return _rng('count', n, C).choice(list(range(-2, C + 2)) + [255], n).astype(np.int64)


# (name, K, HW, kind): 'rand', 'under' (every mask under the threshold), 'last' (overlapping kept masks)
REGION_CASES = [('k0', 0, 15, 'rand'), ('hw1', 3, 1, 'rand'), ('hw15', 5, 15, 'rand'), ('hw17', 5, 17, 'last'),
                ('hw4097', 7, 4097, 'last'), ('under', 4, 17, 'under')]
REGION_THR = 4


def region_inputs(name, K, HW, kind):
    """-> (masks (K, 1, HW) uint8, areas (K,) int64, thr)."""
    rng = _rng('regions', name)
    masks = (rng.random((K, 1, HW)) < 0.4).astype(np.uint8)
    if kind == 'last' and K >= 2:
        masks[K - 1, 0, HW // 2:] = 1
        masks[K - 2, 0, :] = 1                                      # the last two overlap: the last one wins
    areas = masks.reshape(K, HW).sum(1).astype(np.int64)
    if kind == 'under':
        areas[:] = REGION_THR - 1
    if HW == 1:
        areas[:] = np.array([REGION_THR, REGION_THR - 1, REGION_THR])[:K]
        masks[:, 0, 0] = [1, 1, 0][:K]
    return masks, areas, REGION_THR


# ---------------------------------------------------------------- which case reaches which path
def paths_reached():
    """{path: [case names]} according to the restatement and the built inputs."""
    out = {}

    def add(p, name):
        out.setdefault(p, []).append(name)

    for c in PSEUDO_CASES + PSEUDO_FLAG_CASES:
        hw = c.shape[0] * c.shape[1]
        route, chunks = pseudo_route(hw)
        add(route, c.name)
        add('c_%d' % c.c, c.name)
        if route == 'vec' and chunks == 2 and hw - PSEUDO_CHUNK == 4:
            add('vec_tail_chunk', c.name)
        if route == 'scalar' and chunks == 2:
            add('scalar_two_chunks', c.name)
        if c.kind == 'ready':
            add('classmax_ready', c.name)
        if c.kind in ('above', 'below', 'nan'):
            soft, _ = pseudo_inputs(c)
            m = soft.reshape(c.b * c.c, -1)
            pos = np.argwhere(~((m >= 0) & (m <= 1)))
            if len(pos) == 1 and pos[0][1] >= (chunks - 1) * PSEUDO_CHUNK and chunks > 1:
                add('flag_%s_%s' % (c.kind, route), c.name)
        if c.kind == 'edge':
            soft, _ = pseudo_inputs(c)
            lab, flag, cm = pseudo_ref(soft, EDGE_TOP, EDGE_LOW)
            l0 = lab.reshape(c.b, -1)[0]
            thr0 = f32(cm[0, 0]) * f32(EDGE_TOP)
            m = soft.reshape(c.b, c.c, -1)[0]
            if m[0, 1] == thr0 and l0[1] == -1:
                add('threshold_equal', c.name)
            if m[0, 2] == np.nextafter(thr0, f32(1)) and l0[2] == 0:
                add('threshold_next', c.name)
            if l0[3] == -1 and (m[:, 3] > 0.8).sum() == 2:
                add('two_pass', c.name)
            if l0[4] == -1 and m[2, 4] > f32(cm[0, 2]) * f32(EDGE_TOP) and l0[5] == 1:
                add('low_dominates', c.name)
    for fused, cases in ((False, LRH_CASES), (True, FUSED_CASES)):
        for c in cases:
            lab, reg = lrh_inputs(c, fused)
            lab, reg = lab.reshape(c.b, -1), reg.reshape(c.b, -1)
            name = ('fused:' if fused else '') + c.name
            chunk = pick_chunk(c.hw, c.b) if fused else lrh_chunk(c.hw, c.b)
            L = lds_regions(c.R, c.C)
            valid = (reg >= 0) & (reg < c.R) & (lab >= 0) & (lab < c.C)
            key = np.where(valid, reg * c.C + lab, -1)
            add('c_%d' % c.C, name)
            if c.hw == 1:
                add('hw_1', name)
            if c.hw <= 64:
                add('one_wave', name)
            if c.ignore == 255:
                add('ignore_255', name)
            if c.percent in (0.0, 1.0):
                add('percent_%d' % c.percent, name)
            if cdiv(c.hw, chunk) == 1:
                add('grid_1', name)
            if cdiv(c.hw, chunk) == 3:
                add('three_chunks', name)
            if c.hw % chunk == 1:
                add('one_pixel_last_chunk', name)
            if c.hw % chunk == 4:
                add('four_pixel_last_chunk', name)
            if c.hw == 4:
                add('one_lane', name)
            if ((reg >= L) & valid).any() and ((reg == L - 1) & valid).any() and ((reg == c.R - 1) & valid).any():
                add('global_hist', name)
            if c.R == FUSED_MAX_REGIONS and (reg == c.R - 1).any():
                add('max_regions_65535', name)
            f = lrh_ref(lab, reg, c.percent, c.C, c.ignore, c.R)[1]
            if f == 1:
                add('flag_bit_1', name)
            if f == 2:
                add('flag_bit_2', name)
            if c.hw >= 257:
                k0 = key[0]
                if k0[60] >= 0 and (k0[60:68] == k0[60]).all() and k0[59] != k0[60] and k0[68] != k0[60]:
                    add('run_across_waves', name)
                if k0[75] == -1 and k0[74] == k0[76] >= 0 and lab[0, 75] == c.ignore:
                    add('run_cut_by_ignore', name)
                if (k0[128:191] != k0[129:192]).all() and (k0[128:192] >= 0).all():
                    add('alternating', name)
                if (c.hw - 1) % 256 == 0 and k0[c.hw - 1] >= 0:
                    add('run_ends_at_invalid_lane', name)
                if not fused:
                    o = lrh_ref(lab, reg, c.percent, c.C, c.ignore, c.R)[0].reshape(c.b, -1)[0]
                    if (o[96:100] == lab[0, 97]).all() and o[96] != lab[0, 96] and (o[104:106] == lab[0, 104:106]).all():
                        add('ratio_both_sides', name)
                    if (lab[0, 108:111] == c.ignore).all() and (reg[0] == reg[0, 108]).sum() == 3:
                        add('all_ignored_region', name)
                    if (reg[0, 230:240] == 0).all() and (o[230:240] == lab[0, 230:240]).all():
                        add('region_0', name)
                if c.kind == 'bad_region' and reg[0, 72] == c.R and k0[71] == k0[73] >= 0:
                    add('run_cut_by_bad_region', name)
                if fused and c.hw >= 512:
                    q = key[0, :c.hw // 4 * 4].reshape(-1, 4)
                    same = (q == q[:, :1]).all(1)
                    waves = [same[i:i + 64].all() for i in range(0, len(same), 64)]
                    if any(waves) and not all(waves):
                        add('same_and_mixed_waves', name)
    for c in DS_CASES:
        add(downscale_route(c.scale, c.w, c.C), c.name)
        add('c_%d' % c.C, c.name)
        add('hw_%d' % (c.h * c.w), c.name)
        add('k_%d' % c.k, c.name)
        add('h_%d' % c.h, c.name)
        if downscale_route(c.scale, c.w, c.C) == 'generic':
            add('scale_%d' % c.scale + ('_odd_w' if c.scale == 16 else '_loop' if c.scale * c.scale > 256 else ''), c.name)
        else:
            if c.w * 8 < 256:
                add('part_workgroup', c.name)
            if c.w * 8 > 256 and (c.w * 8) % 256:
                add('second_x_block', c.name)
        if c.min_ratio <= 0.5:
            add('ties_visible', c.name)
    for c in REFINE_CASES:
        h, w, H, W = c.shape
        add('c_%d' % c.C, c.name)
        if c.sup:
            add('sup_views_%d' % c.views, c.name)
            sup = sup_map(c.b, H, W, _rng('x')).reshape(c.b, -1)
            n = H * W
            waves = [len(set(sup[0, i:i + 64])) == 1 for i in range(0, n - n % 64, 64)]
            if any(waves) and not all(waves):
                add('sup_whole_and_mixed_waves', c.name)
            if n % 256:
                add('sup_ragged', c.name)
        else:
            add('views_%d' % c.views, c.name)
        if c.views & 1:
            add('k_%d' % c.k, c.name)
            add('slices_%d' % refine_slices(c.C), c.name)
            sh = slice_shapes(c.C, c.k)
            if any(a == 0 and t == 0 for a, t in sh):
                add('empty_slices', c.name)
            if all(a == 0 for a, t in sh) and any(t for a, t in sh):
                add('tail_only', c.name)
            if any(a and t for a, t in sh):
                add('tail_4_plus_1', c.name)
            if refine_lds(c.C, c.k) > LDS_ATTR:
                add('lds_attr', c.name)
            if (h * w) % REFINE_PX:
                add('ok_guard', c.name)
        gx, gy, _ = refine_grid(H, W, c.b)
        if W % REFINE_COLS and gx > 1:
            add('W_ragged_%d_blocks' % gx, c.name)
        if W == 257:
            add('W_257', c.name)
        if H % REFINE_ROWS:
            add('H_not_8', c.name)
        if h == 1:
            add('h_1', c.name)
        if w == 1:
            add('w_1', c.name)
        if H == h and W == w:
            add('H_eq_h', c.name)
        if (h > 1 and (H - 1) % (h - 1)) or (w > 1 and (W - 1) % (w - 1)):
            add('non_integer_scale', c.name)
        # a workgroup's 8 rows cross a low-res row pair boundary (the cached horizontal lerp is refreshed mid-walk)
        i0 = lerp_ac(h, H)[0].numpy()
        if any(len(set(i0[y:y + REFINE_ROWS])) > 1 for y in range(0, H, REFINE_ROWS)):
            add('row_pair_changes', c.name)
    return out


REQUIRED = [
    # pseudo_select
    'scalar', 'vec', 'vec_tail_chunk', 'scalar_two_chunks', 'c_1', 'c_5', 'c_6', 'c_7', 'c_16', 'threshold_equal',
    'threshold_next', 'two_pass', 'low_dominates', 'classmax_ready', 'flag_above_scalar', 'flag_below_scalar',
    'flag_nan_scalar', 'flag_above_vec', 'flag_below_vec', 'flag_nan_vec',
    # lrh, fused
    'hw_1', 'one_wave', 'run_across_waves', 'run_cut_by_ignore', 'run_cut_by_bad_region', 'alternating',
    'run_ends_at_invalid_lane', 'global_hist', 'ratio_both_sides', 'all_ignored_region', 'region_0', 'ignore_255',
    'percent_0', 'percent_1', 'flag_bit_1', 'flag_bit_2', 'one_pixel_last_chunk', 'three_chunks', 'grid_1', 'one_lane',
    'four_pixel_last_chunk', 'same_and_mixed_waves', 'max_regions_65535',
    # downscale + prototypes
    'generic', 'fast', 'wide', 'scale_2', 'scale_3', 'scale_8', 'scale_16_odd_w', 'scale_32_loop', 'part_workgroup',
    'second_x_block', 'ties_visible', 'c_8', 'c_14', 'c_15', 'hw_1', 'hw_15', 'hw_300', 'k_1', 'k_4', 'k_260', 'h_1', 'h_3',
    # label_refine
    'views_1', 'views_2', 'views_3', 'sup_views_0', 'sup_views_1', 'sup_views_2', 'sup_views_3', 'slices_8', 'slices_16',
    'empty_slices', 'tail_only', 'tail_4_plus_1', 'lds_attr', 'ok_guard', 'k_36', 'k_68', 'k_2048', 'k_4096',
    'W_ragged_2_blocks', 'W_ragged_3_blocks', 'W_257', 'H_not_8', 'h_1', 'w_1', 'H_eq_h', 'non_integer_scale',
    'row_pair_changes', 'sup_whole_and_mixed_waves', 'sup_ragged',
]
