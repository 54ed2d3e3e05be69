"""The upsample-loss kernels of regda_amd/csrc/loss_kernels.hip (rgda_upsample_ce; rgda_upsample_loss: OHEM, focal, GHM,
UPS, UVEM): a Python restatement of the host-side decisions, a simulation of the OHEM radix select on fp32 keys, a float64
reference of the whole operation, and a table of small cases that each name the path they are there to reach.

The restatement mirrors loss_kernels.hip; tests/test_loss_cases_cpu.py parses the constants it copies out of the source,
so a change there that is not made here fails on a machine without a GPU.

Reference (`ref64`): F.interpolate(align_corners=True) in double from the fp32 inputs, each loss in double, gradients by
autograd.  Decisions (the OHEM keep set, the GHM bin and bucket, the UPS gate, the UVEM branch) are taken in double; of
equal OHEM losses the lowest pixel index is kept.  Pixels whose decision value lies within eps of a boundary are set to
ignore on both sides before either side runs (`settle`), eps = max(1e-5, 3 x the fp32-vs-fp64 deviation of the decision
value on the case); exact ties are never excused.  `ref32` is the fp32 restatement tests/loss_ref.py on the same inputs:
tests/golden/derive_loss_tolerances.py derives every bound from its deviation from `ref64`.

Inputs are built on the CPU from fixed seeds; nothing here needs a GPU or the library.
"""
import contextlib
import functools
import zlib
from collections import namedtuple

import numpy as np
import torch
import torch.nn.functional as F

import loss_ref

# ---------------------------------------------------------------- the restatement (loss_kernels.hip, common.h)
MIN_CLASSES, MAX_CLASSES = 6, 16     # RGDA_MIN_CLASSES / RGDA_MAX_CLASSES
ROW_LDS_MAX = 150 * 1024             # RGDA_LOSS_ROW_LDS_MAX: above, the entry point refuses (RGDA_ERR_UNSUPPORTED)
LDS_ATTR = 64 * 1024                 # lds_attr: above, hipFuncAttributeMaxDynamicSharedMemorySize is set before the launch
ROW_THREADS = 256                    # the row loop `for (X = threadIdx.x; X < W; X += 256)`
SEL_PASSES, SEL_BINS = 6, 2048
SEL_SHIFT = (53, 42, 32, 21, 10, 0)  # kSelShift / kSelWidth: the loss bits in 11 + 11 + 10, the inverted index likewise
SEL_WIDTH = (11, 11, 10, 11, 11, 10)
SEL_CHUNK, SEL_MAX_WG = 256 * 8, 512  # the select grid: min(cdiv(n, 256 * 8), 512) workgroups per head
CNT_REPL = 64                        # copies of the counters; row workgroup i adds to copy i % CNT_REPL
GHM_BINS = 30
GHM_EDGES = loss_ref.GHM_EDGES.double()      # the f32 edges, as the kernel's s_edges
OHEM_THRESH = loss_ref.OHEM_THRESH


def cdiv(a, b):
    return -(-a // b)


def grad_lds(c, w, W, want=True):
    """dynamic LDS of the grad pass: rows[2][c][2][w] | G[2][c][W] (with gradients) | lxi[W] | lxl[W]"""
    return (2 * c * 2 * w + (2 * c * W if want else 0) + 2 * W) * 4


def row_route(c, w, W, want=True):
    lds = grad_lds(c, w, W, want)
    return 'refuse' if lds > ROW_LDS_MAX else 'attr' if lds > LDS_ATTR else 'default'


def select_grid(n):
    return min(cdiv(n, SEL_CHUNK), SEL_MAX_WG)


def row_iters(W):
    return cdiv(W, ROW_THREADS)


def lerp_ac(n_in, n_out):
    """common.h lerp_ac for every destination index: (i0, i1, l1) with the fp32 product scale * dst."""
    scale = np.float32(n_in - 1) / np.float32(n_out - 1) if n_out > 1 else np.float32(0)
    src = (scale * np.arange(n_out, dtype=np.float32)).astype(np.float32)
    i0 = src.astype(np.int64)
    i1 = i0 + (i0 < n_in - 1)
    return i0, i1, (src - i0.astype(np.float32)).astype(np.float32)


def covered(n_in, n_out):
    """bool[n_in]: the low-res positions some output position reads (downsampling leaves some without a contributor)."""
    i0, i1, l1 = lerp_ac(n_in, n_out)
    c = np.zeros(n_in, bool)
    c[i0[l1 < 1]] = True
    c[i1[l1 > 0]] = True
    return c


def footprint(n_in, n_out):
    """the largest number of output positions one low-res position takes a weight from"""
    i0, i1, l1 = lerp_ac(n_in, n_out)
    n = np.bincount(i0, minlength=n_in) + np.bincount(i1[i1 != i0], minlength=n_in)
    return int(n.max())


# ---------------------------------------------------------------- the radix select, simulated on fp32 keys
def select_sim(v, n_min, thresh=OHEM_THRESH):
    """ohem_select_kernel after loss_finalize_kernel on one head's fp32 losses v (ignored pixels 0) ->
    dict(branch 'thresh' | 'topk', resolved: the pass that wrote the cut (None on the threshold branch), keep: bool[n],
    kept: #(v > thresh), straddle: a group of equal losses lies on both sides of the cut)."""
    v = np.ascontiguousarray(v, np.float32).reshape(-1) + np.float32(0)      # (torch's nll gives -0.0 for a CE of 0)
    n = v.size
    key = (v.view(np.uint32).astype(np.uint64) << np.uint64(32)) | (n - 1 - np.arange(n)).astype(np.uint64)
    kept = int((v > np.float32(thresh)).sum())
    if kept >= n_min:
        cut = np.uint64((int(np.float32(thresh).view(np.uint32)) + 1) << 32)
        return dict(branch='thresh', resolved=None, keep=key >= cut, kept=kept, straddle=False)
    prefix, rem = 0, n_min
    for p in range(SEL_PASSES):
        shift, width = SEL_SHIFT[p], SEL_WIDTH[p]
        top = shift + width
        m = np.ones(n, bool) if top == 64 else (key >> np.uint64(top)) == np.uint64(prefix >> top)
        hist = np.bincount(((key[m] >> np.uint64(shift)) & np.uint64((1 << width) - 1)).astype(np.int64), minlength=1 << width)
        cum = hist[::-1].cumsum()                    # from the top digit down
        j = int(np.searchsorted(cum, rem))           # the first digit whose count crosses rem
        d = (1 << width) - 1 - j
        left = rem - int(cum[j] - hist[d])
        prefix |= d << shift
        if hist[d] == left or p == SEL_PASSES - 1:
            keep = key >= np.uint64(prefix)
            assert int(keep.sum()) == n_min
            vk = v[keep].min()
            return dict(branch='topk', resolved=p, keep=keep, kept=kept, straddle=bool((v >= vk).sum() > n_min))
        rem = left
    raise AssertionError('unreachable')


# ---------------------------------------------------------------- the cases
Geo = namedtuple('Geo', 'name b C h w H W')
GEOS = {g.name: g for g in [
    Geo('one_px', 1, 6, 1, 1, 5, 7),             # h == 1, w == 1, whole-row footprints
    Geo('identity', 2, 6, 8, 8, 8, 8),           # weights 0 / 1; the gradient is per pixel
    Geo('ragged_row', 2, 6, 3, 5, 17, 300),      # X tail (256 + 44), non-integer ratios on both axes, non-square
    Geo('narrow_down', 2, 6, 9, 7, 4, 3),        # downsampling, W < 64, low-res pixels without a contributor
    Geo('odd_ratio', 2, 6, 33, 33, 64, 64),      # ratio 63 / 32, footprint bounds; n = 8192: four select workgroups
    Geo('repl_wrap', 3, 11, 5, 6, 37, 41),       # b * H = 111 > CNT_REPL, odd sizes, 11 classes
    Geo('wide_c7', 1, 7, 2, 64, 3, 1024),        # 72 704 B: the raised-attribute route, four X iterations
    Geo('wide_c16', 1, 16, 4, 32, 9, 512),       # 77 824 B at 16 classes
    Geo('refuse_c16', 1, 16, 2, 64, 3, 1024),    # 155 648 B with gradients: refused; 24 576 B without: served
    Geo('up16', 2, 6, 2, 2, 32, 32),             # the production kind of ratio, small
    # the geometries of the per-kind cases: the keep mask, the bins and the gate are visible per pixel in the gradient
    Geo('id64', 2, 6, 64, 64, 64, 64),           # n = 8192
    Geo('id32', 2, 6, 32, 32, 32, 32),           # n = 2048: a one-workgroup select
]}
TABLE_GEOS = ['one_px', 'identity', 'ragged_row', 'narrow_down', 'odd_ratio', 'repl_wrap', 'wide_c7', 'wide_c16', 'up16']
KINDS = ('ce', 'ohem', 'focal', 'ghm', 'ups', 'uvem')
TAKES_CW = ('ce', 'ohem', 'ups', 'uvem')
DEFAULTS = dict(cw=False, gamma=None, m=0.2, t=0.7, thresh=OHEM_THRESH, momentum=0.99, ignore=-1, heads=2, want_grad=True)

# name, kind, geometry, the builder of the inputs, parameters other than DEFAULTS, the paths the case is there for
Case = namedtuple('Case', 'name kind geo build prm paths')


def _case(name, kind, geo, build='rand', paths=(), **prm):
    return Case(name, kind, geo, build, tuple(sorted(prm.items())), tuple(paths))


def _table():
    out = []
    for geo in TABLE_GEOS:
        for kind in KINDS:
            for cw in ((False, True) if kind in TAKES_CW else (False,)):
                out.append(_case('%s-%s%s' % (geo, kind, '-cw' if cw else ''), kind, geo, cw=cw))
    # the refused row, without gradients
    out += [_case('refuse_c16-%s' % kind, kind, 'refuse_c16', paths=('served_without_grad',), want_grad=False) for kind in KINDS]
    return out


CASES = _table() + [
    # ---- OHEM on identity geometries: the keep mask can be read off the gradient
    _case('id64-ohem-thresh', 'ohem', 'id64', 'rand', ('ohem_thresh', 'select_multi_wg')),
    _case('id64-ohem-topk', 'ohem', 'id64', 'topk', ('ohem_topk', 'select_pass_1', 'select_multi_wg')),
    _case('id64-ohem-tie_cut', 'ohem', 'id64', 'tie_cut', ('tie_straddles', 'select_pass_5')),
    _case('id64-ohem-tie_p0', 'ohem', 'id64', 'tie_p0', ('select_pass_0',)),
    _case('id64-ohem-tie_p1', 'ohem', 'id64', 'tie_p1', ('select_pass_1',)),
    # (two values closer than 2^-22 of their size and further apart than eps: only above ~1, so the threshold is 5)
    _case('id64-ohem-tie_p2', 'ohem', 'id64', 'tie_p2', ('select_pass_2',), thresh=5.0),
    _case('id64-ohem-tie_p4', 'ohem', 'id64', 'tie_p4', ('tie_straddles', 'select_pass_4')),
    _case('id64-ohem-zeros_cut', 'ohem', 'id64', 'zeros_cut', ('zeros_cut', 'tie_straddles', 'select_pass_5')),
    _case('id64-ohem-nmin0', 'ohem', 'id64', 'nmin0', ('n_min_0',)),
    _case('id64-ohem-kept_eq', 'ohem', 'id64', 'kept_eq', ('kept_eq_n_min',)),
    _case('id64-ohem-all_ignored', 'ohem', 'id64', 'all_ignored', ('all_ignored',)),
    _case('id64-ohem-head_split', 'ohem', 'id64', 'head_split', ('heads_on_both_branches',)),
    _case('id32-ohem-one_wg', 'ohem', 'id32', 'topk', ('select_single_wg', 'ohem_topk')),
    _case('id32-ohem-one_wg-cw', 'ohem', 'id32', 'topk', ('select_single_wg',), cw=True),
    _case('id64-ohem-gap', 'ohem', 'id64', 'topk_gap', ('ohem_topk',)),
    _case('ragged_row-ohem-gap', 'ohem', 'ragged_row', 'topk_gap', ('ohem_topk',)),
    _case('ragged_row-ohem-gap-cw', 'ohem', 'ragged_row', 'topk_gap', ('ohem_topk',), cw=True),
    # a tie group whose needed part is exactly the pixels below index 2048 of n = 2^21 + 2048: the first index digit
    # decides, which needs more than 2^21 pixels.  w == 1: a row's pixels share their logits, H == h: a row per tie row
    _case('far-ohem-tie_p3', 'ohem', 'far', 'tie_p3', ('tie_straddles', 'select_pass_3', 'n_above_2_21')),
    # ---- GHM
    _case('id32-ghm-m0', 'ghm', 'id32', 'rand', ('ghm_momentum_0',), momentum=0.0),
    _case('ragged_row-ghm-m0', 'ghm', 'ragged_row', 'rand', ('ghm_momentum_0',), momentum=0.0),
    _case('id32-ghm-sat', 'ghm', 'id32', 'sat', ('ghm_saturated', 'ghm_momentum_0'), momentum=0.0),
    _case('id32-ghm-sat99', 'ghm', 'id32', 'sat', ('ghm_saturated', 'ghm_momentum_099')),
    _case('id32-ghm-ig255', 'ghm', 'id32', 'rand', ('ghm_ignore_255',), ignore=255, momentum=0.0),
    _case('ragged_row-ghm-ig255', 'ghm', 'ragged_row', 'rand', ('ghm_ignore_255',), ignore=255),
    _case('id32-ghm-h1', 'ghm', 'id32', 'rand', ('ghm_heads_1',), heads=1, momentum=0.0),
    _case('ragged_row-ghm-h1', 'ghm', 'ragged_row', 'rand', ('ghm_heads_1',), heads=1),
    # ---- UPS / UVEM
    _case('id32-uvem-m0', 'uvem', 'id32', 'rand', ('uvem_m_0',), m=0.0, t=0.7, gamma=4.0),
    _case('ragged_row-uvem-m0-cw', 'uvem', 'ragged_row', 'rand', ('uvem_m_0',), m=0.0, t=0.7, gamma=4.0, cw=True),
    _case('id32-uvem-m_eq_t', 'uvem', 'id32', 'rand', ('uvem_m_eq_t',), m=0.5, t=0.5, gamma=2.0),
    _case('ragged_row-uvem-m_eq_t', 'uvem', 'ragged_row', 'rand', ('uvem_m_eq_t',), m=0.5, t=0.5, gamma=2.0),
    _case('ragged_row-ups-t05', 'ups', 'ragged_row', 'rand', (), t=0.5),
    _case('ragged_row-ups-zeros', 'ups', 'ragged_row', 'soft_zeros', ('soft_zeros',)),
    _case('ragged_row-uvem-zeros', 'uvem', 'ragged_row', 'soft_zeros', ('soft_zeros',)),
    _case('id32-uvem-zeros-m0', 'uvem', 'id32', 'soft_zeros', ('soft_zeros', 'uvem_m_0'), m=0.0),
    _case('id32-ups-nogate', 'ups', 'id32', 'nogate', ('gate_empty',)),
    _case('id32-uvem-nogate', 'uvem', 'id32', 'nogate', ('gate_empty',)),
    _case('ragged_row-uvem-nogate-cw', 'uvem', 'ragged_row', 'nogate', ('gate_empty',), cw=True),
] + [
    # ---- focal: every gamma with a valid block whose CE is exactly 0
    _case('%s-focal-g%s' % (geo, str(g).replace('.', '_')), 'focal', geo, 'sat',
          ('focal_saturated', 'focal_gamma_2' if g == 2 else 'focal_gamma_0' if g == 0 else 'focal_powf'), gamma=float(g))
    for geo in ('id32', 'up16') for g in (2, 1, 3.5, 0)
]
GEOS['far'] = Geo('far', 1, 6, 2050, 1, 2050, 1024)
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)


def params(case):
    p = dict(DEFAULTS)
    p['gamma'] = 2.0 if case.kind == 'focal' else 4.0
    p.update(dict(case.prm))
    return p


def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def _up32(p, size):
    return loss_ref.up(p, size)


def _build(case, attempt):
    """the raw inputs of a case (before `settle`): dict of CPU tensors and parameters"""
    geo, prm = GEOS[case.geo], params(case)
    b, C, h, w, H, W = geo[1:]
    g = _gen('loss', case.name, attempt)
    ig = prm['ignore']
    n = b * H * W
    p1, p2 = torch.randn(b, C, h, w, generator=g) * 2, torch.randn(b, C, h, w, generator=g) * 2
    lab = torch.randint(0, C, (b, H, W), generator=g)
    ign = torch.rand(b, H, W, generator=g) < 0.1
    soft = torch.softmax(torch.randn(b, C, H, W, generator=g) * 3, 1) if case.kind in ('ups', 'uvem') else None
    x = dict(kind=case.kind, name=case.name, geo=geo, tie=None, **prm)
    bd = case.build
    ident = (h, w) == (H, W)
    if bd in ('topk', 'head_split'):
        # head 1 (and head 2 of 'topk') predicts the label except at ~8 % relabelled pixels: fewer than n_min above the
        # threshold, distinct values at the cut; head 2 of 'head_split' is unrelated to the label: the threshold branch
        p1 = p1 * 6
        lab = _up32(p1, (H, W)).argmax(1)
        flip = torch.rand(b, H, W, generator=g) < 0.04
        lab = torch.where(flip, (lab + 1 + torch.randint(0, C - 1, (b, H, W), generator=g)) % C, lab)
        if bd == 'topk':
            p2 = p1 + torch.randn(b, C, h, w, generator=g) * 0.3
    elif bd == 'topk_gap':
        # as tests/test_losses_gpu.full_size_inputs(confident=True): a gap at the k-th place
        base = torch.randn(b, C, h, w, generator=g) * 24
        p1, p2 = base + torch.randn(b, C, h, w, generator=g) * 0.2, base + torch.randn(b, C, h, w, generator=g) * 0.2
        lab = _up32(base, (H, W)).argmax(1)
        v = torch.stack([loss_ref._ce(_up32(p, (H, W)), lab, -1) for p in (p1, p2)])
        low, high = v.amax(0) < 0.01, v.amin(0) > 0.3
        keep = (low | high) & (torch.rand(n, generator=g) >= 0.15)
        n_min = int(keep.sum()) // 5
        cand = torch.nonzero(low & keep)[:, 0]
        n_flip = n_min - int((high & keep).sum())
        assert 0 < n_flip <= cand.numel()
        fl = cand[torch.randperm(cand.numel(), generator=g)[:n_flip]]
        lab = lab.reshape(-1).clone()
        lab[fl] = (lab[fl] + 1) % C
        ign = ~keep.reshape(b, H, W)
        lab = lab.reshape(b, H, W)
    elif bd in ('tie_cut', 'tie_p0', 'tie_p1', 'tie_p2', 'tie_p4', 'zeros_cut', 'kept_eq', 'nmin0'):
        assert ident
        # every pixel confident (CE exactly 0) but: `big` pixels with a wrong label (CE ~ 50 +- noise, distinct), a tie
        # group with logits (3, 0, ..) and label 0 (CE 0.2219 < -log 0.7), a second group at 3.01 (CE 0.2203: the
        # same first digit of the key, another second one)
        hot = torch.randint(0, C, (n,), generator=g)
        z = F.one_hot(hot, C).float() * 50.0
        labf = hot.clone()
        perm = torch.randperm(n, generator=g)
        ignf = torch.zeros(n, dtype=torch.bool)
        n_min = n // 5
        n_big, n_tie, n_low, tie_at = dict(tie_cut=(1000, 1000, 0, None), tie_p0=(1000, n_min - 1000, 0, None),
                                           tie_p1=(1000, n_min - 1000, 300, None),
                                           tie_p2=(1000, n_min - 1000, 300, None), tie_p4=(1000, 0, 0, 'blocks'),
                                           zeros_cut=(500, 0, 0, None), kept_eq=(n_min, 0, 0, None), nmin0=(0, 0, 0, None))[bd]
        if bd == 'zeros_cut':
            ignf = torch.rand(n, generator=g) < 0.1
        big = perm[:n_big]
        if bd == 'kept_eq':
            # n_min pixels clearly above the threshold (CE 1.0 .. 1.4), every other one clearly below (CE 0.05)
            z[:] = F.one_hot(hot, C).float() * 4.5
            z[big] = F.one_hot(hot[big], C).float() * (0.5 + 0.5 * torch.rand(n_big, 1, generator=g))
        else:
            labf[big] = (hot[big] + 1) % C
            z[big] += torch.randn(n_big, C, generator=g)
        tie = perm[n_big:n_big + n_tie]
        if tie_at == 'blocks':
            # the n_min - 1000 = 638 tie pixels that are needed all lie below index 1024, 500 more lie above: the second
            # index digit (index / 1024) decides
            first = torch.nonzero(~torch.isin(torch.arange(1024), big))[:, 0][:n_min - n_big]
            later = torch.nonzero(~torch.isin(torch.arange(n), big) & (torch.arange(n) >= 1024))[:, 0]
            later = later[torch.randperm(later.numel(), generator=g)[:500]]
            tie = torch.cat([first, later])
        z[tie] = 0.0
        z[tie, 0] = 3.0
        labf[tie] = 0
        lowg = perm[n_big + n_tie:n_big + n_tie + n_low]
        z[lowg] = 0.0
        z[lowg, 0] = 3.01
        if bd == 'tie_p2':          # CE 3.2223 and 8e-5 below it: the same first two digits of the key
            z[tie, 0], z[tie, 1], z[lowg, 0], z[lowg, 1] = 0.0, 3.0, 0.0, 3.0 - 1e-4
        labf[lowg] = 0
        if bd == 'nmin0':
            # four valid pixels: n_min = 0, the threshold branch; three of them above the threshold
            ignf[:] = True
            four = perm[:4]
            ignf[four] = False
            z[four] = torch.randn(4, C, generator=g)
            labf[four[:3]] = z[four[:3]].argmin(1)
            labf[four[3]] = z[four[3]].argmax()
        p1 = z.reshape(b, H, W, C).permute(0, 3, 1, 2).contiguous()
        p2 = p1.clone()
        lab, ign = labf.reshape(b, H, W), ignf.reshape(b, H, W)
        x['tie'] = tie
    elif bd == 'tie_p3':
        # rows 0 .. 2 (3072 pixels) are the tie group, rows 3 .. 12 hold 1000 wrong labels, the rest is ignored:
        # n_min = (3072 + 1000 + 11168) // 5 = 3048 = 1000 + 2048: rows 0 and 1 are kept, row 2 is not
        z = torch.zeros(h, C)
        z[:, 0] = 50.0
        z[:3, 0] = 3.0
        p1 = z.t().reshape(1, C, h, 1).contiguous()
        p2 = p1.clone()
        labf = torch.zeros(n, dtype=torch.int64)
        ignf = torch.ones(n, dtype=torch.bool)
        ignf[:3072] = False
        wrong = 3072 + torch.randperm(10 * 1024, generator=g)[:1000]
        labf[wrong] = 1 + torch.randint(0, C - 1, (1000,), generator=g)
        ignf[wrong] = False
        conf = 3072 + 10 * 1024 + torch.arange(11168)
        ignf[conf] = False
        p1[0, :, 3:13, 0] += torch.randn(C, 10, generator=g) * 0.5
        p2 = p1.clone()
        lab, ign = labf.reshape(b, H, W), ignf.reshape(b, H, W)
        x['tie'] = torch.arange(3072)
    elif bd == 'all_ignored':
        ign = torch.ones(b, H, W, dtype=torch.bool)
    elif bd == 'sat':
        # a valid block whose CE is exactly 0: the low-res corner block saturated at class 2, labelled 2 at full size
        hh, ww = max(1, h // 4), max(1, w // 4)
        for p in (p1, p2):
            p[:, :, :hh, :ww] = 0.0
            p[:, 2, :hh, :ww] = 50.0
        HH, WW = (hh, ww) if ident else (H // 2, W // 2)
        lab[:, :HH, :WW] = 2
        ign[:, :HH, :WW] = False
    elif bd == 'soft_zeros':
        soft = torch.where(torch.rand(b, C, H, W, generator=g) < 0.05, torch.zeros(()), soft)
    elif bd == 'nogate':
        soft = torch.softmax(torch.randn(b, C, H, W, generator=g) * 0.3, 1)      # u ~ log 6 > t everywhere
    else:
        assert bd == 'rand', bd
    if ig != -1:
        assert ig >= C
    x.update(p1=p1.contiguous(), p2=p2.contiguous(), lab=torch.where(ign, torch.full_like(lab, ig), lab).contiguous(), soft=soft)
    x['cw'] = (0.5 + torch.rand(2, C, generator=g) * 1.5) if prm['cw'] else None
    x['acc0'] = ((0.5 + torch.rand(GHM_BINS, generator=g)) * (n / GHM_BINS)) if case.kind == 'ghm' else None
    return x


def make_x(kind, p1, p2, lab, soft=None, cw=None, acc0=None, **prm):
    """inputs that are not of the table (the goldens), in the form `ref64` / `ref32` take"""
    q = dict(DEFAULTS, gamma=2.0 if kind == 'focal' else 4.0)
    q.update(prm)
    b, C, h, w = p1.shape
    H, W = lab.shape[-2:]
    q.update(kind=kind, name='adhoc', geo=Geo('adhoc', b, C, h, w, H, W), tie=None, p1=p1, p2=p2, lab=lab, soft=soft, cw=cw,
             acc0=acc0)
    return q


# ---------------------------------------------------------------- decisions, boundaries, the excused pixels
def _heads(x):
    return [x['p1']] if x['heads'] == 1 else [x['p1'], x['p2']]


def _pixel_weight(x, hd, dtype):
    if x['cw'] is None:
        return None
    lab = x['lab'].reshape(-1)
    return x['cw'][hd].to(dtype)[torch.where(lab == x['ignore'], torch.zeros_like(lab), lab)]


def _up(p, size):
    return p if p.shape[-2:] == size else F.interpolate(p, size=size, mode='bilinear', align_corners=True)


def decision_values(x, hd, dtype):
    """the per-pixel value head `hd` decides on, at `dtype`: OHEM the (class-weighted) CE, GHM |p_y - 1|, UPS / UVEM u"""
    kind, lab, ig = x['kind'], x['lab'], x['ignore']
    if kind in ('ups', 'uvem'):
        return loss_ref.entropy(x['soft'].to(dtype))
    z = _up(_heads(x)[hd].to(dtype), lab.shape[-2:])
    if kind == 'ohem':
        v = loss_ref._ce(z, lab, ig)
        pw = _pixel_weight(x, hd, dtype)
        return v if pw is None else v * pw
    return loss_ref.ghm_g(z, lab, ig)


def near_boundary(x, v, eps):
    """bool[n]: pixels whose float64 decision value v lies within eps of a boundary of the loss's decisions; equal values
    on the OHEM cut follow the tie rule on both sides and are never excused"""
    kind = x['kind']
    lab = x['lab'].reshape(-1)
    if kind == 'ohem':
        n_min = int((lab != x['ignore']).sum()) // 5
        thr = float(np.float32(x['thresh']))
        if int((v > thr).sum()) < n_min and n_min > 0:
            kth = torch.sort(v, descending=True).values[n_min - 1]
            return ((v - kth).abs() < eps) & (v != kth)
        return (v - thr).abs() < eps
    if kind == 'ghm':
        return ((v[:, None] - GHM_EDGES[None, :GHM_BINS]).abs() < eps).any(1) & (v > 0)
    if kind in ('ups', 'uvem'):
        near = (v - float(np.float32(x['t']))).abs() < eps
        if kind == 'uvem':
            near |= (v - float(np.float32(x['m']))).abs() < eps
        return near
    return torch.zeros_like(lab, dtype=torch.bool)


def settle(x):
    """Set the pixels near a decision boundary to ignore, until none is left.  Adds eps, noise (the measured fp32
    deviation of the decision value) and excused (the number of pixels) to x."""
    x['eps'], x['noise'], x['excused'] = 1e-5, 0.0, 0
    if x['kind'] in ('ce', 'focal'):
        return x
    nh = 1 if x['kind'] in ('ups', 'uvem') else len(_heads(x))
    for hd in range(nh):
        v32, v64 = decision_values(x, hd, torch.float32), decision_values(x, hd, torch.float64)
        ok = torch.isfinite(v32) & torch.isfinite(v64)
        if ok.any():
            x['noise'] = max(x['noise'], float((v32.double() - v64)[ok].abs().max()))
    x['eps'] = max(1e-5, 3 * x['noise'])
    for _ in range(20):
        near = torch.zeros(x['lab'].numel(), dtype=torch.bool)
        for hd in range(nh):
            near |= near_boundary(x, decision_values(x, hd, torch.float64), x['eps'])
        near &= x['lab'].reshape(-1) != x['ignore']
        if not near.any():
            return x
        x['excused'] += int(near.sum())
        x['lab'] = torch.where(near.reshape(x['lab'].shape), torch.full_like(x['lab'], x['ignore']), x['lab'])
    raise AssertionError('pixels near a decision boundary remain: ' + x['name'])


EXCUSED_SHARE = 0.002        # the cap of tests/test_losses_gpu.py
SMALL_CASE = 500             # below: no pixel may be excused


def excused_ok(x):
    n = x['lab'].numel()
    return x['excused'] <= EXCUSED_SHARE * n and (n >= SMALL_CASE or x['excused'] == 0)


@functools.lru_cache(maxsize=None)
def inputs(name):
    """The settled inputs of a case.  The seed is the first of (name, 0), (name, 1), .. for which the share of excused
    pixels keeps its cap (tests/test_loss_cases_cpu.py asserts it)."""
    case = BY_NAME[name]
    for attempt in range(40):
        x = settle(_build(case, attempt))
        if excused_ok(x):
            x['attempt'] = attempt
            return x
    raise AssertionError('no seed keeps the excused share: ' + name)


# ---------------------------------------------------------------- the float64 reference
def _uvem_weight64(u, m, t, gamma):
    left = torch.ones_like(u)
    if m > 0:
        xx = torch.where((u <= m) & (u >= 0), u, left)
        left = torch.clamp((-1 / (m ** 2)) * (xx - m) ** 2 + 1, 0.0, 1.0) ** (1.0 / gamma)
    right = torch.zeros_like(u)
    if m < t:
        xx = torch.where((u > m) & (u <= t), u, right)
        right = torch.clamp((-1 / ((t - m) ** 2)) * (xx - m) ** 2 + 1, 0.0, 1.0) ** (1.0 / gamma)
    return torch.where(u >= t, torch.zeros_like(u), torch.where(u <= m, left, right))


def ref64(x):
    """-> dict(loss, g [per head], full [max |d loss / d upsampled logit|], term [max |per-pixel term of a head's loss|],
    acc [GHM state after the call], hist [the integer histogram of the last head], keep [OHEM keep mask per head],
    branch [OHEM branch per head])"""
    kind, lab, ig = x['kind'], x['lab'], x['ignore']
    size = tuple(lab.shape[-2:])
    labf = lab.reshape(-1)
    valid = labf != ig
    ps = [p.double().clone().requires_grad_(True) for p in _heads(x)]
    out = dict(keep=[], branch=[], hist=None, acc=None, term=0.0)
    acc = x['acc0'].double().clone() if kind == 'ghm' else None
    total, fulls = 0.0, []
    for hd, p in enumerate(ps):
        z = _up(p, size)
        if z is p:
            z = p * 1.0
        z.retain_grad()
        fulls.append(z)
        ce = F.cross_entropy(z, lab, ignore_index=ig, reduction='none').reshape(-1)
        pw = _pixel_weight(x, hd, torch.float64)
        if kind == 'ce':
            pix = (ce if pw is None else ce * pw) / ce.numel()
        elif kind == 'ohem':
            v = ce if pw is None else ce * pw
            vd = v.detach()
            n_min = int(valid.sum()) // 5
            keep = vd > float(np.float32(x['thresh']))
            if int(keep.sum()) < n_min:
                order = torch.sort(vd, descending=True, stable=True).indices[:n_min]
                keep = torch.zeros_like(keep)
                keep[order] = True
                denom, br = n_min, 'topk'
            else:
                denom, br = int(keep.sum()), 'thresh'
            out['keep'].append(keep)
            out['branch'].append(br)
            pix = torch.where(keep, v, torch.zeros_like(v)) / denom if denom else v * float('nan')
        elif kind == 'focal':
            pix = (1 - torch.exp(-ce)) ** x['gamma'] * ce / ce.numel()
        elif kind == 'ghm':
            prob = torch.softmax(z.detach(), 1).permute(0, 2, 3, 1).reshape(-1, z.shape[1])
            py = prob.gather(1, torch.where(valid, labf, torch.zeros_like(labf))[:, None])[:, 0]
            gg = torch.where(valid, (py - 1.0).abs(), torch.full_like(py, -1.0))
            inr = (gg >= 0) & (gg <= 1)
            hist = torch.bincount((gg[inr] * GHM_BINS).floor().long().clamp(max=GHM_BINS - 1), minlength=GHM_BINS)
            ind = (GHM_EDGES[None, :] < gg[:, None]).sum(1)
            mom = float(np.float32(x['momentum']))
            acc = mom * acc + float(np.float32(1.0 - x['momentum'])) * hist.double() if mom > 0 else hist.double()
            wgt = torch.where((ind > 0) & (ind <= GHM_BINS), 1.0 / acc[(ind - 1).clamp(0, GHM_BINS - 1)], torch.zeros_like(gg))
            pix = ce * wgt / (float((labf != -1).sum()) + 1e-7)
            out['hist'] = hist
        else:
            u = loss_ref.entropy(x['soft'].double())
            t, m = float(np.float32(x['t'])), float(np.float32(x['m']))
            gate = u > t
            wgt = torch.ones_like(u) if kind == 'ups' else _uvem_weight64(u, m, t, x['gamma'])
            wgt = torch.where(gate, torch.zeros_like(u), wgt)
            if pw is not None:
                wgt = wgt * pw
            pix = wgt * ce / (float(((u <= t) & valid).sum()) + 1e-7)
        ok = torch.isfinite(pix.detach())
        if ok.any():
            out['term'] = max(out['term'], float(pix.detach()[ok].abs().max()))
        total = total + pix.sum()
    total = total / len(ps)
    out['loss'] = float(total.detach())
    if np.isfinite(out['loss']):
        total.backward()
        out['g'] = [p.grad if p.grad is not None else torch.zeros_like(p) for p in ps]
        out['full'] = max(float(z.grad.abs().max()) if z.grad is not None else 0.0 for z in fulls)
    else:                                # every label ignored: NaN loss, exactly zero gradients
        out['g'] = [torch.zeros_like(p) for p in ps]
        out['full'] = 0.0
    out['acc'] = acc
    return out


# ---------------------------------------------------------------- the fp32 restatement (tests/loss_ref.py), and mutants
def ref32(x):
    """tests/loss_ref.py on the same inputs -> dict(loss, g [per head], acc)"""
    kind, lab, ig = x['kind'], x['lab'], x['ignore']
    size = tuple(lab.shape[-2:])
    st = None
    if kind == 'ghm':
        st = loss_ref.GhmState(x['momentum'])
        st.acc_sum = x['acc0'].clone()
    ps = [p.clone().requires_grad_(True) for p in _heads(x)]
    total = 0.0
    for hd, p in enumerate(ps):
        z = loss_ref.up(p, size)
        pw = _pixel_weight(x, hd, torch.float32)
        if kind == 'ce':
            v = loss_ref._ce(z, lab, ig)
            l = (v if pw is None else v * pw).mean()
        elif kind == 'ohem':
            l = loss_ref.ohem(z, lab, ig, pw, x['thresh'])
        elif kind == 'focal':
            l = loss_ref.focal(z, lab, ig, x['gamma'])
        elif kind == 'ghm':
            l = loss_ref.ghm(z, lab, st, ig)
        else:
            l = loss_ref.ups(z, lab, x['soft'], ig, pw, x['t'], None if kind == 'ups' else (x['m'], x['gamma']))
        total = total + l
    total = total / len(ps)
    out = dict(loss=float(total.detach()), acc=None if st is None else st.acc_sum.clone())
    if np.isfinite(out['loss']):
        total.backward()
        out['g'] = [p.grad if p.grad is not None else torch.zeros_like(p) for p in ps]
    else:
        out['g'] = [torch.zeros_like(p) for p in ps]
    return out


class _ShortFootprint(torch.autograd.Function):
    """the upsample with a backward whose horizontal footprint is one column short: the last output column that
    contributes to a low-res column is left out of its sum"""

    @staticmethod
    def forward(ctx, p, size):
        ctx.shape, ctx.size = p.shape, size
        return F.interpolate(p, size=size, mode='bilinear', align_corners=True)

    @staticmethod
    def backward(ctx, gz):
        (h, w), (H, W) = ctx.shape[-2:], ctx.size
        with torch.enable_grad():
            q = torch.zeros(ctx.shape, requires_grad=True)
            F.interpolate(q, size=ctx.size, mode='bilinear', align_corners=True).backward(gz)
        g = q.grad
        i0, i1, l1 = lerp_ac(w, W)
        yi0, yi1, yl1 = lerp_ac(h, H)
        Ry = torch.zeros(H, h)
        Ry[torch.arange(H), torch.from_numpy(yi0)] += torch.from_numpy(1 - yl1)
        Ry[torch.arange(H), torch.from_numpy(yi1)] += torch.from_numpy(yl1)
        T = torch.einsum('Yy,bcYX->bcyX', Ry, gz)
        for xlo in range(w):
            Xs = [X for X in range(W) if (i0[X] == xlo and l1[X] < 1) or (i1[X] == xlo and l1[X] > 0)]
            if Xs:
                X = Xs[-1]
                wt = (1 - l1[X] if i0[X] == xlo else 0) + (l1[X] if i1[X] == xlo else 0)
                g[..., xlo] -= float(wt) * T[..., X]
        return g, None


def _ohem_mut(tie_high=False, denom_kept=False):
    def ohem(p, label, ig=-1, pixel_weight=None, thresh=loss_ref.OHEM_THRESH):
        lab = label.reshape(-1)
        n_min = int((lab != ig).sum()) // 5
        v = loss_ref._ce(p, label, ig)
        if pixel_weight is not None:
            v = v * pixel_weight
        keep = v > thresh
        if int(keep.sum()) < n_min:
            if tie_high:
                order = v.numel() - 1 - torch.sort(v.detach().flip(0), descending=True, stable=True).indices[:n_min]
            else:
                order = torch.sort(v.detach(), descending=True, stable=True).indices[:n_min]
            return v[order].sum() / int(keep.sum()) if denom_kept else v[order].mean()
        return v[keep].mean()
    return ohem


def _ghm_mut(denom_ig=False, bucket=False):
    def ghm(p, label, state, ig=-1):
        g = loss_ref.ghm_g(p, label, ig)
        inr = (g >= 0) & (g <= 1)
        bins = torch.bincount((g[inr] * 30).floor().long().clamp(max=29), minlength=30).float()
        ind = (loss_ref.GHM_EDGES[None, :] < g[:, None]).sum(1)
        if bucket:
            ind = torch.where(ind == 30, ind - 1, ind)       # the top bucket folded into the one below
        m = state.momentum
        state.acc_sum = m * state.acc_sum + (1 - m) * bins if m > 0 else bins
        w = torch.where((ind > 0) & (ind <= 30), 1.0 / state.acc_sum[ind - 1], torch.zeros_like(g))
        lab = label.reshape(-1)
        return (loss_ref._ce(p, label, ig) * w).sum() / ((lab != (ig if denom_ig else -1)).sum() + 1e-7)
    return ghm


def _uvem_mut(u, m, t, gamma):
    """the right branch taken at m == t: the choice `u <= m ? left : right` made only while m < t"""
    left = torch.ones_like(u)
    if m > 0:
        xx = torch.where((u <= m) & (u >= 0), u, left)
        left = torch.clamp((-1 / (m ** 2)) * (xx - m) ** 2 + 1, 0.0, 1.0) ** (1.0 / gamma)
    right = torch.zeros_like(u)
    if m < t:
        xx = torch.where((u > m) & (u <= t), u, right)
        right = torch.clamp((-1 / ((t - m) ** 2)) * (xx - m) ** 2 + 1, 0.0, 1.0) ** (1.0 / gamma)
    w = torch.where((u <= m) & torch.tensor(m < t), left, right)
    return torch.where(u >= t, torch.zeros_like(u), w)


MUTATIONS = {
    'footprint_short': ('up', lambda p, size: p if p.shape[-2:] == size else _ShortFootprint.apply(p, size)),
    'tie_highest_index': ('ohem', _ohem_mut(tie_high=True)),
    'ghm_denominator_ignore_label': ('ghm', _ghm_mut(denom_ig=True)),
    'ghm_bucket_off_by_one': ('ghm', _ghm_mut(bucket=True)),
    'ohem_denominator_kept': ('ohem', _ohem_mut(denom_kept=True)),
    'uvem_right_at_m_eq_t': ('uvem_weight', _uvem_mut),
}


@contextlib.contextmanager
def mutated(name):
    """tests/loss_ref.py with ONE wrong line, for the mutation checks of tests/test_loss_cases_cpu.py"""
    attr, fn = MUTATIONS[name]
    old = getattr(loss_ref, attr)
    setattr(loss_ref, attr, fn)
    try:
        yield
    finally:
        setattr(loss_ref, attr, old)


# ---------------------------------------------------------------- bounds: 3 x the restatement's deviation + the floor
MARGIN = 3.0
F32_EPS = 2.0 ** -24


def deviations(x, r64=None, r32=None):
    """-> (observed, floor): per output (loss [relative], g1, g2 [absolute, per element], acc [absolute]) the deviation
    of the fp32 restatement from the float64 reference on this case, and the accumulation floor: the number of terms in
    the longest sum x 2^-24 x the largest term."""
    r64 = r64 or ref64(x)
    r32 = r32 or ref32(x)
    geo = x['geo']
    n = x['lab'].numel()
    obs, floor = {}, {}
    if np.isfinite(r64['loss']) and r64['loss'] != 0:
        obs['loss'] = abs(r32['loss'] - r64['loss']) / abs(r64['loss'])
        floor['loss'] = n * F32_EPS * r64['term'] / abs(r64['loss'])
    if x['want_grad']:
        terms = footprint(geo.h, geo.H) * footprint(geo.w, geo.W)
        for k, (a, b) in enumerate(zip(r32['g'], r64['g'])):
            obs['g%d' % (k + 1)] = float((a.double() - b).abs().max())
            floor['g%d' % (k + 1)] = terms * F32_EPS * r64['full']
    if x['kind'] == 'ghm' and x['momentum'] > 0:
        obs['acc'] = float((r32['acc'].double() - r64['acc']).abs().max())
        floor['acc'] = 3 * F32_EPS * float(r64['acc'].abs().max())
    return obs, floor


def bounds(obs, floor):
    return {k: MARGIN * obs[k] + floor[k] for k in obs}


# ---------------------------------------------------------------- which case reaches which path
def paths_reached():
    """{path: [case names]} according to the restatement, the simulation and the built inputs"""
    out = {}

    def add(p, name):
        out.setdefault(p, []).append(name)

    for c in CASES:
        x = inputs(c.name)
        geo = x['geo']
        b, C, h, w, H, W = geo[1:]
        n = b * H * W
        add('kind_' + c.kind, c.name)
        if x['cw'] is not None:
            add('class_weight_' + c.kind, c.name)
        route = row_route(C, w, W, True)
        if route == 'attr' and x['want_grad']:
            add('lds_attr', c.name)
        if route == 'refuse' and not x['want_grad'] and row_route(C, w, W, False) == 'default':
            add('refusal', c.name)
            add('served_without_grad', c.name)
        if W % ROW_THREADS and W > ROW_THREADS:
            add('x_tail', c.name)
        if row_iters(W) == 4:
            add('x_four_iterations', c.name)
        if W < 64:
            add('W_below_64', c.name)
        if w == 1:
            add('w_1', c.name)
        if h == 1:
            add('h_1', c.name)
        if (H, W) == (h, w):
            add('identity', c.name)
        if W < w or H < h:
            add('downsampling', c.name)
            if not (covered(w, W).all() and covered(h, H).all()):
                add('uncovered_low_res', c.name)
        if (h > 1 and (H - 1) % (h - 1)) or (w > 1 and (W - 1) % (w - 1)):
            add('non_integer_ratio', c.name)
        if b * H > CNT_REPL:
            add('replica_wrap', c.name)
        if C not in (6,):
            add('c_%d' % C, c.name)
        lab = x['lab'].reshape(-1)
        valid = lab != x['ignore']
        if c.kind == 'ohem':
            n_min = int(valid.sum()) // 5
            sims = [select_sim(decision_values(x, hd, torch.float32).numpy(), n_min, x['thresh']) for hd in range(2)]
            add('select_multi_wg' if select_grid(n) > 1 else 'select_single_wg', c.name)
            for s in sims:
                add('ohem_' + s['branch'], c.name)
                if s['branch'] == 'topk':
                    add('select_pass_%d' % s['resolved'], c.name)
                    if s['straddle']:
                        add('tie_straddles', c.name)
                        vk = decision_values(x, 0, torch.float32).numpy()[s['keep']].min()
                        if vk == 0 and not valid.all():
                            add('zeros_cut', c.name)
                elif n_min == 0 and valid.any():
                    add('n_min_0', c.name)
                elif s['kept'] == n_min and n_min > 0:
                    add('kept_eq_n_min', c.name)
            if sims[0]['branch'] == 'topk' and sims[1]['branch'] == 'thresh':
                add('heads_on_both_branches', c.name)
            if not valid.any():
                add('all_ignored', c.name)
            if n > (1 << 21):
                add('n_above_2_21', c.name)
        if c.kind == 'ghm':
            add('ghm_momentum_0' if x['momentum'] == 0 else 'ghm_momentum_099', c.name)
            if x['ignore'] == 255 and (lab == 255).any() and not (lab == -1).any():
                add('ghm_ignore_255', c.name)
            if x['heads'] == 1:
                add('ghm_heads_1', c.name)
            g32 = decision_values(x, 0, torch.float32)
            if ((g32 == 0) & valid).any() and x['geo'].name.startswith('id'):
                add('ghm_saturated', c.name)
        if c.kind in ('ups', 'uvem'):
            u = loss_ref.entropy(x['soft'])
            if torch.isnan(u).any():
                add('soft_zeros', c.name)
            if not ((u <= x['t']) & valid).any() and not torch.isnan(u).any():
                add('gate_empty', c.name)
            elif (u > x['t']).any() and (u <= x['t']).any():
                add('gate_both_sides', c.name)
            if c.kind == 'uvem':
                if x['m'] == 0:
                    add('uvem_m_0', c.name)
                elif x['m'] == x['t']:
                    add('uvem_m_eq_t', c.name)
                elif ((u <= x['m']) & valid).any() and ((u > x['m']) & (u < x['t']) & valid).any():
                    add('uvem_left_and_right', c.name)
        if c.kind == 'focal':
            add('focal_gamma_2' if x['gamma'] == 2 else 'focal_gamma_0' if x['gamma'] == 0 else 'focal_powf', c.name)
            ce = loss_ref._ce(loss_ref.up(x['p1'], (H, W)), x['lab'], x['ignore'])
            if ((ce == 0) & valid).any():
                add('focal_saturated', c.name)
    return out


REQUIRED = [
    'select_pass_0', 'select_pass_1', 'select_pass_2', 'select_pass_3', 'select_pass_4', 'select_pass_5',
    'select_multi_wg', 'select_single_wg', 'ohem_thresh', 'ohem_topk', 'tie_straddles', 'zeros_cut', 'n_min_0',
    'kept_eq_n_min', 'all_ignored', 'heads_on_both_branches', 'n_above_2_21',
    'lds_attr', 'refusal', 'served_without_grad', 'x_tail', 'x_four_iterations', 'W_below_64', 'w_1', 'h_1', 'identity',
    'downsampling', 'uncovered_low_res', 'non_integer_ratio', 'replica_wrap', 'c_7', 'c_11', 'c_16',
    'ghm_momentum_0', 'ghm_momentum_099', 'ghm_ignore_255', 'ghm_heads_1', 'ghm_saturated',
    'soft_zeros', 'gate_empty', 'gate_both_sides', 'uvem_m_0', 'uvem_m_eq_t', 'uvem_left_and_right',
    'focal_gamma_2', 'focal_gamma_0', 'focal_powf', 'focal_saturated',
] + ['kind_' + k for k in KINDS] + ['class_weight_' + k for k in TAKES_CW]
