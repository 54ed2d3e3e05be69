"""The pseudo-label analysis contract (include/rgda_hip.h: rgda_pseudo_analysis, rgda_pseudo_analysis_fold) restated in
numpy, and the seeded inputs its tests and tests/golden/make_analysis_goldens.py share (the goldens hold outputs only).

Per pixel: the pseudo_selection decision (oracle/labels.py), the entropy sum_c -p_c log p_c in fp64 in class order rounded
once to f32, the difficulty 1 - p[gt] in f32 (1 where gt is ignored); the pixel counts in every bin i with
lo[i] <= entropy < hi[i] (f32 edges) and in row R where the entropy is NaN.  Everything that leaves is an integer, except
the fold's per-image quotients (fp64)."""
import math

import numpy as np

from oracle import labels as olab

KINDS = ('softmax', 'confident', 'zeros', 'uniform', 'gt_ignore', 'gt_argmax')
CLASSES = (6, 7, 16)
R = 100
TOP, LOW, IGNORE = 0.8, 0.6, -1
EDGE_MARGIN = 1e-5      # 4 x the bound on |f32 reference entropy - fp64 entropy| at 16 classes (about 2.5e-6)


def shapes():
    """(b, C, H, W) of every case: 33 x 45 has an odd H * W; 96 x 100 takes several workgroups per image."""
    return [(2, C, 33, 45) for C in CLASSES] + [(3, 6, 96, 100)]


def edges(C, R=R):
    """-> (x, lo f32 [R], hi f32 [R]) as the reference compares: f32(1.0 * i * step), f32(1.0 * i * step + step)."""
    step = math.log(C) / R
    return ([i * step for i in range(R)], np.array([1.0 * i * step for i in range(R)], np.float32),
            np.array([1.0 * i * step + step for i in range(R)], np.float32))


def entropy64(soft):
    """fp64 entropy in class order, (b, H, W); NaN where a probability is exactly 0."""
    p = soft.astype(np.float64)
    e = np.zeros(p.shape[:1] + p.shape[2:])
    with np.errstate(divide='ignore', invalid='ignore'):
        for k in range(p.shape[1]):
            e = e + (-p[:, k]) * np.log(p[:, k])
    return e


def difficulty(soft, gt, ignore=IGNORE):
    """f32 1 - p[gt], 1 where gt is ignored."""
    pg = np.take_along_axis(soft, np.clip(gt, 0, soft.shape[1] - 1)[:, None], 1)[:, 0]
    return np.where(gt == ignore, np.float32(1), np.float32(1) - pg).astype(np.float32)


def _softmax(rng, n, C):
    scale = rng.choice(np.array([0.5, 2.0, 5.0, 10.0]), size=(n, 1))
    z = rng.standard_normal((n, C)) * scale
    z -= z.max(1, keepdims=True)
    p = np.exp(z)
    return (p / p.sum(1, keepdims=True)).astype(np.float32)


def _confident(rng, n, C):
    eps = rng.uniform(1e-4, 0.05, size=(n, 1))
    p = np.repeat(eps / (C - 1), C, 1)
    p[np.arange(n), rng.integers(0, C, n)] = 1 - eps[:, 0]
    return p.astype(np.float32)


def _near_edge(p, C):
    _, lo, hi = edges(C)
    e = entropy64(p.T[None, :, :, None])[0, :, 0]
    ed = np.unique(np.concatenate([lo, hi]).astype(np.float64))
    at = np.clip(np.searchsorted(ed, e), 1, ed.size - 1)        # the nearest edge is one of the two around e
    with np.errstate(invalid='ignore'):
        return np.isfinite(e) & (np.minimum(np.abs(e - ed[at - 1]), np.abs(e - ed[at])) <= EDGE_MARGIN)


def inputs(kind, b, C, H, W, seed):
    """-> (soft f32 (b, C, H, W) in [0, 1], gt int64 (b, H, W) in -1 .. C - 1), seeded.  No finite entropy lies within
    EDGE_MARGIN of a bin edge (such pixels are redrawn), except in `uniform`, which is made of one such value."""
    assert kind in KINDS
    rng = np.random.default_rng([seed, KINDS.index(kind), b, C, H, W])
    n = b * H * W
    if kind == 'uniform':
        p = np.full((n, C), np.float32(1) / np.float32(C), np.float32)
    else:
        draw = _confident if kind == 'confident' else _softmax
        p = draw(rng, n, C)
        if kind == 'zeros':
            hot = rng.random(n) < 0.3                 # exact one-hots
            p[hot] = np.eye(C, dtype=np.float32)[rng.integers(0, C, int(hot.sum()))]
            two = ~hot & (rng.random(n) < 0.3)        # two classes share the mass, the others are exactly 0
            p[two] = 0
            a = rng.integers(0, C, int(two.sum()))
            p[np.flatnonzero(two), a] = np.float32(0.75)
            p[np.flatnonzero(two), (a + 1 + rng.integers(0, C - 1, a.size)) % C] = np.float32(0.25)
        else:
            assert (p > 0).all()
        for _ in range(50):
            bad = _near_edge(p, C)
            if not bad.any():
                break
            p[bad] = draw(rng, int(bad.sum()), C)
        assert not _near_edge(p, C).any()
    soft = np.ascontiguousarray(p.reshape(b, H, W, C).transpose(0, 3, 1, 2))
    arg = soft.argmax(1)
    if kind == 'gt_ignore':
        gt = np.full((b, H, W), -1, np.int64)
    elif kind == 'gt_argmax':
        gt = arg.astype(np.int64)
    else:       # half right, a tenth ignored
        gt = np.where(rng.random((b, H, W)) < 0.5, arg, rng.integers(0, C, (b, H, W))).astype(np.int64)
        gt[rng.random((b, H, W)) < 0.1] = -1
    return soft, gt


def analyse(soft, gt, R=R, top=TOP, low=LOW, ignore=IGNORE):
    """-> dict of the per-image tables: used, hit int64 (b, R + 1, C), inbin, diff24 int64 (b, R + 1), flag.  Pixels that
    raise a flag bit are skipped."""
    b, C, H, W = soft.shape
    _, lo, hi = edges(C, R)
    ok_p = np.all((soft >= 0) & (soft <= 1), 1)             # NaN fails both
    ok_g = (gt == ignore) | ((gt >= 0) & (gt < C))
    flag = (0 if ok_p.all() else 1) | (0 if ok_g.all() else 2)
    if flag & 1:        # outside the contract: the flag is what the call promises, the tables are not pinned
        pseudo = np.full((b, H, W), -1, np.int64)
    else:
        pseudo = olab.pseudo_selection(soft, top, low, -1)
    with np.errstate(invalid='ignore'):
        ef = entropy64(soft).astype(np.float32)
    d24 = (difficulty(soft, gt, ignore).astype(np.float64) * 2.0 ** 24)
    assert (d24[ok_p & ok_g] == np.floor(d24[ok_p & ok_g])).all()
    d24 = np.where(ok_p & ok_g, d24, 0).astype(np.int64)
    out = dict(used=np.zeros((b, R + 1, C), np.int64), hit=np.zeros((b, R + 1, C), np.int64),
               inbin=np.zeros((b, R + 1), np.int64), diff24=np.zeros((b, R + 1), np.int64), flag=flag)
    for i in range(R + 1):
        with np.errstate(invalid='ignore'):
            m = (np.isnan(ef) if i == R else (ef >= lo[i]) & (ef < hi[i])) & ok_p & ok_g
        for img in range(b):
            mi = m[img]
            out['inbin'][img, i] = mi.sum()
            out['diff24'][img, i] = d24[img][mi].sum()
            ps, g = pseudo[img][mi], gt[img][mi]
            out['used'][img, i] = np.bincount(ps[ps >= 0], minlength=C)
            out['hit'][img, i] = np.bincount(ps[(ps >= 0) & (ps == g)], minlength=C)
    return out


def new_state(C, R=R):
    return dict(used=np.zeros((R + 1, C), np.int64), hit=np.zeros((R + 1, C), np.int64), inbin=np.zeros(R + 1, np.int64),
                diff24=np.zeros(R + 1, np.int64), acc_sum=np.zeros(R), diffi_sum=np.zeros(R), acc_cnt=np.zeros(R, np.int32),
                diffi_cnt=np.zeros(R, np.int32), images=0, flag=0)


def fold(state, t):
    """Adds a batch's tables to the running state, image after image (rgda_pseudo_analysis_fold)."""
    R = t['inbin'].shape[1] - 1
    for img in range(t['inbin'].shape[0]):
        used = t['used'][img, :R].sum(1) + t['used'][img, R].sum()
        hit = t['hit'][img, :R].sum(1) + t['hit'][img, R].sum()
        d24 = t['diff24'][img, :R] + t['diff24'][img, R]
        state['acc_sum'] += hit.astype(np.float64) / (used.astype(np.float64) + 1e-7)
        state['acc_cnt'] += used != 0
        state['diffi_sum'] += (d24.astype(np.float64) * 2.0 ** -24) / (t['inbin'][img, :R].astype(np.float64) + 1e-7)
        state['diffi_cnt'] += d24 != 0
        for k in ('used', 'hit', 'inbin', 'diff24'):
            state[k] += t[k][img]
    state['images'] += t['inbin'].shape[0]
    state['flag'] |= t['flag']
    return state


def summary(state, C):
    """What PseudoLabelAnalysis.summary() returns."""
    R = state['inbin'].shape[0] - 1
    used = state['used'][:R] + state['used'][R]
    true = state['hit'][:R] + state['hit'][R]
    return dict(x=edges(C, R)[0], acc_list=list(state['acc_sum'] / (state['acc_cnt'] + 1e-7)),
                diffi_list=list(state['diffi_sum'] / (state['diffi_cnt'] + 1e-7)), cnt_true_list=true.sum(1),
                cnt_used_list=used.sum(1), used=used, true=true, in_bin=state['inbin'][:R].copy(),
                nan_pixels=int(state['inbin'][R]), images=state['images'])


def run(soft, gt, per_image=False):
    """The summary of one batch; per_image: folded one image at a time, as the reference's loop sees them."""
    C = soft.shape[1]
    st = new_state(C)
    if per_image:
        for i in range(soft.shape[0]):
            fold(st, analyse(soft[i:i + 1], gt[i:i + 1]))
    else:
        fold(st, analyse(soft, gt))
    return summary(st, C)
