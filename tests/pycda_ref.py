"""The PyCDA region pyramid term (rgda_upsample_pycda, include/rgda_hip.h) restated in float64 torch, and the inputs the
tests share.  The reference has no such code: the contract is the header's, and this file states it a second time, from
the header and not from the kernels -- integer targets, `F.interpolate(..., align_corners=True)`, the gradient by autograd.
"""
import torch
import torch.nn.functional as F

FIX = 2 ** 24
EPS = 1e-7


def region_sum(x, s):
    """(b, c, H, W) -> (b, c, ceil(H/s), ceil(W/s)): sums over the squares of side s anchored at (0, 0), border squares
    clipped; s = 0: the whole image."""
    b, c, H, W = x.shape
    if s == 0:
        return x.sum((2, 3), keepdim=True)
    ry, rx = -(-H // s), -(-W // s)
    x = F.pad(x, (0, rx * s - W, 0, ry * s - H))
    return x.reshape(b, c, ry, s, rx, s).sum((3, 5))


def clamp_soft(soft):
    """The out-of-contract rule: NaN counts as 0, everything else is clamped into [0, 1]."""
    return torch.nan_to_num(soft, nan=0.0, posinf=1.0, neginf=0.0).clamp(0.0, 1.0)


def targets(soft, sizes, thresh=0.5):
    """Per level (T float64 (b, c, ry, rx), active bool (b, c, ry, rx), area int64 (1, 1, ry, rx), n_l int): exact
    integers up to the final division."""
    b, c, H, W = soft.shape
    fix = torch.round(clamp_soft(soft).double() * FIX).to(torch.int64)
    thr = int(round(float(thresh) * FIX))
    ones = torch.ones(1, 1, H, W, dtype=torch.int64)
    out = []
    for s in sizes:
        tfix, area = region_sum(fix, s), region_sum(ones, s)
        active = tfix > thr * area
        out.append((tfix.double() / (area.double() * FIX), active, area, int(active.any(1).sum())))
    return out


def predictions(p, size):
    return torch.softmax(F.interpolate(p, size=tuple(size), mode='bilinear', align_corners=True), dim=1)


def loss(preds, soft, sizes, thresh=0.5, level_weight=None):
    """preds: a list of one or two logit tensors (float64 for the reference values) -> (total, levels [L], n_active [L]);
    total and levels are differentiable in the logits."""
    tg = targets(soft, sizes, thresh)
    lw = [1.0 / len(sizes)] * len(sizes) if level_weight is None else [float(v) for v in level_weight]
    levels = []
    for s, (T, active, area, n) in zip(sizes, tg):
        per_head = []
        for p in preds:
            Q = region_sum(predictions(p, soft.shape[-2:]), s) / area.to(p.dtype)
            term = torch.where(active, -T.to(p.dtype) * torch.log(Q + EPS), torch.zeros_like(Q))
            per_head.append(term.sum() / max(n, 1))
        levels.append(sum(per_head) / len(per_head))
    total = sum(w * l for w, l in zip(lw, levels))
    return total, torch.stack(levels), [n for *_, n in tg]


def loss_and_grads(preds, soft, sizes, thresh=0.5, level_weight=None, weight=1.0):
    """float64 reference: (loss [1 + L] = total then levels, n_active, [d(weight * total) / d(logits) per prediction])."""
    ps = [p.detach().double().requires_grad_(True) for p in preds]
    total, levels, n = loss(ps, soft, sizes, thresh, level_weight)
    if total.requires_grad:
        (weight * total).backward()
    grads = [torch.zeros_like(p) if p.grad is None else p.grad for p in ps]
    return torch.cat([total.detach().reshape(1), levels.detach()]), n, grads


def closed_form_grad(z, soft, sizes, thresh=0.5, level_weight=None):
    """d total / d z for ONE prediction already at the label resolution, the way the kernels compute it:
    a_l = -w_l T / (max(n_l, 1) |r| (Q + eps)) where active, pushed down to the pixels as A = sum_l a_l, and
    dz_k = q_k (A_k - sum_c A_c q_c)."""
    b, c, H, W = z.shape
    q = torch.softmax(z, dim=1)
    lw = [1.0 / len(sizes)] * len(sizes) if level_weight is None else [float(v) for v in level_weight]
    A = torch.zeros_like(q)
    for w, s, (T, active, area, n) in zip(lw, sizes, targets(soft, sizes, thresh)):
        Q = region_sum(q, s) / area.to(q.dtype)
        a = torch.where(active, -w * T.to(q.dtype) / (max(n, 1) * area.to(q.dtype) * (Q + EPS)), torch.zeros_like(Q))
        if s == 0:
            A = A + a.expand(b, c, H, W)
        else:
            A = A + a.repeat_interleave(s, 2).repeat_interleave(s, 3)[:, :, :H, :W]
    return q * (A - (A * q).sum(1, keepdim=True))


# ------------------------------------------------------------------------------------------------- inputs
def make_soft(b, c, H, W, seed):
    """Smooth class regions with confident interiors and mixed borders: softmax(bilinear upsample of N(0, 6^2) logits on
    a 3 x 4 grid + 0.5 N(0, 1) per pixel), f32."""
    g = torch.Generator().manual_seed(seed)
    coarse = torch.randn(b, c, 3, 4, generator=g, dtype=torch.float64) * 6.0
    z = F.interpolate(coarse, size=(H, W), mode='bilinear', align_corners=True)
    z = z + 0.5 * torch.randn(b, c, H, W, generator=g, dtype=torch.float64)
    return torch.softmax(z, dim=1).float()


def make_logits(b, c, h, w, seed, heads=2):
    g = torch.Generator().manual_seed(seed + 7919)
    return [3.0 * torch.randn(b, c, h, w, generator=g) for _ in range(heads)]


# (low-resolution logits, label size, sizes): three shapes of the pyramid's own and the upsample pipeline's edge shapes
# (tests/test_iast_gpu.py: SHAPES) -- odd sizes with clipped border squares, h == H, an integer ratio
CASE_SHAPES = [((5, 7), (33, 45), (4, 16, 0)), ((4, 6), (64, 96), (4, 8, 16, 32)), ((3, 5), (48, 80), (2, 64, 0)),
               ((5, 7), (33, 45), (2, 8, 0)), ((9, 11), (9, 11), (2, 8, 0)), ((4, 4), (64, 64), (2, 8, 0))]
CLASSES = (6, 7, 16)
BATCH = 2
_CASES = {}


def case_seed(C, k):
    return 1000 * C + 10 * k


def case(C, k):
    """The shared inputs of case (C, shape k), made once: soft f32, two heads of logits f32, the sizes, and a cache for
    the float64 references."""
    if (C, k) not in _CASES:
        lo, hi, sizes = CASE_SHAPES[k]
        seed = case_seed(C, k)
        _CASES[(C, k)] = dict(soft=make_soft(BATCH, C, *hi, seed), p=make_logits(BATCH, C, *lo, seed), sizes=sizes, lo=lo, hi=hi,
                              refs={})
    return _CASES[(C, k)]


def case_reference(d, heads, weight=1.0):
    key = (heads, weight)
    if key not in d['refs']:
        d['refs'][key] = loss_and_grads(d['p'][:heads], d['soft'], d['sizes'], weight=weight)
    return d['refs'][key]
