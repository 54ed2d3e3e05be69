"""The region-overlap term (rgda_upsample_overlap, include/rgda_hip.h) restated in torch on the CPU, and the inputs the
tests share.  The reference has no such code: the contract is the header's, and this file states it a second time, from
the header and not from the kernels -- `F.interpolate(..., align_corners=True)`, one-hot masks, the gradient by autograd.
Everything runs in the dtype of the logits it is given: float64 for the reference values, float32 to measure what the
restatement itself loses in single precision (tests/test_overlap_gpu.py, header).
"""
import torch
import torch.nn.functional as F

EPS = 1e-7
IGNORE = -1


def valid_mask(label, C, ignore_label=IGNORE):
    """A pixel counts iff its label is not ignore_label and lies in [0, C)."""
    return (label != ignore_label) & (label >= 0) & (label < C)


def sums(p, label, ignore_label=IGNORE):
    """One head: (TP, FP, FN) [C] in p's dtype over the valid pixels of the batch, Y int64 [C]."""
    C = p.shape[1]
    q = torch.softmax(F.interpolate(p, size=tuple(label.shape[-2:]), mode='bilinear', align_corners=True), dim=1)
    ok = valid_mask(label, C, ignore_label)
    onehot = F.one_hot(torch.where(ok, label, torch.zeros_like(label)), C).permute(0, 3, 1, 2).bool() & ok[:, None]
    other = ~onehot & ok[:, None]
    on, off = onehot.to(q.dtype), other.to(q.dtype)
    return (q * on).sum((0, 2, 3)), (q * off).sum((0, 2, 3)), ((1 - q) * on).sum((0, 2, 3)), onehot.sum((0, 2, 3))


def head_loss(p, label, alpha, beta, gamma, smooth, ignore_label=IGNORE):
    """One head -> (loss_hd, T [C] with 0 for an absent class, Y [C])."""
    TP, FP, FN, Y = sums(p, label, ignore_label)
    N = TP + smooth
    M = alpha * FP + beta * FN + EPS
    present = Y > 0
    n = int(present.sum())
    T = torch.where(present, N / (N + M), torch.zeros_like(N))
    if n == 0:
        return (p * 0).sum(), T, Y
    return torch.where(present, (M / (N + M)) ** gamma, torch.zeros_like(N)).sum() / n, T, Y


def loss(preds, label, alpha=0.5, beta=0.5, gamma=1.0, smooth=0.0, ignore_label=IGNORE):
    """preds: a list of one or two logit tensors -> (loss = the mean over the heads, index [heads, C], present [C])."""
    per = [head_loss(p, label, alpha, beta, gamma, smooth, ignore_label) for p in preds]
    return sum(l for l, _, _ in per) / len(per), torch.stack([t for _, t, _ in per]), per[0][2]


def loss_and_grads(preds, label, alpha=0.5, beta=0.5, gamma=1.0, smooth=0.0, weight=1.0, ignore_label=IGNORE,
                   dtype=torch.float64):
    """(loss, index [heads, C], present [C], [d(weight * loss) / d(logits) per prediction]) evaluated in `dtype`.  With
    two heads that is per head the gradient of 0.5 * weight * loss_hd, the entry point's g1 and g2; with one, g1 + g2."""
    ps = [p.detach().to(dtype).requires_grad_(True) for p in preds]
    total, index, present = loss(ps, label, alpha, beta, gamma, smooth, ignore_label)
    (weight * total).backward()
    return total.detach(), index.detach(), present, [p.grad for p in ps]


def closed_form_grad(z, label, alpha=0.5, beta=0.5, gamma=1.0, smooth=0.0, ignore_label=IGNORE):
    """d loss / d z for ONE prediction already at the label resolution, the way the kernels compute it: per class the two
    coefficients dL/dq = -k (D - (1 - beta) N) / D^2 for the pixels of the class and +k alpha N / D^2 for the others, with
    D = N + M and k = gamma (M / D)^(gamma - 1) / n (0 for an absent class), and dz_k = q_k (u_k - sum_c q_c u_c) over
    the valid pixels."""
    C = z.shape[1]
    TP, FP, FN, Y = sums(z, label, ignore_label)
    N = TP + smooth
    M = alpha * FP + beta * FN + EPS
    D = N + M
    present = Y > 0
    n = max(int(present.sum()), 1)
    k = torch.where(present, gamma * (M / D) ** (gamma - 1.0) / n, torch.zeros_like(N))
    a = (-k * (D - (1.0 - beta) * N) / D ** 2).view(1, C, 1, 1)
    b = (k * alpha * N / D ** 2).view(1, C, 1, 1)
    ok = valid_mask(label, C, ignore_label)
    onehot = F.one_hot(torch.where(ok, label, torch.zeros_like(label)), C).permute(0, 3, 1, 2).bool()
    u = torch.where(onehot, a, b)
    q = torch.softmax(z, dim=1)
    return q * (u - (q * u).sum(1, keepdim=True)) * ok[:, None].to(z.dtype)


# ------------------------------------------------------------------------------------------------- inputs
def make_logits(b, c, h, w, seed, heads=2):
    g = torch.Generator().manual_seed(seed + 7919)
    return [3.0 * torch.randn(b, c, h, w, generator=g) for _ in range(heads)]


def make_label(b, C, H, W, seed):
    """Blocky class regions over the classes 0 .. C - 3 (the argmax of a bilinearly upsampled 3 x 4 grid), a tenth of the
    pixels ignored, class C - 2 on exactly one pixel, class C - 1 absent."""
    g = torch.Generator().manual_seed(seed + 104729)
    coarse = torch.randn(b, C - 2, 3, 4, generator=g, dtype=torch.float64)
    label = F.interpolate(coarse, size=(H, W), mode='bilinear', align_corners=True).argmax(1)
    label[torch.rand(b, H, W, generator=g) < 0.1] = IGNORE
    label[b - 1, H // 2, W - 1] = C - 2
    return label


# (low-resolution logits, label size): the upsample pipeline's edge shapes (tests/test_iast_gpu.py: SHAPES) -- odd sizes,
# an integer ratio, h == H, and a row wider than the workgroup (a thread owns more than one pixel of it)
CASE_SHAPES = [((5, 7), (33, 45)), ((4, 6), (64, 96)), ((9, 11), (9, 11)), ((4, 4), (64, 64)), ((3, 5), (48, 300))]
CLASSES = (6, 7, 16)
BATCH = 2
# (alpha, beta, gamma, smooth): Dice, soft Jaccard, a focal-Tversky
VARIANTS = dict(dice=(0.5, 0.5, 1.0, 0.0), jaccard=(1.0, 1.0, 1.0, 0.0), tversky=(0.3, 0.7, 1.5, 1.0))
_CASES = {}


def case_seed(C, k):
    return 1000 * C + 10 * k


def case(C, k):
    """The shared inputs of case (C, shape k), made once: labels int64, two heads of logits f32, and a cache for the
    references."""
    if (C, k) not in _CASES:
        lo, hi = CASE_SHAPES[k]
        seed = case_seed(C, k)
        _CASES[(C, k)] = dict(label=make_label(BATCH, C, *hi, seed), p=make_logits(BATCH, C, *lo, seed), lo=lo, hi=hi,
                              refs={})
    return _CASES[(C, k)]


def case_reference(d, heads, variant, weight=1.0, dtype=torch.float64):
    key = (heads, variant, weight, dtype)
    if key not in d['refs']:
        d['refs'][key] = loss_and_grads(d['p'][:heads], d['label'], *VARIANTS[variant], weight=weight, dtype=dtype)
    return d['refs'][key]
