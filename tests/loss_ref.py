"""CPU restatement of the losses of the --ls / --lt flags (regda/gast/balance.py:104-216,306-435), written from their
formulas in fp32 torch so that autograd gives the gradients.  Pinned to the reference's own classes by
tests/golden/losses.npz (tests/test_losses_cpu.py); the GPU tests compare the fused kernels against it.

`pixel_weight` is the per-pixel class weight of a ClassBalance call (oracle.labelpath.ClassBalanceState.pixel_weight),
or None.  Every function takes ONE prediction already at the label size; loss_calc upsamples and averages the heads."""
import torch
import torch.nn.functional as F

OHEM_THRESH = float(-torch.log(torch.tensor(0.7, dtype=torch.float)))      # f32 -log(0.7)
GHM_EDGES = torch.tensor([k / 30 for k in range(30)] + [1 + 1e-3], dtype=torch.float32)


def _ce(p, label, ig):
    return F.cross_entropy(p, label, ignore_index=ig, reduction='none').reshape(-1)


def entropy(soft):
    """u = sum_c -s log s per pixel (NaN where a class probability is exactly 0)."""
    return (-soft * torch.log(soft)).sum(1).reshape(-1)


def ohem(p, label, ig=-1, pixel_weight=None, thresh=OHEM_THRESH):
    lab = label.reshape(-1)
    n_min = int((lab != ig).sum()) // 5
    v = _ce(p, label, ig)
    if pixel_weight is not None:
        v = v * pixel_weight
    keep = v > thresh
    if int(keep.sum()) < n_min:
        # the n_min largest; of equal losses the lowest pixel index first (a stable descending sort)
        order = torch.sort(v.detach(), descending=True, stable=True).indices[:n_min]
        return v[order].mean()
    return v[keep].mean()


def focal(p, label, ig=-1, gamma=2.0):
    ce = _ce(p, label, ig)
    return ((1 - torch.exp(-ce)) ** gamma * ce).mean()


def ghm_g(p, label, ig=-1):
    """|p_y - 1| per pixel, -1 where the label is ignored."""
    prob = torch.softmax(p.detach(), 1).permute(0, 2, 3, 1).reshape(-1, p.shape[1])
    lab = label.reshape(-1)
    py = prob.gather(1, torch.where(lab == ig, torch.zeros_like(lab), lab)[:, None])[:, 0]
    return torch.where(lab == ig, torch.full_like(py, -1.0), (py - 1.0).abs())


class GhmState:
    """acc_sum of GHMLoss: persists across calls, updated once per call."""

    def __init__(self, momentum=0.99):
        self.momentum = momentum
        self.acc_sum = torch.zeros(30)


def ghm(p, label, state, ig=-1):
    g = ghm_g(p, label, ig)
    inr = (g >= 0) & (g <= 1)
    bins = torch.bincount((g[inr] * 30).floor().long().clamp(max=29), minlength=30).float()   # histc(g, 30, 0, 1)
    ind = (GHM_EDGES[None, :] < g[:, None]).sum(1)                                             # bucketize, right=False
    m = state.momentum
    state.acc_sum = m * state.acc_sum + (1 - m) * bins if m > 0 else bins
    w = torch.where((ind > 0) & (ind <= 30), 1.0 / state.acc_sum[ind - 1], torch.zeros_like(g))
    lab = label.reshape(-1)
    return (_ce(p, label, ig) * w).sum() / ((lab != -1).sum() + 1e-7)


def uvem_weight(u, m, t, gamma):
    left = torch.ones_like(u)
    if m > 0:
        x = torch.where((u <= m) & (u >= 0), u, left)
        left = torch.clamp((-1 / (m ** 2)) * (x - m) ** 2 + 1, 0.0, 1.0) ** (1.0 / gamma)
    right = torch.zeros_like(u)
    if m < t:
        x = torch.where((u > m) & (u <= t), u, right)
        right = torch.clamp((-1 / ((t - m) ** 2)) * (x - m) ** 2 + 1, 0.0, 1.0) ** (1.0 / gamma)
    w = torch.where(u <= m, left, right)
    return torch.where(u >= t, torch.zeros_like(u), w)


def ups(p, label, soft, ig=-1, pixel_weight=None, t=0.7, uvem=None):
    """UPSLoss; uvem=(m, gamma) gives UVEMLoss with the same threshold t."""
    lab = label.reshape(-1)
    u = entropy(soft)
    ce = torch.where(u > t, torch.zeros_like(u), _ce(p, label, ig))
    w = torch.ones_like(u) if uvem is None else uvem_weight(u, uvem[0], t, uvem[1])
    if pixel_weight is not None:
        w = w * pixel_weight
    return (w * ce).sum() / (((u <= t) & (lab != ig)).sum() + 1e-7)


def up(p, size):
    return p if p.shape[-2:] == size else F.interpolate(p, size=size, mode='bilinear', align_corners=True)


def make_loss(kind, ig=-1, balancer=None, ghm_state=None, m=0.2, t=0.7, gamma=4.0):
    """kind: 'ce', 'ohem', 'focal', 'ghm', 'ups', 'uvem' -> fn(p_full, label, soft) of ONE head call (the balancer is
    EMA-updated per call, as in the reference)."""
    pw = (lambda lab: balancer.pixel_weight(lab)) if balancer is not None else (lambda lab: None)
    if kind == 'ce':
        def fn(p, lab, soft):
            v = _ce(p, lab, ig)
            w = pw(lab)
            return (v if w is None else v * w).mean()
        return fn
    if kind == 'ohem':
        return lambda p, lab, soft: ohem(p, lab, ig, pw(lab))
    if kind == 'focal':
        return lambda p, lab, soft: focal(p, lab, ig)
    if kind == 'ghm':
        return lambda p, lab, soft: ghm(p, lab, ghm_state, ig)
    if kind == 'ups':
        return lambda p, lab, soft: ups(p, lab, soft, ig, pw(lab), 0.7)
    if kind == 'uvem':
        return lambda p, lab, soft: ups(p, lab, soft, ig, pw(lab), t, (m, gamma))
    raise ValueError(kind)


def loss_calc(preds, label, fn, soft=None):
    """tools.py:240-254 / balance.py:438-460 (multi=True): upsample each head, one loss call per head, mean."""
    total = 0
    for p in preds:
        total = total + fn(up(p, label.shape[-2:]), label.long(), soft)
    return total / len(preds)


def near_boundary(kind, p_full, label, soft=None, eps=1e-5, ig=-1, pixel_weight=None, m=0.2, t=0.7):
    """Pixels of ONE head whose decision value lies within eps of a boundary of the loss's decisions: the OHEM threshold
    (or the k-th largest value), the GHM bin edges, the UPS / UVEM gate t and UVEM's branch point m.  Their gradient
    may legitimately differ between two correct implementations."""
    lab = label.reshape(-1)
    if kind == 'ohem':
        v = _ce(p_full, label, ig).detach()
        if pixel_weight is not None:
            v = v * pixel_weight
        n_min = int((lab != ig).sum()) // 5
        near = (v - OHEM_THRESH).abs() < eps
        if int((v > OHEM_THRESH).sum()) < n_min and n_min > 0:
            kth = torch.sort(v, descending=True).values[n_min - 1]
            near = ((v - kth).abs() < eps) & (v != kth)     # equal values follow the tie rule on both sides
        return near
    if kind == 'ghm':
        g = ghm_g(p_full, label, ig)
        return ((g[:, None] - GHM_EDGES[None, :30]).abs() < eps).any(1) & (g > 0)
    if kind in ('ups', 'uvem'):
        u = entropy(soft)
        near = (u - t).abs() < eps
        if kind == 'uvem':
            near |= (u - m).abs() < eps
        return near
    return torch.zeros_like(lab, dtype=torch.bool)
