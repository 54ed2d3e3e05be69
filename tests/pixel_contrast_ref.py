"""The pixel-to-pixel contrastive loss (regda/gast/contrastive.py::PixelContrastLoss) restated for the tests: the
selection (nearest downscale, the (class, hard / easy) lists, the keep counts and the recorded `randperm` draws), the loss
and its closed-form feature gradient in float64, float64 autograd of the definition, and the arithmetic contract of
rgda_pixel_contrast_loss (include/rgda_hip.h) emulated on the CPU.  Nothing here imports the product."""
import numpy as np
import torch

BF = torch.bfloat16
NAMES = ['b2_k64_16x16_live', 'b2_k64_16x16_sat', 'b3_k96_16x16_live', 'b3_k64_16x32', 'b2_k64_few_easy',
         'b2_k64_few_hard', 'b2_k64_hard0', 'b2_k64_absent']


# ------------------------------------------------------------------------------------------------ selection
def downscale_labels(labels, size):
    """what `interpolate(labels.float(), size, mode='nearest').long()` reads for integer ratios: pixel (y H / h, x W / w)"""
    h, w = size
    b, H, W = labels.shape
    assert H % h == 0 and W % w == 0
    return labels[:, ::H // h, ::W // w].contiguous()


def predict_labels(predict):
    """int64 (b, h, w) as it is; f32 logits (b, C, h, w) -> argmax, the lowest index on ties (numpy's rule)"""
    if predict.dtype == torch.int64:
        return predict
    return torch.from_numpy(np.argmax(predict.numpy(), axis=1)).long()


def select_restated(labels, predict, C, size, ignore_label=-1):
    """-> counts int32 (b, C, 2), order int32 (b, h*w), flag (4 when a label outside [0, C) is not ignore_label)"""
    lab = downscale_labels(labels, size).reshape(labels.shape[0], -1)
    pr = predict_labels(predict).reshape(lab.shape[0], -1)
    valid = (lab >= 0) & (lab < C) & (lab != ignore_label)
    flag = 4 if bool(((lab != ignore_label) & ~((lab >= 0) & (lab < C))).any()) else 0
    key = torch.where(valid, 2 * lab + (pr == lab).long(), torch.full_like(lab, 2 * C))
    order = torch.from_numpy(np.argsort(key.numpy(), axis=1, kind='stable')).int()
    counts = torch.stack([(key == q).sum(1) for q in range(2 * C)], 1).view(-1, C, 2).int()
    return counts, order, flag


def keep_counts(num_hard, num_easy, n_view):
    """contrastive.py:82-90"""
    if num_hard >= n_view / 2 and num_easy >= n_view / 2:
        return n_view // 2, n_view - n_view // 2
    if num_hard >= n_view / 2:
        return n_view - num_easy, num_easy
    assert num_easy >= n_view / 2
    return num_hard, n_view - num_hard


def sampling_restated(labels, predict, size, perms, ignore_label=-1, max_samples=1024, max_views=100):
    """`_hard_anchor_sampling` on the downscaled label and the prediction with the recorded draws `perms` (a list of
    int64 tensors, in the reference's order) -> (pixel indices (A, n_view) int64 within each anchor's image, anchors as a
    list of (image, class, hard_keep), n_view); (None, [], 0) when no class qualifies.  Written from the reference's
    lists (`nonzero` per image and class), not from the sorted order the kernel uses."""
    lab = downscale_labels(labels, size).reshape(labels.shape[0], -1)
    pr = predict_labels(predict).reshape(lab.shape[0], -1)
    found = []
    for i in range(lab.shape[0]):
        for c in torch.unique(lab[i]).tolist():
            if c != ignore_label and int((lab[i] == c).sum()) > max_views:
                found.append((i, c))
    if not found:
        return None, [], 0
    n_view = min(max_samples // len(found), max_views)
    perms = list(perms)
    sel, anchors = [], []
    for i, c in found:
        hard = ((lab[i] == c) & (pr[i] != c)).nonzero().view(-1)
        easy = ((lab[i] == c) & (pr[i] == c)).nonzero().view(-1)
        hk, ek = keep_counts(hard.numel(), easy.numel(), n_view)
        ph, pe = perms.pop(0), perms.pop(0)
        assert ph.numel() == hard.numel() and pe.numel() == easy.numel()
        sel.append(torch.cat([hard[ph[:hk]], easy[pe[:ek]]]))
        anchors.append((i, c, hk))
    assert not perms
    return torch.stack(sel), anchors, n_view


def rows_from_tables(counts, order, anchors, ranks):
    """what rgda_pixel_contrast_loss gathers: row r = v A + a -> (global pixel row image * hw + pixel, class), from the
    kernel-side tables (counts, order) and the plan (anchors int32 [A, 3], ranks int32 [A, n_view])"""
    A, n_view = ranks.shape
    hw = order.shape[1]
    pix = torch.empty(n_view, A, dtype=torch.int64)
    cls = torch.empty(n_view, A, dtype=torch.int64)
    flat = counts.reshape(counts.shape[0], -1).long()
    for a in range(A):
        i, c, hk = (int(v) for v in anchors[a])
        start = int(flat[i, :2 * c].sum())
        easy0 = start + int(flat[i, 2 * c])
        for v in range(n_view):
            slot = (start if v < hk else easy0) + int(ranks[a, v])
            pix[v, a] = i * hw + int(order[i, slot])
            cls[v, a] = c
    return pix.view(-1), cls.view(-1)


def view_major(sel, anchors, hw):
    """(A, n_view) in-image pixel indices -> the N = n_view * A global pixel rows and classes, r = v A + a"""
    img = torch.tensor([a[0] for a in anchors])
    cls = torch.tensor([a[1] for a in anchors])
    return (sel + img[:, None] * hw).t().reshape(-1), cls[None, :].expand(sel.shape[1], -1).reshape(-1)


def pixel_rows(feats):
    """NCHW (b, k, h, w) -> (b*h*w, k) pixel-major rows"""
    return feats.permute(0, 2, 3, 1).reshape(-1, feats.shape[1])


# ------------------------------------------------------------------------------------------------ loss and gradient
def _masks(cls):
    same = cls[:, None] == cls[None, :]
    eye = torch.eye(cls.numel(), dtype=torch.bool)
    return same & ~eye, ~same


def contrast_restated(F, cls, temperature=0.1, base_temperature=0.07, eps=1e-5):
    """float64: F (N, k) the selected rows view-major, cls (N,) -> (loss, dL/dF by the closed form)"""
    F = F.double()
    N = F.shape[0]
    pos, negm = _masks(cls)
    G = F @ F.T / temperature
    l = G - G.max(1, keepdim=True).values
    e = torch.exp(l)
    neg = (e * negm).sum(1, keepdim=True)
    d = e + neg + eps
    lp = l - torch.log(d)
    P = pos.sum(1).double()
    scale = -(temperature / base_temperature)
    loss = scale * ((pos * lp).sum(1) / (P + eps)).mean()
    c = (scale / (N * (P + eps)))[:, None]
    s1 = (pos / d).sum(1, keepdim=True)
    Wm = torch.where(pos, c * (1 - e / d), torch.zeros_like(e)) + torch.where(negm, -c * e * s1, torch.zeros_like(e))
    return loss, (Wm + Wm.T) @ F / temperature


def contrast_graph(F, cls, temperature=0.1, base_temperature=0.07, eps=1e-5):
    """the definition (the mask algebra of contrastive.py:107-143, the row maximum detached) on F (N, k) in F's own
    dtype, as a differentiable torch expression: what a composed oracle adds to its loss"""
    N = F.shape[0]
    mask = (cls[:, None] == cls[None, :]).to(F.dtype)
    adc = F @ F.T / temperature
    logits = adc - adc.max(1, keepdim=True).values.detach()
    neg_mask = 1 - mask
    mask = mask * (1 - torch.eye(N, dtype=F.dtype))
    neg_logits = (torch.exp(logits) * neg_mask).sum(1, keepdim=True)
    log_prob = logits - torch.log(torch.exp(logits) + neg_logits + eps)
    return (-(temperature / base_temperature) * (mask * log_prob).sum(1) / (mask.sum(1) + eps)).mean()


def contrast_autograd(F, cls, temperature=0.1, base_temperature=0.07, eps=1e-5):
    """float64 autograd of the definition"""
    F = F.double().clone().requires_grad_(True)
    loss = contrast_graph(F, cls, temperature, base_temperature, eps)
    loss.backward()
    return loss.detach(), F.grad


def contrast_emulated(F, cls, temperature=0.1, base_temperature=0.07, eps=1e-5, weight=1.0, sums='exact'):
    """The kernel's rounding contract on the CPU -> (loss fp32, the gradient rows as the bf16 values the kernel stores,
    float32).  sums='exact': every fp32 sum is the exact sum rounded once; sums='fp32': the sums run in fp32 in the
    CPU library's order.  The kernel's sums run in fp32 in a third order; the two variants differ from each other as
    two legitimate orders do, which is what the tight bounds are made of (derive_pixel_contrast_tolerances.py)."""
    f32 = np.float32
    X = F.float().to(BF).float()
    N = X.shape[0]
    pos, negm = _masks(cls)

    def mm(a, b):
        return (a.double() @ b.double()).float() if sums == 'exact' else a @ b

    def rsum(t):
        return t.double().sum(1).float() if sums == 'exact' else t.sum(1)

    G = mm(X, X.T) / f32(temperature)
    G = torch.triu(G) + torch.triu(G, 1).T               # stored symmetric
    m = G.max(1, keepdim=True).values
    l = G - m
    e = torch.exp(l)
    neg = rsum(e * negm)[:, None]
    epsf = f32(eps)
    d = e + neg + epsf
    lp = l - torch.log(d)
    P = pos.sum(1).float()
    cscale = f32(-(f32(temperature) / f32(base_temperature)) / f32(N))
    rowloss = rsum(torch.where(pos, lp, torch.zeros_like(lp))) / (P + epsf)
    tot = rowloss.double().sum().float() if sums == 'exact' else rowloss.sum()
    loss = f32(f32(weight) * cscale) * tot
    c = (cscale / (P + epsf))[:, None]
    s1 = rsum(torch.where(pos, 1.0 / d, torch.zeros_like(d)))[:, None]
    Wm = torch.where(pos, c * (1 - e / d), torch.zeros_like(e)) + torch.where(negm, -c * e * s1, torch.zeros_like(e))
    M = (Wm + Wm.T).to(BF).float()
    g = (f32(f32(weight) / f32(temperature)) * mm(M, X)).to(BF).float()
    return loss, g


# ------------------------------------------------------------------------------------------------ fixtures
def golden_cases(g):
    """the fixture's cases as dicts: name, seed, feats f32 (b, k, h, w), labels int64 (b, H, W), predict int64
    (b, h, w), perms (the recorded randperm results), sel (A, n_view) the reference's selected in-image pixel indices,
    classes (A,), loss, grad f32 (N, k): the reference's gradient at the selected rows, view-major (every other row of
    its gradient was zero: checked when the file was minted)"""
    for name in [str(n) for n in g['names']]:
        src = str(g[name + '_like']) if name + '_like' in g else name       # a case may share another's inputs and draws
        q = torch.from_numpy(g[src + '_q'].astype(np.float32))
        feats = q / 8.0 * float(g[name + '_scale'])
        lens = g[src + '_perm_lens']
        flat = torch.from_numpy(g[src + '_perms'].astype(np.int64))
        perms, o = [], 0
        for n in lens:
            perms.append(flat[o:o + int(n)])
            o += int(n)
        yield dict(name=name, seed=int(g[name + '_seed']), feats=feats, labels=torch.from_numpy(g[src + '_labels'].astype(np.int64)),
                   predict=torch.from_numpy(g[src + '_predict'].astype(np.int64)), perms=perms,
                   sel=torch.from_numpy(g[name + '_sel'].astype(np.int64)), classes=torch.from_numpy(g[name + '_classes'].astype(np.int64)),
                   loss=float(g[name + '_loss']), grad=torch.from_numpy(g[name + '_grad']))


def case_rows(c):
    """-> (the N global pixel rows, their classes) of a golden case, from the reference's own selection"""
    hw = c['feats'].shape[2] * c['feats'].shape[3]
    sel, anchors, n_view = sampling_restated(c['labels'], c['predict'], c['feats'].shape[2:], c['perms'])
    return view_major(sel, anchors, hw)


def production_inputs(seed=2048, b=2, k=2048, h=32, w=32, C=7):
    """the production channel count once: instance-norm-like features (unit normal), labels at feature resolution in
    vertical bands of four classes per image (256 pixels each), 30 % of the predictions moved to the next class
    -> (feats, labels, predict, C); A = 8, n_view = 100, N = 800"""
    gen = torch.Generator().manual_seed(seed)
    feats = torch.randn(b, k, h, w, generator=gen)
    labels = (torch.arange(w) // (w // 4))[None, None, :].expand(b, h, w).clone()
    labels[1] += 2
    flip = torch.rand(b, h, w, generator=gen) < 0.3
    predict = torch.where(flip, (labels + 1) % C, labels)
    return feats, labels.long(), predict.long(), C


def production_plan(labels, predict, size, seed=2048):
    """the draws of the production case: the restated lists and keep counts with randperm from a seeded generator
    -> (global pixel rows, classes)"""
    gen = torch.Generator().manual_seed(seed)
    counts, order, _ = select_restated(labels, predict, 16, size)
    perms = []
    found = [(i, c) for i in range(counts.shape[0]) for c in range(counts.shape[1]) if int(counts[i, c].sum()) > 100]
    for i, c in found:
        perms.append(torch.randperm(int(counts[i, c, 0]), generator=gen))
        perms.append(torch.randperm(int(counts[i, c, 1]), generator=gen))
    sel, anchors, n_view = sampling_restated(labels, predict, size, perms)
    return view_major(sel, anchors, size[0] * size[1]), perms
