"""The class-aware whitening loss restated from its formulas (not from the reference's code), for the tests:

    for every class c of class_ids and every group g of s = k / groups consecutive channels:
        n_c = number of pixels labelled c;   n_c <= 1: the block contributes 0
        B = the (n_c, s) rows of the group for the class's pixels, minus their mean
        S = B^T B / (n_c - 1);   term = mean((S - I)^2) over the s^2 elements
    L = sum of the terms
    dL/dx_p[g block] = 4 (x_p - mu_c)[g block] (S_cg - I) / (s^2 (n_c - 1))   for a pixel p of class c with n_c >= 2,
    0 for every other pixel.

`whiten_restated` is that in float64; `whiten_emulated` follows the arithmetic contract of rgda_whiten_loss
(include/rgda_hip.h): fp32 class means, centred operands rounded to bf16 once, fp32 sums of the bf16 products,
S - I in fp32, bf16(S - I) in the gradient product, the gradient stored in bf16."""
import torch

BF = torch.bfloat16


def rows_of(x):
    """(b, k, h, w) -> (b*h*w, k) pixel rows"""
    return x.permute(0, 2, 3, 1).reshape(-1, x.shape[1])


def _as_map(g, shape):
    b, k, h, w = shape
    return g.view(b, h, w, k).permute(0, 3, 1, 2)


def whiten_restated(feats, labels, class_ids, groups):
    """feats (b, k, h, w), labels (b, h, w) or (b, 1, h, w) -> (loss, dL/dfeats in feats' shape), float64"""
    x = rows_of(feats.double())
    lab = labels.reshape(-1)
    k = x.shape[1]
    s = k // groups
    eye = torch.eye(s, dtype=torch.float64)
    loss = torch.zeros((), dtype=torch.float64)
    grad = torch.zeros_like(x)
    for c in class_ids:
        sel = (lab == c).nonzero().flatten()
        n = sel.numel()
        if n <= 1:
            continue
        xc = x[sel] - x[sel].mean(0)
        for g in range(groups):
            blk = xc[:, g * s:(g + 1) * s]
            d = blk.T @ blk / (n - 1) - eye
            loss = loss + (d * d).mean()
            grad[sel, g * s:(g + 1) * s] = 4.0 * blk @ d / (s * s * (n - 1))
    return loss, _as_map(grad, feats.shape)


def whiten_differentiable(feats, labels, class_ids, groups):
    """the same loss written with differentiable operations only, in feats' dtype, connected to feats' graph"""
    x = rows_of(feats)
    lab = labels.reshape(-1)
    s = x.shape[1] // groups
    eye = torch.eye(s, dtype=x.dtype)
    loss = torch.zeros((), dtype=x.dtype)
    for c in class_ids:
        sel = (lab == c).nonzero().flatten()
        n = sel.numel()
        if n <= 1:
            continue
        xc = x[sel] - x[sel].mean(0, keepdim=True)
        for g in range(groups):
            blk = xc[:, g * s:(g + 1) * s]
            loss = loss + ((blk.T @ blk / (n - 1) - eye) ** 2).mean()
    return loss


def whiten_restated_autograd(feats, labels, class_ids, groups):
    """-> (loss, float64 autograd gradient of whiten_differentiable)"""
    f = feats.double().clone().requires_grad_(True)
    loss = whiten_differentiable(f, labels, class_ids, groups)
    if loss.requires_grad:
        loss.backward()
        return loss.detach(), f.grad
    return loss, torch.zeros_like(f)


def whiten_emulated(feats, labels, class_num, groups, weight=1.0):
    """The kernel's rounding contract on the CPU -> (loss fp32, gradient as the bf16 values the kernel stores, in
    feats' shape, float32).  Only the order of the fp32 sums differs from the kernel."""
    x = rows_of(feats.float())
    lab = labels.reshape(-1)
    k = x.shape[1]
    s = k // groups
    eye = torch.eye(s)
    loss = torch.zeros(())
    grad = torch.zeros_like(x)
    for c in range(class_num):
        sel = (lab == c).nonzero().flatten()
        n = sel.numel()
        if n <= 1:
            continue
        xc = (x[sel] - x[sel].mean(0)).to(BF).float()
        for g in range(groups):
            blk = xc[:, g * s:(g + 1) * s]
            d = blk.T @ blk / (n - 1) - eye
            loss = loss + (d * d).sum() / (s * s)
            grad[sel, g * s:(g + 1) * s] = (blk @ d.to(BF).float()) * (4.0 * weight / (s * s * (n - 1)))
    return weight * loss, _as_map(grad.to(BF).float(), feats.shape)


def golden_cases(g):
    """the fixture's cases as dicts: name, feats (b,k,h,w) f32, labels (b,h,w) int64, class_num, groups, loss, grad"""
    for name in [str(n) for n in g['names']]:
        q = g[name + '_q']
        yield dict(name=name, feats=torch.from_numpy(q.astype('float32') / 32.0) * float(g[name + '_scale']),
                   labels=torch.from_numpy(g[name + '_lab'].astype('int64')), class_num=int(g[name + '_C']),
                   groups=int(g[name + '_groups']), loss=float(g[name + '_loss']),
                   grad=torch.from_numpy(g[name + '_grad']))


def production_inputs(seed=2048, b=8, k=2048, h=32, w=32, class_num=6):
    """8 x 2048 x 32 x 32 features (unit normal with a per-channel scale between 0.6 and 1.4 and a per-class offset, so
    that neither the means nor S - I are noise) and blocky labels with unequal class frequencies: about 35 / 25 / 15 /
    10 / 5 / 2 % of the pixels and 8 % ignored."""
    gen = torch.Generator().manual_seed(seed)
    freq = torch.tensor([0.08, 0.35, 0.25, 0.15, 0.10, 0.05, 0.02][:class_num + 1])
    cells = torch.multinomial(freq / freq.sum(), b * (h // 4) * (w // 4), replacement=True, generator=gen) - 1
    lab = cells.view(b, h // 4, w // 4).repeat_interleave(4, 1).repeat_interleave(4, 2)
    noise = torch.rand(b, h, w, generator=gen) < 0.1
    rnd = torch.multinomial(freq / freq.sum(), b * h * w, replacement=True, generator=gen).view(b, h, w) - 1
    lab = torch.where(noise, rnd, lab).long()
    scale = 0.6 + 0.8 * torch.rand(1, k, 1, 1, generator=gen)
    offs = 0.5 * torch.randn(class_num + 1, k, generator=gen)
    feats = torch.randn(b, k, h, w, generator=gen) * scale + offs[lab + 1].permute(0, 3, 1, 2)
    return feats.contiguous(), lab
