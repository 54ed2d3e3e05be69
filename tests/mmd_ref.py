"""The MMD loss of regda/gast/mmd.py restated from its formulas (not from the reference's code), for the tests.

    total = source rows then target rows, n = ns + nt;  l2_ij = |x_i - x_j|^2
    bw = fix_sigma, or sum_ij l2_ij / (n^2 - n);  bw /= kernel_mul^(kernel_num // 2);  bw_q = bw kernel_mul^q
    kappa_ij = sum_q exp(-l2_ij / bw_q);  s_ij = 1/ns^2 (source-source), 1/nt^2 (target-target), -1/(ns nt) (mixed)
    L = sum_ij s_ij kappa_ij
    closed forms: l2_ij = r_i + r_j - 2 x_i.x_j on rows centred by the common mean (r_i = |x_i|^2),
                  sum_ij l2_ij = 2 n sum_i r_i - 2 |sum_i x_i|^2,
                  W_ij = s_ij sum_q exp(-l2_ij / bw_q) / bw_q (W_ii = 0), rho_i = sum_j W_ij,
                  dL/dx_i = -4 (rho_i x_i - sum_j W_ij x_j)     (the bandwidth is a constant of the backward)
    linear: L = |mean_s - mean_t|^2 / d; dL/dxs rows 2 (mean_s - mean_t) / (d ns), dL/dxt rows -2 (...) / (d nt)

`mmd_restated` is the closed form in float64; `mmd_pairwise_autograd` the plain pairwise definition differentiated by
float64 autograd; `mmd_emulated` follows the arithmetic contract of rgda_mmd_loss (include/rgda_hip.h): fp32 mean,
centred rows rounded to bf16 once, fp32 sums of the bf16 products, fp32 epilogue, bf16 W, fp32 row sums of the rounded
W, the gradient stored in bf16."""
import numpy as np
import torch

BF = torch.bfloat16


def rows_of(x):
    """(b, d, h, w) -> (b*h*w, d) pixel rows; (n, d) as it is"""
    return x.permute(0, 2, 3, 1).reshape(-1, x.shape[1]) if x.dim() == 4 else x


def pair_weights(ns, nt, dtype):
    a = torch.cat([torch.full((ns,), 1.0 / ns, dtype=dtype), torch.full((nt,), -1.0 / nt, dtype=dtype)])
    return a[:, None] * a[None, :]


def bandwidth_pairwise(total):
    """the reference's definition: the explicit sum of all pairwise squared distances / (n^2 - n)"""
    n = total.shape[0]
    l2 = ((total[None, :, :] - total[:, None, :]) ** 2).sum(2)
    return l2.sum() / (n * n - n)


def bandwidth_closed(total):
    n = total.shape[0]
    r = (total * total).sum(1)
    return (2 * n * r.sum() - 2 * (total.sum(0) ** 2).sum()) / (n * n - n)


def _bandwidths(bw, kernel_mul, kernel_num):
    bw = bw / kernel_mul ** (kernel_num // 2)
    return [bw * kernel_mul ** q for q in range(kernel_num)]


def mmd_linear_restated(xs, xt):
    xs, xt = xs.double(), xt.double()
    d, ns, nt = xs.shape[1], xs.shape[0], xt.shape[0]
    delta = xs.mean(0) - xt.mean(0)
    return (delta * delta).sum() / d, (2 * delta / (d * ns)).expand(ns, d), (-2 * delta / (d * nt)).expand(nt, d)


def mmd_restated(xs, xt, kernel_type='rbf', kernel_mul=2.0, kernel_num=5, fix_sigma=None):
    """rows (ns, d), (nt, d) -> (loss, dL/dxs, dL/dxt), float64 closed forms"""
    if kernel_type == 'linear':
        return mmd_linear_restated(xs, xt)
    ns, nt = xs.shape[0], xt.shape[0]
    total = torch.cat([xs, xt]).double()
    x = total - total.mean(0)
    r = (x * x).sum(1)
    l2 = (r[:, None] + r[None, :] - 2 * x @ x.T).clamp_min(0)
    l2.fill_diagonal_(0)
    bws = _bandwidths(fix_sigma if fix_sigma else bandwidth_closed(x), kernel_mul, kernel_num)
    s = pair_weights(ns, nt, torch.float64)
    loss = (s * sum(torch.exp(-l2 / b) for b in bws)).sum()
    W = s * sum(torch.exp(-l2 / b) / b for b in bws)
    W.fill_diagonal_(0)
    g = -4 * (W.sum(1)[:, None] * x - W @ x)
    return loss, g[:ns], g[ns:]


def mmd_pairwise_autograd(xs, xt, kernel_mul=2.0, kernel_num=5, fix_sigma=None):
    """the plain pairwise definition, float64 autograd -> (loss, dL/dxs, dL/dxt)"""
    xs, xt = xs.double().clone().requires_grad_(True), xt.double().clone().requires_grad_(True)
    ns = xs.shape[0]
    total = torch.cat([xs, xt])
    l2 = ((total[None, :, :] - total[:, None, :]) ** 2).sum(2)
    n = total.shape[0]
    bw = fix_sigma if fix_sigma else (l2.detach().sum() / (n * n - n))
    k = sum(torch.exp(-l2 / b) for b in _bandwidths(bw, kernel_mul, kernel_num))
    loss = k[:ns, :ns].mean() + k[ns:, ns:].mean() - k[:ns, ns:].mean() - k[ns:, :ns].mean()
    loss.backward()
    return loss.detach(), xs.grad, xt.grad


def mmd_differentiable(xs, xt, kernel_type='rbf', kernel_mul=2.0, kernel_num=5, fix_sigma=None):
    """the loss in the inputs' dtype, connected to their graph (Gram form; the bandwidth detached as in the reference)"""
    ns = xs.shape[0]
    if kernel_type == 'linear':
        delta = xs.mean(0) - xt.mean(0)
        return (delta * delta).sum() / delta.shape[0]
    total = torch.cat([xs, xt])
    x = total - total.mean(0, keepdim=True)
    r = (x * x).sum(1)
    l2 = (r[:, None] + r[None, :] - 2 * x @ x.T).clamp_min(0)
    l2 = l2 * (1 - torch.eye(l2.shape[0], dtype=l2.dtype))
    bws = _bandwidths(fix_sigma if fix_sigma else bandwidth_closed(x.detach()), kernel_mul, kernel_num)
    return (pair_weights(ns, xt.shape[0], l2.dtype) * sum(torch.exp(-l2 / b) for b in bws)).sum()


def mmd_emulated(xs, xt, kernel_type='rbf', kernel_mul=2.0, kernel_num=5, fix_sigma=None, weight=1.0, parts=False):
    """The kernel's rounding contract on the CPU -> (loss fp32, the two gradients as the bf16 values the kernel stores,
    float32).  Only the order of the fp32 sums and the device exp differ from the kernel.  parts=True also returns
    (W as float32 of its bf16 values, the centred bf16 rows as float32, sum_ij |s_ij| kappa_ij)."""
    xs, xt = xs.float(), xt.float()
    ns, nt, d = xs.shape[0], xt.shape[0], xs.shape[1]
    if kernel_type == 'linear':
        delta = xs.mean(0) - xt.mean(0)
        gs = (weight * 2.0 / (d * ns) * delta).to(BF).float().expand(ns, d)
        gt = (-weight * 2.0 / (d * nt) * delta).to(BF).float().expand(nt, d)
        return weight * (delta * delta).sum() / d, gs, gt
    n = ns + nt
    total = torch.cat([xs, xt])
    mu = (xs.sum(0) + xt.sum(0)) / n
    x = (total - mu).to(BF).float()
    r = (x * x).sum(1)
    l2 = (r[:, None] + r[None, :] - 2 * (x @ x.T)).clamp_min(0)
    l2.fill_diagonal_(0)
    if fix_sigma:
        bw = torch.tensor(float(fix_sigma))
    else:
        bw = (2.0 * n * r.sum() - 2.0 * (x.sum(0) ** 2).sum()) * np.float32(1.0 / (float(n) * n - n))
    bw = bw * np.float32(1.0 / float(kernel_mul) ** (kernel_num // 2))
    ibs, m = [], np.float32(1.0)
    for _ in range(kernel_num):
        ibs.append(1.0 / (bw * m))
        m = np.float32(m * np.float32(kernel_mul))
    s = pair_weights(ns, nt, torch.float32)
    kap = torch.zeros_like(l2)
    wsum = torch.zeros_like(l2)
    for ib in ibs:
        e = torch.exp(-l2 * ib)
        kap += e
        wsum += e * ib
    loss = weight * (s * kap).sum()
    W = (s * wsum).to(BF).float()
    W.fill_diagonal_(0)
    g = ((-4.0 * weight) * (W.sum(1)[:, None] * x - W @ x)).to(BF).float()
    return (loss, g[:ns], g[ns:], W, x, (s.abs() * kap).sum().item()) if parts else (loss, g[:ns], g[ns:])


def relu_like(gen, n, d, scale, shift):
    """post-ReLU-like rows on a grid of 1/32: a per-channel offset plus noise, clipped at 0, then scaled and shifted"""
    base = torch.rand(1, d, generator=gen) * 1.5
    q = torch.clamp(torch.round((base + torch.randn(n, d, generator=gen)) * 32.0), 0, 255)
    return q.to(torch.uint8), scale, shift


def golden_cases(g):
    """the fixture's cases as dicts: name, xs, xt (rows, f32), settings (MMDLoss keyword arguments), loss, gs, gt"""
    for name in [str(n) for n in g['names']]:
        a, b, o = (float(v) for v in g[name + '_scales'])
        st = {}
        if name + '_kernel_mul' in g:
            st['kernel_mul'] = float(g[name + '_kernel_mul'])
        if name + '_kernel_num' in g:
            st['kernel_num'] = int(g[name + '_kernel_num'])
        if name + '_fix_sigma' in g:
            st['fix_sigma'] = float(g[name + '_fix_sigma'])
        if name + '_linear' in g:
            st['kernel_type'] = 'linear'
        yield dict(name=name, xs=torch.from_numpy(g[name + '_qs'].astype(np.float32) / 32.0) * a,
                   xt=torch.from_numpy(g[name + '_qt'].astype(np.float32) / 32.0) * b + o, settings=st,
                   loss=float(g[name + '_loss']), gs=torch.from_numpy(g[name + '_gs']), gt=torch.from_numpy(g[name + '_gt']))


def production_inputs(seed=4096, b=2, d=2048, h=32, w=32):
    """one (2b, d, h, w) map whose two batch halves are the domains: ReLU-like features (a per-channel offset plus unit
    noise, clipped at 0), the target half scaled by 1.3 and shifted by 0.2"""
    gen = torch.Generator().manual_seed(seed)
    base = torch.rand(1, d, 1, 1, generator=gen) * 1.5
    f = torch.clamp(base + torch.randn(2 * b, d, h, w, generator=gen), min=0.0)
    f[b:] = f[b:] * 1.3 + 0.2
    return f.contiguous(), b
