"""The semantic-aware whitening loss (regda/gast/SAW.py) restated from its formulas (not from the reference's code), for
the tests:

    A = |W| (n_cls, k);  C = len(selected);  G = k // C;  nod = C (C - 1) / 2
    slot (g, j), g < G: ch[g][j] = the channel of rank g of A[selected[j]] in descending order, equal values by the lower
    channel index;  wgh[g][j] = sigmoid(A[selected[j]][ch[g][j]])
    xt[b][g][j][p] = wgh[g][j] x[b][ch[g][j]][p];   cov[b][g] = xt xt^T / (hw - 1)   (no centring)
    s[b][g] = sum_{j < j'} |cov_jj'|;   margin = 0 if relax_denom == 0 else nod // relax_denom
    L = sum_g sum_b max((s - margin) / nod, 0) / B
    for s > margin:  dL/dxt_j[p] = sum_{j' != j} sign(cov_jj') xt_j'[p] / (B nod (hw - 1));  dL/dx sums wgh dL/dxt over the
    slots of a channel.

`saw_restated` is that in float64, `saw_emulated` in float32 (the arithmetic contract of rgda_saw_loss without the bf16
store of the gradient), `saw_differentiable` is written with differentiable operations only."""
import torch


def saw_margin(C, relax_denom):
    nod = float(C * (C - 1) // 2)
    return 0.0 if relax_denom == 0 else float(nod // relax_denom)


def saw_plan(W, selected, k=None):
    """-> (ch int64 [G, C], A float64 [G, C]: |w| of the slot's channel for its class).  Stable ranks: descending |w|,
    equal values by the lower channel index."""
    A = W.detach().double().abs()
    k = A.shape[1] if k is None else k
    C = len(selected)
    G = k // C
    order = torch.stack([torch.sort(A[c], descending=True, stable=True).indices for c in selected], 1)      # [k, C]
    ch = order[:G]
    a = torch.stack([A[c][ch[:, j]] for j, c in enumerate(selected)], 1)
    return ch, a


def pair_index(C):
    """the pairs (j, j'), j < j', row-major -- the order of the kernel's sign table"""
    iu = torch.triu_indices(C, C, 1)
    return iu[0], iu[1]


def _signs_matrix(signs, C):
    """[b, G, nod] pair signs -> the symmetric [b, G, C, C] matrix with a zero diagonal"""
    j0, j1 = pair_index(C)
    S = torch.zeros(*signs.shape[:2], C, C, dtype=signs.dtype)
    S[:, :, j0, j1] = signs
    S[:, :, j1, j0] = signs
    return S


def _saw(feats, W, selected, relax_denom, dtype, table=None):
    b, k, h, w = feats.shape
    hw = h * w
    C = len(selected)
    nod = C * (C - 1) // 2
    margin = saw_margin(C, relax_denom)
    ch, a = saw_plan(W, selected, k)
    G = ch.shape[0]
    wgh = torch.sigmoid(a.to(dtype))                                        # [G, C]
    x = feats.to(dtype).reshape(b, k, hw)
    xt = x[:, ch.reshape(-1)].view(b, G, C, hw) * wgh.view(1, G, C, 1)
    cov = xt @ xt.transpose(2, 3) / (hw - 1)
    j0, j1 = pair_index(C)
    corr = cov[:, :, j0, j1]                                                # [b, G, nod]
    s = corr.abs().sum(-1)
    active = s > margin
    loss = (torch.clamp((s - margin) / nod, min=0).sum() / b).to(dtype)
    if table is None:
        signs, act = torch.sign(corr), active
    else:
        signs, act = table['signs'].to(dtype), table['active']
    S = _signs_matrix(signs, C) * act.view(b, G, 1, 1).to(dtype)
    dslot = (S @ xt) * (wgh.view(1, G, C, 1) / (b * nod * (hw - 1)))
    grad = torch.zeros(b, k, hw, dtype=dtype).index_add_(1, ch.reshape(-1), dslot.view(b, G * C, hw))
    norms = xt.norm(dim=3)                                                  # [b, G, C]
    return dict(loss=loss, grad=grad.view(b, k, h, w), s=s, corr=corr, active=active, signs=torch.sign(corr).to(torch.int8),
                ch=ch, wgh=wgh, margin=margin, nod=nod, norms=norms)


def loss_scale(r):
    """sum over the active groups of s / (nod B): what a loss deviation is measured against (s - margin cancels, so a
    bound relative to the loss itself would measure the margin)"""
    return (r['s'][r['active']].sum() / (r['nod'] * r['s'].shape[0])).item()


def fp32_s_bound(r, hw):
    """Worst case of an fp32 s against float64 `r`, [b, G]: a pair's fp32 dot product of hw terms errs by at most
    hw 2^-24 |a| |b| (Cauchy-Schwarz; the scaled planes' own roundings are two more terms of that size), divided by
    hw - 1; s adds that over its pairs, and the division and the sum of the nod values round nod + 1 times more."""
    C = r['norms'].shape[2]
    j0, j1 = pair_index(C)
    dots = ((hw + 2) * 2.0 ** -24 * r['norms'][:, :, j0] * r['norms'][:, :, j1]).sum(-1) / (hw - 1)
    return dots + (r['nod'] + 1) * 2.0 ** -24 * r['s']


def fp32_loss_bound(r, hw):
    """Worst case of the fp32 loss against float64 `r`, absolute: the bounds of s of the active groups add up, over
    nod B; the subtraction, the division, the sum of the partials and the final scaling are a few more roundings of the
    result (8 granted)."""
    return (fp32_s_bound(r, hw)[r['active']].sum() / (r['nod'] * r['s'].shape[0])).item() + 8 * 2.0 ** -24 * loss_scale(r)


def saw_restated(feats, W, selected, relax_denom=2.0, table=None):
    """float64 -> dict: loss, grad (feats' shape), s [b, G], corr [b, G, nod] (the upper-triangle covariances), active
    [b, G], signs int8 [b, G, nod], ch, wgh, margin, nod.  table (optional): dict(signs [b, G, nod], active [b, G]) to form
    the gradient with instead of the float64 signs and active bits."""
    return _saw(feats, W, selected, relax_denom, torch.float64, table)


def saw_emulated(feats, W, selected, relax_denom=2.0, table=None):
    """the same in float32: the sigmoid, the scaled planes, the products and the sums"""
    return _saw(feats, W, selected, relax_denom, torch.float32, table)


def saw_differentiable(feats, W, selected, relax_denom=2.0):
    """the same loss written with differentiable operations only, in feats' dtype, connected to feats' graph (W is a
    constant, as in the reference, which reads state_dict())"""
    b, k, h, w = feats.shape
    hw = h * w
    C = len(selected)
    nod = C * (C - 1) // 2
    ch, a = saw_plan(W, selected, k)
    G = ch.shape[0]
    wgh = torch.sigmoid(a).to(feats.dtype)
    xt = feats.reshape(b, k, hw)[:, ch.reshape(-1)].view(b, G, C, hw) * wgh.view(1, G, C, 1)
    cov = xt @ xt.transpose(2, 3) / (hw - 1)
    j0, j1 = pair_index(C)
    s = cov[:, :, j0, j1].abs().sum(-1)
    return torch.clamp((s - saw_margin(C, relax_denom)) / nod, min=0).sum() / b


def pair_band(hw):
    """|corr| below this may take either sign in fp32: an fp32 dot product of hw terms errs by at most
    hw 2^-24 |a| |b| (Cauchy-Schwarz), doubled"""
    return 2.0 * hw * 2.0 ** -24


def group_band(hw, C):
    """the matching band on s - margin: s adds nod pairs"""
    return (C * (C - 1) // 2) * pair_band(hw)


def golden_cases(g):
    """the fixture's cases as dicts: name, feats (b, k, h, w) f32, W (n_cls, k) f32, selected, relax_denom, loss, grad"""
    for name in [str(n) for n in g['names']]:
        q = g[name + '_q']
        yield dict(name=name, feats=torch.from_numpy(q.astype('float32') / 32.0) * float(g[name + '_scale']),
                   W=torch.from_numpy(g[name + '_W']), selected=[int(c) for c in g[name + '_sel']],
                   relax_denom=float(g[name + '_relax']), loss=float(g[name + '_loss'].reshape(-1)[0]),
                   grad=torch.from_numpy(g[name + '_grad']))


def production_inputs(seed=2028, b=8, k=2048, h=32, w=32, n_cls=6, shared=3):
    """-> (feats (b, k, h, w) f32, W (n_cls, k) f32): unit normal noise mixed with `shared` components per image that
    every channel loads on with normal loadings of scale 2 (so that the covariances are not all tiny: at relax_denom 2.0
    about 16 % of the groups are active), instance-normalised per image and channel as the model's `feat` is; W normal of
    scale 2.  The seed: with 2728 groups of which a sixth lies above the margin 7, two to five group sums fall inside the
    guard band of 1.8e-3 around it at most seeds (2023 .. 2030 were looked at), at or above the 0.1 % that may differ; at
    2028 float64 has none there, and 8 of the 40 920 pair covariances inside theirs."""
    gen = torch.Generator().manual_seed(seed)
    z = torch.randn(b, shared, h * w, generator=gen)
    load = torch.randn(k, shared, generator=gen) * 2.0
    x = torch.randn(b, k, h * w, generator=gen) + torch.einsum('kr,brp->bkp', load, z)
    x = (x - x.mean(2, keepdim=True)) / x.var(2, unbiased=False, keepdim=True).add(1e-5).sqrt()
    W = torch.randn(n_cls, k, generator=gen) * 2.0
    return x.view(b, k, h, w).contiguous(), W
