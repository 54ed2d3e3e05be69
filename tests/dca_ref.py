"""Deep Covariance Alignment (regda/dca_modules.py: CategoryAlign_Module, ICR, CCR, MSE_intra, MSE_cross) restated for
the tests, on the CPU:

    dca_differentiable  the definition as the reference writes it, on torch tensors, for autograd
    dca_restated        the definition with the closed-form gradient (float64, or fp32 for the reference's own noise)
    dca_emulated        the arithmetic contract of rgda_dca_loss (include/rgda_hip.h): fp32 softmax, fp32 sums over the
                        pixels in a sequential order, fp32 tail, bf16 gradient rows (`prior` for accumulate)
    make_inputs, CASES  structured inputs and the shapes the CPU and GPU tests share
    golden_cases        the cases of tests/golden/dca.npz

A side is (feat (b, c, h, w), preds): preds a tuple of one or two (b, C, h, w) maps read according to pred_kind ('prob':
probabilities as given, 'logits': softmax, 'logits2': the mean of two softmaxes).  The definition:

    Z[b,k] = sum_p P[b,k,p];  v[b,k,:] = sum_p feat[b,:,p] P[b,k,p] / Z[b,k];  ignore_bg drops class 0 (n = C - 1)
    u[b,k,c] = v[b,k,c] / max(sqrt(sum_k' v[b,k',c]^2), 1e-12)        (F.normalize over the CLASS axis)
    cov: R[i,j] = pearson(mean_b u_a[i,:], mean_b u_b[j,:]);  L = -mean_i log R_ii - mean_{i!=j} log(1 - max(R_ij, 1e-6))
    mse: L = mean (u_a - u_b)^2

Unstructured inputs (randn features and logits) give a negative diagonal and a NaN loss, so make_inputs builds a pixel
label map in which every class occurs, feat = cw * centroid[label] + randn and logits = sharp * onehot(label) + randn;
cov_conditions states what every cov case then satisfies in float64."""
import numpy as np
import torch

EPS = 1e-12
LOW = 1e-6

# name: (images per side, C, c, h, w, cw, sharp, seed) -- the table of the GPU tests
CASES = {
    'b2_k6_c32_5x7': (2, 6, 32, 5, 7, 1.0, 3.0, 41),
    'b4_k7_c96_9x9': (4, 7, 96, 9, 9, 1.0, 3.0, 42),
    'b2_k16_c64_8x8': (2, 16, 64, 8, 8, 1.0, 3.0, 43),
    'b2_k6_c64_33x33': (2, 6, 64, 33, 33, 1.0, 3.0, 44),
    'b4_k6_c2048_16x16': (4, 6, 2048, 16, 16, 0.5, 2.0, 45),
}
GOLDEN_NAMES = ['b2_k6_c32_5x7', 'b4_k7_c96_9x9']


def make_inputs(b, C, c, h, w, cw=1.0, sharp=3.0, seed=0, b_b=None):
    """-> ((feat_a, (l1_a, l2_a)), (feat_b, (l1_b, l2_b))): two sides of b (and b_b) images that share the class
    centroids; every class occurs in every image"""
    gen = torch.Generator().manual_seed(seed)
    centroid = torch.randn(C, c, generator=gen)
    sides = []
    for bs in (b, b if b_b is None else b_b):
        lab = torch.randint(0, C, (bs, h * w), generator=gen)
        lab[:, :C] = torch.arange(C)
        lab = lab[:, torch.randperm(h * w, generator=gen)]
        feat = cw * centroid[lab].permute(0, 2, 1) + torch.randn(bs, c, h * w, generator=gen)
        onehot = torch.nn.functional.one_hot(lab, C).permute(0, 2, 1).float()
        l1 = sharp * onehot + torch.randn(bs, C, h * w, generator=gen)
        l2 = sharp * onehot + torch.randn(bs, C, h * w, generator=gen)
        sides.append((feat.view(bs, c, h, w).contiguous(), (l1.view(bs, C, h, w).contiguous(), l2.view(bs, C, h, w).contiguous())))
    return tuple(sides)


def case_inputs(name):
    return make_inputs(*CASES[name])


def random_inputs(b, C, c, h, w, seed):
    """unstructured inputs: the correlation matrix has a negative diagonal entry and the cov loss is NaN"""
    gen = torch.Generator().manual_seed(seed)
    return tuple((torch.randn(b, c, h, w, generator=gen), (torch.randn(b, C, h, w, generator=gen), torch.randn(b, C, h, w, generator=gen)))
                 for _ in range(2))


def golden_cases(npz):
    for name in [str(s) for s in npz['names']]:
        g = {k[len(name) + 1:]: npz[k] for k in npz.files if k.startswith(name + '_')}
        yield name, g


def probs(preds, pred_kind, dtype=torch.float64):
    """-> P (b, C, hw) in dtype"""
    preds = tuple(p.to(dtype).flatten(2) for p in preds)
    if pred_kind == 'prob':
        return preds[0]
    if pred_kind == 'logits':
        return preds[0].softmax(1)
    assert pred_kind == 'logits2'
    return (preds[0].softmax(1) + preds[1].softmax(1)) / 2


# ---------------------------------------------------------------- the definition as the reference writes it
def _pearson(x, y):
    """audtorch.metrics.functional.pearsonr as published: the centred product sum over c - 1, divided by the product of
    the two unbiased standard deviations"""
    xc, yc = x - x.mean(), y - y.mean()
    return (xc * yc).sum() / (x.numel() - 1) / (x.std(unbiased=True) * y.std(unbiased=True))


def _get_context(P, feat, ignore_bg):
    b, c = feat.shape[:2]
    v = (feat.reshape(b, 1, c, -1) * P.reshape(b, P.shape[1], 1, -1)).sum(-1) / P.reshape(b, P.shape[1], 1, -1).sum(-1)
    if ignore_bg:
        v = v[:, 1:, :]
    return torch.nn.functional.normalize(v, dim=1)


def dca_differentiable(feat_a, P_a, feat_b, P_b, kind='cov', ignore_bg=True):
    """feat_* (b, c, h, w) tensors (any dtype, may require grad), P_* (b, C, hw) constants -> the scalar loss"""
    ua, ub = _get_context(P_a, feat_a, ignore_bg), _get_context(P_b, feat_b, ignore_bg)
    if kind == 'mse':
        return torch.nn.functional.mse_loss(ua, ub, reduction='mean')
    ma, mb = ua.mean(0), ub.mean(0)
    n = ma.shape[0]
    R = torch.stack([torch.stack([_pearson(ma[i], mb[j]) for j in range(n)]) for i in range(n)])
    pos = -torch.log(torch.diag(R)).mean()
    undiag = R.flatten()[:-1].view(n - 1, n + 1)[:, 1:].flatten()
    neg = -torch.log(1 - undiag.max(torch.tensor([LOW], dtype=R.dtype))).mean()
    return pos + neg


# ---------------------------------------------------------------- closed form
def _seq_sums(feat, P, reverse):
    """S[b,k,c] = sum_p P feat and Z, added pixel after pixel in the working precision (descending with reverse)"""
    b, c, hw = feat.shape
    S = torch.zeros(b, P.shape[1], c, dtype=feat.dtype)
    Z = torch.zeros(b, P.shape[1], dtype=feat.dtype)
    for p in (range(hw - 1, -1, -1) if reverse else range(hw)):
        S = S + P[:, :, p, None] * feat[:, None, :, p]
        Z = Z + P[:, :, p]
    return S, Z


def _context(feat, P, ignore_bg, seq=None):
    feat = feat.flatten(2)
    if seq is None:
        S, Z = torch.einsum('bkp,bcp->bkc', P, feat), P.sum(-1)
    else:
        S, Z = _seq_sums(feat, P, seq)
    v = S / Z[..., None]
    if ignore_bg:
        v = v[:, 1:]
    N = v.pow(2).sum(1, keepdim=True).sqrt()
    return dict(Z=Z, v=v, N=N, u=v / N.clamp(min=EPS), T=torch.einsum('bkp,bcp->bkc', P, feat.abs()) / Z[..., None])


def _back(gu, ctx, P, ignore_bg):
    """dL/du (b, n, c) -> (G (b, C, c), dL/dfeat as pixel-major rows (b * hw, c))"""
    u, N, Z = ctx['u'], ctx['N'], ctx['Z']
    k0 = 1 if ignore_bg else 0
    dot = (gu * u).sum(1, keepdim=True)
    gv = torch.where(N >= EPS, (gu - u * dot) / N.clamp(min=EPS), gu / EPS)
    G = gv / Z[:, k0:, None]
    if ignore_bg:
        G = torch.cat([torch.zeros_like(G[:, :1]), G], 1)
    rows = torch.einsum('bkp,bkc->bpc', P, G).reshape(-1, G.shape[2])
    return G, rows


def _flip(x, on):
    return x.flip(-1) if on else x


def _closed_form(sides, pred_kind, kind, ignore_bg, dtype, seq=None):
    (fa, pa), (fb, pb) = sides
    Pa, Pb = probs(pa, pred_kind, dtype), probs(pb, pred_kind, dtype)
    ca, cb = _context(fa.to(dtype), Pa, ignore_bg, seq), _context(fb.to(dtype), Pb, ignore_bg, seq)
    ua, ub = ca['u'], cb['u']
    out = dict(u_a=ua, u_b=ub, v_a=ca['v'], v_b=cb['v'], Z_a=ca['Z'], Z_b=cb['Z'], T_a=ca['T'], T_b=cb['T'])
    fl = bool(seq)                    # the second order also adds the channels the other way round
    if kind == 'mse':
        assert ua.shape == ub.shape
        d = ua - ub
        loss = _flip(d.pow(2).flatten(), fl).sum() / d.numel()
        gua, gub = 2 * d / d.numel(), -2 * d / d.numel()
    else:
        ma, mb = ua.sum(0) / ua.shape[0], ub.sum(0) / ub.shape[0]
        n, c = ma.shape
        ac = ma - (_flip(ma, fl).sum(1) / c)[:, None]
        bc = mb - (_flip(mb, fl).sum(1) / c)[:, None]
        sa, sb = _flip(ac.pow(2), fl).sum(1), _flip(bc.pow(2), fl).sum(1)
        den = sa.sqrt()[:, None] * sb.sqrt()[None, :]
        R = (_flip(ac, fl) @ _flip(bc, fl).t()) / den
        eye = torch.eye(n, dtype=torch.bool)
        nn = n * (n - 1)
        with np.errstate(all='ignore'):
            terms = torch.where(eye, -torch.log(R) / n, -torch.log(1 - R.clamp(min=LOW)) / nn)
        loss = terms.sum()
        W = torch.where(eye, -1 / (n * R), torch.where(R > LOW, 1 / (nn * (1 - R)), torch.zeros_like(R)))
        dma = (W / den) @ bc - ((W * R).sum(1) / sa)[:, None] * ac
        dmb = (W / den).t() @ ac - ((W * R).sum(0) / sb)[:, None] * bc
        gua = (dma / ua.shape[0])[None].expand_as(ua)
        gub = (dmb / ub.shape[0])[None].expand_as(ub)
        out.update(R=R, W=W)
    out['G_a'], out['rows_a'] = _back(gua, ca, Pa, ignore_bg)
    out['G_b'], out['rows_b'] = _back(gub, cb, Pb, ignore_bg)
    out.update(loss=float(loss), gu_a=gua, gu_b=gub)
    return out


def dca_restated(sides, pred_kind='logits2', kind='cov', ignore_bg=True, dtype=torch.float64):
    """-> dict: loss (float), u_a / u_b (b, n, c), v_*, Z_*, R and W = dL/dR (cov), rows_a / rows_b = dL/dfeat as
    pixel-major rows (b * hw, c) of BOTH sides (CCR / MSE_cross use rows_b only), T_* = sum_p |feat| P / Z"""
    return _closed_form(sides, pred_kind, kind, ignore_bg, dtype)


def dca_emulated(sides, pred_kind='logits2', kind='cov', ignore_bg=True, weight=1.0, prior=(None, None), reverse=False):
    """The contract in fp32: softmax and every sum in fp32, the sums over the pixels added one pixel after the other
    (ascending; descending, and the channel sums flipped, with reverse: the second summation order the tight bounds of the
    GPU test are measured with), weight * dL/dfeat rounded once to bf16, a prior row added in fp32 before the rounding.
    -> the dict of dca_restated in fp32 plus grad_a / grad_b: bf16 rows, and rows_* scaled by weight."""
    out = _closed_form(sides, pred_kind, kind, ignore_bg, torch.float32, seq=bool(reverse))
    out['loss'] = float(np.float32(weight) * np.float32(out['loss']))
    for s, pr in zip('ab', prior):
        rows = np.float32(weight) * out['rows_' + s]
        out['rows_' + s] = rows
        out['grad_' + s] = (rows if pr is None else rows + pr.float()).bfloat16()
    return out


def cov_conditions(R):
    """-> (min diagonal, max off-diagonal, the least distance of an off-diagonal entry from the 1e-6 switch, the share of
    clamped off-diagonal entries) of a float64 correlation matrix"""
    R = R.double()
    n = R.shape[0]
    eye = torch.eye(n, dtype=torch.bool)
    off = R[~eye]
    return float(R.diag().min()), float(off.max()), float((off - LOW).abs().min()), float((off <= LOW).float().mean())


def check_cov_conditions(R, who=''):
    dmin, omax, gap, share = cov_conditions(R)
    assert dmin >= 0.5 and omax <= 0.9 and gap >= 1e-4, (who, dmin, omax, gap)
    return dmin, omax, gap, share


def relnorm(got, ref):
    got, ref = torch.as_tensor(got).double(), torch.as_tensor(ref).double()
    n = ref.norm().item()
    d = (got - ref).norm().item()
    return d / n if n else d
