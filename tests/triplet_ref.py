"""The batch-hard triplet loss (regda/gast/triple.py::TripletLoss) restated for the tests, on the CPU:

    triplet_restated        the definition in float64 (or fp32) with the closed-form gradient
    triplet_differentiable  the definition on a torch tensor, for autograd
    triplet_on_pairs        the loss with the selection given, for autograd
    triplet_emulated        the arithmetic contract of rgda_triplet_loss (include/rgda_hip.h): bf16 rows and fp32 sums for
                            the mining, the selected distances and the gradient in fp32 from the unrounded rows, bf16
                            gradient rows
    make_inputs, CASES      x = cw * centroid[label] + randn; the shapes the CPU and GPU tests share
    golden_cases            the cases of tests/golden/triplet.npz

Definition: d_ij = sqrt(max(|x_i - x_j|^2, 1e-12)); d_ap(i) = max over j with t_j = t_i (i itself included), d_an(i) =
min over j with t_j != t_i; L = mean over the anchors of max(0, d_ap - d_an + margin).  Rows labelled ignore_label (when
given) are neither anchors nor candidates; an anchor without a negative takes no part (fewer than two distinct labels:
loss 0, gradient 0, m = 0).  Ties go to the lowest index."""
import numpy as np
import torch

CLAMP = 1e-12
F32 = np.float32

# name: (n, k, classes, cw, seed).  cw sets how far the class centroids lie apart in units of the noise: it moves the
# share of positive hinges.  Shares measured in float64: n300_k64 0.51, n512_k2048 0.70; n96_k32 and n8192_k64 all
# active; n130_k96_far none.
CASES = {
    'n96_k32': (96, 32, 3, 0.5, 11),
    'n300_k64': (300, 64, 4, 1.1, 12),
    'n130_k96_far': (130, 96, 3, 3.0, 13),
    'n512_k2048': (512, 2048, 6, 0.4, 14),
    'n8192_k64': (8192, 64, 8, 0.5, 15),
}
GOLDEN_NAMES = ['n96_k32', 'n300_k64', 'n130_k96_far']
MIXED = {'n300_k64', 'n512_k2048'}            # cases meant to mix positive and zero hinges


def make_inputs(n, k, classes, cw, seed):
    """-> (x f32 [n, k], labels int64 [n]); every class has at least two members"""
    gen = torch.Generator().manual_seed(seed)
    labels = torch.randint(0, classes, (n,), generator=gen)
    labels[:2 * classes] = torch.arange(classes).repeat(2)
    centroid = torch.randn(classes, k, generator=gen)
    x = cw * centroid[labels] + torch.randn(n, k, generator=gen)
    return x.float(), labels


def case_inputs(name):
    return make_inputs(*CASES[name])


def variant_cases():
    """name -> (x f32 [n, k], labels, ignore_label): n300_k64 with the edge conditions of the GPU tests"""
    x, lab = case_inputs('n300_k64')
    out = {}
    li = lab.clone()
    li[::7] = -1                                           # ignored rows in every tile
    out['n300_k64_ignore'] = (x, li, -1)
    xd, ld = x.clone(), lab.clone()
    xd[150:160] = xd[0:10]                                 # duplicates of the same class: tied positives
    ld[150:160] = ld[0:10]
    xd[200:205] = xd[20:25]                                # duplicates of another class: d_an below the clamp
    ld[200:205] = (ld[20:25] + 1) % 4
    out['n300_k64_dup'] = (xd, ld, None)
    ls = lab.clone()
    ls[17] = 4                                             # a class of one: its positive is itself
    out['n300_k64_single'] = (x, ls, None)
    return out


def golden_cases(npz):
    for name in [str(s) for s in npz['names']]:
        yield dict(name=name, x=torch.from_numpy(npz[name + '_x']), labels=torch.from_numpy(npz[name + '_labels']),
                   loss=float(npz[name + '_loss']), grad=torch.from_numpy(npz[name + '_grad']),
                   margin=float(npz[name + '_margin']))


def _np(x, dtype):
    return (x.detach().cpu().numpy() if torch.is_tensor(x) else np.asarray(x)).astype(dtype)


def _valid(labels, ignore_label):
    lab = _np(labels, np.int64).reshape(-1)
    ok = np.ones(lab.shape, bool) if ignore_label is None else lab != ignore_label
    return lab, ok


def _mine(d2_rows, lab, ok, block=1024, gaps=False):
    """d2_rows(i0, i1) -> [i1 - i0, n] squared distances.  -> p, q (int64 [n], -1: none) and, with gaps, the distance
    between the best and the second-best candidate of each search (inf where there is no second)."""
    n = lab.shape[0]
    p = np.full(n, -1, np.int64)
    q = np.full(n, -1, np.int64)
    gp = np.full(n, np.inf)
    gq = np.full(n, np.inf)
    for i0 in range(0, n, block):
        i1 = min(i0 + block, n)
        d2 = d2_rows(i0, i1)
        same = (lab[i0:i1, None] == lab[None, :]) & ok[None, :]
        other = (lab[i0:i1, None] != lab[None, :]) & ok[None, :]
        a = np.where(same, d2, -np.inf)
        b = np.where(other, d2, np.inf)
        pi, qi = a.argmax(1), b.argmin(1)                    # numpy: the first occurrence on ties
        rows = ok[i0:i1]
        p[i0:i1] = np.where(rows & same.any(1), pi, -1)
        q[i0:i1] = np.where(rows & other.any(1), qi, -1)
        if gaps and n >= 2:
            top = np.partition(a, n - 2, axis=1)[:, n - 2:].astype(np.float64)
            low = np.partition(b, 1, axis=1)[:, :2].astype(np.float64)
            with np.errstate(invalid='ignore'):
                gp[i0:i1] = np.nan_to_num(top[:, 1] - top[:, 0], nan=np.inf)
                gq[i0:i1] = np.nan_to_num(low[:, 1] - low[:, 0], nan=np.inf)
    return p, q, gp, gq


def _fma(a, b, c):
    """fp32 fused multiply-add: the product of two fp32 values is exact in float64"""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(F32)


def _butterfly(v):
    """v [rows, 64] fp32 -> [rows]: v += v[lane ^ o] for o = 32, 16, .., 1 (the wavefront's xor butterfly)"""
    lane = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[:, lane ^ o]
    return v[:, 0]


def pair_sq(x, i, j, dtype=np.float64):
    """|x_i - x_j|^2 for index vectors i, j.  float64: plainly.  float32: in the kernel's order -- the difference in
    fp32, lane l of 64 accumulates the channels l + 64 t in order with a fused multiply-add, then the butterfly."""
    if dtype == np.float64:
        d = x[i].astype(np.float64) - x[j].astype(np.float64)
        return (d * d).sum(1)
    d = x[i].astype(F32) - x[j].astype(F32)
    rows, k = d.shape
    kp = (k + 63) // 64 * 64
    d = np.concatenate([d, np.zeros((rows, kp - k), F32)], 1).reshape(rows, kp // 64, 64)
    acc = np.zeros((rows, 64), F32)
    for t in range(kp // 64):
        acc = _fma(d[:, t], d[:, t], acc)
    return _butterfly(acc)


def hinge_sum(h):
    """the kernel's sum over the rows: 256 strided fp32 partials, a butterfly per wavefront, (w0 + w1) + (w2 + w3)"""
    n = h.shape[0]
    npad = (n + 255) // 256 * 256
    v = np.concatenate([h.astype(F32), np.zeros(npad - n, F32)]).reshape(npad // 256, 256)
    acc = np.zeros(256, F32)
    for t in range(v.shape[0]):
        acc = acc + v[t]
    w = _butterfly(acc.reshape(4, 64))
    return (w[0] + w[1]) + (w[2] + w[3])


def true_distances(x, lab_ok, direct=None):
    """float64 squared-distance rows of x: the direct sum of squared differences where n^2 k is small (exact zeros and
    exact ties for duplicated rows), else s_i + s_j - 2 G with the diagonal set to 0"""
    x64 = x.astype(np.float64)
    n, k = x64.shape
    if direct is None:
        direct = n * n * k <= 2e8
    if direct:
        return lambda i0, i1: ((x64[i0:i1, None, :] - x64[None, :, :]) ** 2).sum(2)
    s = (x64 * x64).sum(1)

    def rows(i0, i1):
        d2 = s[i0:i1, None] + s[None, :] - 2.0 * (x64[i0:i1] @ x64.T)
        d2[np.arange(i1 - i0), np.arange(i0, i1)] = 0.0
        return np.maximum(d2, 0.0)
    return rows


def _closed_form(x, p, q, margin, weight, dtype):
    """from the selected pairs: loss, gradient, per-row values.  dtype float64: exact; float32: the kernel's order"""
    n, k = x.shape
    has = (p >= 0) & (q >= 0)
    idx = np.nonzero(has)[0]
    m = int(has.sum())
    sp = np.zeros(n)
    sn = np.zeros(n)
    sp[idx] = pair_sq(x, idx, p[idx], dtype)
    sn[idx] = pair_sq(x, idx, q[idx], dtype)
    clamp = dtype(CLAMP)
    sp, sn = sp.astype(dtype), sn.astype(dtype)
    d_ap = np.sqrt(np.maximum(sp, clamp))
    d_an = np.sqrt(np.maximum(sn, clamp))
    hinge = np.where(has, (d_ap - d_an) + dtype(margin), dtype(0)).astype(dtype)
    active = has & (hinge > 0)
    hinge = np.where(active, hinge, dtype(0)).astype(dtype)
    grad = np.zeros((n, k), dtype)
    if m == 0:
        return dict(loss=0.0, grad=grad, p=p, n=q, d_ap=d_ap, d_an=d_an, hinge=hinge, m=0, active=0)
    total = hinge_sum(hinge) if dtype == np.float32 else hinge.sum()
    loss = dtype(weight) * (total / dtype(m))
    c = dtype(weight) / dtype(m)
    use_p = active & (sp >= clamp)
    use_q = active & (sn >= clamp)
    xd = x.astype(dtype)
    with np.errstate(divide='ignore', invalid='ignore'):
        cp = np.where(use_p, c / d_ap, dtype(0)).astype(dtype)
        cq = np.where(use_q, c / d_an, dtype(0)).astype(dtype)
    pc, qc = np.maximum(p, 0), np.maximum(q, 0)
    # the row's own anchor first ...
    fma = _fma if dtype == np.float32 else (lambda a, b, c: a * b + c)
    grad += cp[:, None] * (xd - xd[pc])
    grad = fma(-cq[:, None], xd - xd[qc], grad)
    # ... then the anchors that selected it, in ascending anchor order (every term one fused multiply-add in fp32)
    for i in np.nonzero(active)[0]:
        if use_p[i] and p[i] != i:
            grad[p[i]] = fma(-cp[i:i + 1], xd[i] - xd[p[i]], grad[p[i]])
        if use_q[i]:
            grad[q[i]] = fma(cq[i:i + 1], xd[i] - xd[q[i]], grad[q[i]])
    return dict(loss=float(loss), grad=grad, p=p, n=q, d_ap=d_ap, d_an=d_an, hinge=hinge, m=m, active=int(active.sum()))


def triplet_restated(x, labels, margin=0.3, ignore_label=None, weight=1.0, dtype=np.float64):
    """The definition.  -> dict: loss (float), grad [n, k], p, n (int64, -1: none), d_ap, d_an, hinge, m, active.
    dtype float64: mining on float64 distances; float32: everything in fp32 (the direct form)."""
    xs = _np(x, np.float32)
    lab, ok = _valid(labels, ignore_label)
    if dtype == np.float64:
        rows = true_distances(xs, ok)
    else:
        def rows(i0, i1):
            d = xs[i0:i1, None, :] - xs[None, :, :]
            return (d * d).sum(2, dtype=np.float32)
    p, q, _, _ = _mine(rows, lab, ok)
    return _closed_form(xs, p, q, margin, weight, dtype)


def triplet_differentiable(x, labels, margin=0.3, ignore_label=None):
    """The definition on a torch tensor (any dtype), differentiable; for small n (an (n, n, k) tensor)."""
    lab = labels.reshape(-1)
    ok = torch.ones_like(lab, dtype=torch.bool) if ignore_label is None else lab != ignore_label
    d2 = ((x[:, None, :] - x[None, :, :]) ** 2).sum(2)
    dist = d2.clamp(min=CLAMP).sqrt()
    same = (lab[:, None] == lab[None, :]) & ok[None, :]
    other = (lab[:, None] != lab[None, :]) & ok[None, :]
    anchors = ok & other.any(1)
    if not bool(anchors.any()):
        return (x * 0.0).sum()
    d_ap = torch.where(same, dist, torch.full_like(dist, -float('inf'))).max(1).values
    d_an = torch.where(other, dist, torch.full_like(dist, float('inf'))).min(1).values
    return torch.relu(d_ap[anchors] - d_an[anchors] + margin).mean()


def triplet_on_pairs(x, p, q, margin=0.3):
    """The loss with the selection given: mean over the anchors i with q_i >= 0 of max(0, d(i, p_i) - d(i, q_i) + margin),
    differentiable in x (a torch tensor); p, q integer tensors."""
    idx = torch.nonzero(q >= 0).reshape(-1)
    if idx.numel() == 0:
        return (x * 0.0).sum()
    d_ap = ((x[idx] - x[p[idx].long()]) ** 2).sum(1).clamp(min=CLAMP).sqrt()
    d_an = ((x[idx] - x[q[idx].long()]) ** 2).sum(1).clamp(min=CLAMP).sqrt()
    return torch.relu(d_ap - d_an + margin).mean()


def emulated_mining(x, labels, ignore_label=None):
    """The mining of the contract: Xh = bf16(x); s = fp32 sums of the rounded squares; G fp32; d2 = (s_i + s_j) - 2 G in
    fp32.  The sums are taken in float64 and rounded once: the kernel's fp32 sums differ from that by their order.
    -> p, q, gap_p, gap_q, s"""
    xs = torch.as_tensor(_np(x, np.float32))
    xh = xs.bfloat16().double().numpy()
    lab, ok = _valid(labels, ignore_label)
    s = (xh * xh).sum(1).astype(F32)

    def rows(i0, i1):
        G = (xh[i0:i1] @ xh.T).astype(F32)
        return (s[i0:i1, None] + s[None, :]) - F32(2.0) * G
    p, q, gp, gq = _mine(rows, lab, ok, gaps=True)
    return p, q, gp, gq, s


def triplet_emulated(x, labels, margin=0.3, ignore_label=None, weight=1.0, prior=None):
    """The contract of rgda_triplet_loss.  prior: bf16 rows the gradient is accumulated onto (accumulate = 1).
    -> dict like triplet_restated (loss fp32; grad the bf16 rows as a torch tensor) plus gap_p, gap_n (the emulated d2
    distance between the best and the second-best candidate per row) and s."""
    xs = _np(x, np.float32)
    p, q, gp, gq, s = emulated_mining(xs, labels, ignore_label)
    out = _closed_form(xs, p, q, margin, weight, np.float32)
    g = torch.from_numpy(out['grad'])
    if prior is not None:
        touched = torch.from_numpy(np.abs(out['grad']).sum(1) != 0) if out['m'] else torch.zeros(len(p), dtype=torch.bool)
        g = torch.where(touched[:, None], g + prior.float(), prior.float())
    out['grad'] = g.bfloat16()
    out.update(gap_p=gp, gap_n=gq, s=s)
    return out


def mining_deviation(x, p, q, ref):
    """The largest relative distance between the true (float64, direct) distance of the selection (p, q) and the true
    extremum of `ref` (a triplet_restated result), over the rows that have both."""
    xs = _np(x, np.float32)
    idx = np.nonzero((ref['p'] >= 0) & (ref['n'] >= 0))[0]
    if not len(idx):
        return 0.0
    assert (p[idx] >= 0).all() and (q[idx] >= 0).all()
    dp = np.sqrt(np.maximum(pair_sq(xs, idx, p[idx]), CLAMP))
    dq = np.sqrt(np.maximum(pair_sq(xs, idx, q[idx]), CLAMP))
    tp = np.sqrt(np.maximum(pair_sq(xs, idx, ref['p'][idx]), CLAMP))
    tq = np.sqrt(np.maximum(pair_sq(xs, idx, ref['n'][idx]), CLAMP))
    return float(max((np.abs(dp - tp) / tp).max(), (np.abs(dq - tq) / tq).max()))
