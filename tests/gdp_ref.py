"""CPU restatement of GDPLoss (regda/gast/balance.py:218-303) and Aligner.get_prototype_weight_4pixel
(regda/gast/alignment.py:267-281), written from their formulas in torch so that autograd gives the gradients.  Pinned to
the reference's own classes by tests/golden/gdp.npz (tests/test_gdp_cpu.py); the GPU tests compare the fused kernels
(rgda_upsample_gdp, rgda_proto_pixel_weight) against it.

Every loss function takes ONE prediction already at the label size; loss_calc upsamples and averages the heads."""
import torch
import torch.nn.functional as F

from loss_ref import GHM_EDGES, _ce, ghm_g, up

BINS = 30


class BalanceState:
    """ClassBalance (balance.py:15-67): the frequency EMA and the per-class weight, updated once per loss call."""

    def __init__(self, class_num, ignore_label=-1, decay=0.99, temperature=0.5, freq=None):
        self.c, self.ig, self.decay, self.temp = class_num, ignore_label, decay, temperature
        self.freq = torch.ones(class_num) / class_num if freq is None else freq.clone().float()

    def class_weight(self):
        p = torch.softmax((1.0 - self.freq) / self.temp, 0)
        return p / (p.max() + 1e-7)

    def pixel_weight(self, label):
        lab = label.reshape(-1)
        valid = lab != self.ig
        cnt = torch.bincount(lab[valid], minlength=self.c).to(self.freq.dtype)
        local = cnt / (valid.to(self.freq.dtype).sum() + 1e-7)
        self.freq = (1.0 - self.decay) * local + self.decay * self.freq
        w = self.class_weight()
        return torch.where(valid, w[lab.clamp(min=0)], torch.zeros((), dtype=w.dtype))


class GdpState:
    """acc_sum / bins_weight of GDPLoss: acc_sum persists across calls, both are updated once per call."""

    def __init__(self, momentum=0.99, dtype=torch.float32):
        self.momentum = momentum
        self.acc_sum = torch.zeros(BINS, dtype=dtype)
        self.bins_weight = None


def bins_weight(acc_sum):
    """_get_dense_weight's per-bin half (balance.py:290-295)."""
    b = 1 - acc_sum / (acc_sum.sum() + 1e-7)
    b = torch.where(acc_sum != 0, b, torch.zeros_like(b))
    return b / (b.max() + 1e-7)


def gdp(p, label, state, ig=-1, proto_weight=None, class_weight=None):
    """One GDPLoss.forward call.  proto_weight / class_weight: per-pixel weights [b*H*W] or None (prototype_refine /
    class_balance off)."""
    g = ghm_g(p, label, ig)
    inr = (g >= 0) & (g <= 1)
    bins = torch.bincount((g[inr] * BINS).floor().long().clamp(max=BINS - 1), minlength=BINS).to(g.dtype)  # histc
    bins = (bins + bins.flip(0)) * 0.5
    ind = (GHM_EDGES.to(g.dtype)[None, :] < g[:, None]).sum(1)                    # bucketize, right=False
    m = state.momentum
    state.acc_sum = m * state.acc_sum + (1 - m) * bins if m > 0 else bins
    state.bins_weight = bw = bins_weight(state.acc_sum)
    w = torch.where((ind > 0) & (ind <= BINS), bw[(ind - 1).clamp(0, BINS - 1)], torch.zeros_like(g))
    terms = 1.0
    if proto_weight is not None:
        w, terms = w + proto_weight.to(w.dtype), terms + 1
    if class_weight is not None:
        w, terms = w + class_weight.to(w.dtype), terms + 1
    lab = label.reshape(-1)
    return (_ce(p, label, ig) * w.detach() / terms).sum() / ((lab != -1).sum() + 1e-7)


def loss_calc(preds, label, state, ig=-1, proto_weight=None, balancer=None):
    """tools.py:240-254 with a GDPLoss: upsample each head, one call per head (head 1 first: acc_sum and the balancer
    advance per call), mean.  A single tensor is one call."""
    single = not isinstance(preds, (list, tuple))
    total = 0
    for p in ([preds] if single else preds):
        cw = balancer.pixel_weight(label) if balancer is not None else None
        total = total + gdp(up(p, label.shape[-2:]), label.long(), state, ig, proto_weight, cw)
    return total if single else total / len(preds)


def pearson_sim(feat, protos):
    """1 / _pearson_dist (alignment.py:396-423) at (b, c, h, w)."""
    b, k, h, w = feat.shape
    f = feat.permute(0, 2, 3, 1).reshape(-1, k)
    fc = f - f.mean(-1, keepdim=True)
    pc = protos - protos.mean(-1, keepdim=True)
    cov = fc @ pc.t() / (k - 1 + 1e-7)
    dist = (-1.0 * cov / (fc.std(-1, keepdim=True) @ pc.std(-1, keepdim=True).t() + 1e-7) + 1.0) * 0.5
    return (1.0 / dist).reshape(b, h, w, -1).permute(0, 3, 1, 2)


def proto_weight_from_sim(sim, label, ig=-1):
    s = F.interpolate(sim, size=label.shape[-2:], mode='bilinear', align_corners=True)
    s = torch.softmax(s, 1)
    s = s / (s.max(1, keepdim=True)[0] + 1e-7)
    pick = s.gather(1, label.clamp(min=0)[:, None])[:, 0]
    return torch.where(label == ig, torch.zeros_like(pick), pick).reshape(-1)


def proto_weight(feat, protos, label, ig=-1):
    """Aligner.get_prototype_weight_4pixel: flat [b*H*W], in the dtype of `feat`."""
    return proto_weight_from_sim(pearson_sim(feat, protos), label, ig)
