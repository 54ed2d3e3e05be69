"""CPU restatement of IAST (regda/utils/tools.py:323-398): entropyloss / kldloss written from their formulas in torch so
that autograd gives the gradients in fp32 or fp64, and the instance-adaptive selector in numpy, written from its arithmetic.
Pinned to the reference's own functions by tests/golden/iast.npz (tests/test_iast_cpu.py); the GPU tests compare the
kernels (rgda_upsample_reg, rgda_iast_*) against it."""
import numpy as np
import torch

from loss_ref import up

BINS = 0x7C01       # the non-negative fp16 bit patterns 0 .. 0x7C00


# ------------------------------------------------------------------------------------------ regularisers (:376-398)
def _w4(weight):
    return weight if weight.dim() == 4 else weight[:, None]


def entropyloss(logits, weight):
    val_num = int((weight > 0).sum())
    ls = torch.log_softmax(logits, dim=1)
    return torch.sum(-torch.softmax(logits, dim=1) * _w4(weight) * ls) / val_num


def kldloss(logits, weight):
    val_num = int((weight > 0).sum())
    ls = torch.log_softmax(logits, dim=1)
    return torch.sum(-1 / logits.shape[1] * _w4(weight) * ls) / val_num


def derived_weights(label, ig=-1, dtype=torch.float32):
    """IAST's regions from a label map: entropy on the ignored pixels, KLD on the labelled ones."""
    return (label == ig).to(dtype), (label != ig).to(dtype)


def reg(preds, size, w_ent, w_kld, lambda_ent=1.0, lambda_kld=1.0, empty_is_zero=False):
    """rgda_upsample_reg's contract on a list of one or two predictions: -> (ent, kld, objective) with ent / kld the
    means over the heads and objective = mean over the heads of lambda_ent * ent_h + lambda_kld * kld_h, whose autograd
    gradient is what the kernel writes.  w_ent / w_kld None: the term is off (0)."""
    zero = torch.zeros((), dtype=preds[0].dtype)
    ents, klds = [], []
    for p in preds:
        z = up(p, tuple(size))
        for w, fn, acc in ((w_ent, entropyloss, ents), (w_kld, kldloss, klds)):
            if w is None or (empty_is_zero and int((w > 0).sum()) == 0):
                acc.append(zero)
            else:
                acc.append(fn(z, w.to(z.dtype)))
    ent, kld = sum(ents) / len(preds), sum(klds) / len(preds)
    return ent, kld, lambda_ent * ent + lambda_kld * kld


# ------------------------------------------------------------------------------------------ selector (:323-373)
def hist(probs):
    """probs (n, C, H, W) f32 -> (arg uint8 (n, H, W): the first maximum, maxp f32, hist int32 [C, BINS] of maxp as fp16)."""
    arg = np.argmax(probs, axis=1)
    maxp = np.max(probs, axis=1)
    bits = maxp.astype(np.float16).view(np.uint16)
    h = np.zeros((probs.shape[1], BINS), np.int64)
    np.add.at(h, (arg.reshape(-1), bits.reshape(-1).astype(np.int64)), 1)
    return arg.astype(np.uint8), maxp, h.astype(np.int32)


def class_thresholds(prepend, confs, alpha, gamma):
    """IAST's per-class candidate thresholds: for class c the p-th percentile, p = 100 (1 - alpha T_c ** gamma), of the
    sample made of the running threshold T_c = prepend[c] followed by the class's fp16 confidences confs[c], taken in
    float64 and stored as float32.  A class without confidences gets T_c back."""
    out = np.empty(len(confs), np.float32)
    for c, conf in enumerate(confs):
        sample = np.concatenate([prepend[c:c + 1], conf.astype(np.float64)])
        out[c] = np.percentile(sample, 100 * (1 - alpha * prepend[c] ** gamma))
    return out


def percentile_from_hist(h, prepend, q):
    """One class: np.quantile([prepend] + the fp16 values the histogram row `h` counts (as f64), q) as f32 -- what
    np.percentile(arr, p) evaluates once it has divided p by 100, so q = p / 100 gives np.percentile's bits."""
    vals = np.arange(BINS, dtype=np.uint16).view(np.float16).astype(np.float64)
    arr = np.concatenate([[prepend], np.repeat(vals, h)])
    return np.float32(np.quantile(arr, q))


class Selector:
    """The instance-adaptive selector, one batch at a time: candidate thresholds from the batch's confidences, an
    exponential moving average with weight `beta` on the old value (the candidate's share is formed in float32, the
    sum in float64), thresholds that reach 1 reset to 0.999, then the labels.  `thresholds(prepend, confs)` replaces
    class_thresholds (the minting script puts the reference's own function there)."""

    def __init__(self, n_class, pl_alpha, pl_beta, pl_gamma, thresholds=None):
        self.n_class, self.alpha, self.beta, self.gamma = n_class, pl_alpha, pl_beta, pl_gamma
        self.cls_thresh = np.full(n_class, 0.9)
        self.tmp = None
        self.thresholds = thresholds or (lambda prepend, confs: class_thresholds(prepend, confs, self.alpha, self.gamma))

    def update(self, probs):
        arg, maxp = np.argmax(probs, axis=1), np.max(probs, axis=1)
        confs = [maxp[arg == c].astype(np.float16) for c in range(self.n_class)]
        self.tmp = self.thresholds(self.cls_thresh, confs)
        moved = self.beta * self.cls_thresh + (1 - self.beta) * self.tmp
        self.cls_thresh = np.where(moved >= 1, 0.999, moved)
        return label_from(arg, maxp, self.cls_thresh)


def label_from(arg, maxp, cls_thresh):
    label = arg.astype(np.int64) + 1
    label[maxp < cls_thresh[arg]] = 0
    return label.astype(np.uint8)


# ------------------------------------------------------------------------------------------ selector inputs
def selector_inputs(kind, n, C, H, W, seed=0):
    """Probabilities (n, C, H, W) f32 in [0, 1] for the stage tests."""
    rng = np.random.default_rng(seed)
    if kind == 'softmax':
        z = rng.standard_normal((n, C, H, W)) * 3
        e = np.exp(z - z.max(1, keepdims=True))
        return (e / e.sum(1, keepdims=True)).astype(np.float32)
    if kind == 'confident':         # every pixel exactly 1.0 in one class
        p = np.zeros((n, C, H, W), np.float32)
        cls = rng.integers(0, C, (n, H, W))
        np.put_along_axis(p, cls[:, None], 1.0, axis=1)
        return p
    if kind == 'fp16_ties':         # maxima half-way between neighbouring fp16 values, and one ulp either side of that
        h16 = rng.integers(0x3000, 0x3BFF, (n, H, W)).astype(np.uint16)
        lo = h16.view(np.float16).astype(np.float32)
        hi = (h16 + 1).astype(np.uint16).view(np.float16).astype(np.float32)
        mid = (lo + hi) / 2         # exact in f32
        step = rng.integers(-1, 2, (n, H, W)).astype(np.int32)
        mx = (mid.view(np.int32) + step).view(np.float32)
        p = np.zeros((n, C, H, W), np.float32)
        cls = rng.integers(0, C, (n, H, W))
        np.put_along_axis(p, cls[:, None], mx[:, None], axis=1)
        return p
    if kind == 'missing_class':     # class 1 never wins
        p = selector_inputs('softmax', n, C, H, W, seed)
        p[:, 1] = 0.0
        return p
    if kind == 'class_ties':        # two (or all) classes share the maximum exactly: the first one wins
        p = selector_inputs('softmax', n, C, H, W, seed)
        mx = p.max(1, keepdims=True)
        other = rng.integers(0, C, (n, 1, H, W))
        np.put_along_axis(p, other, mx, axis=1)
        p[:, :, 0, :] = 0.25
        return p
    raise KeyError(kind)
