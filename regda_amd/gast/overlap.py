"""Region-overlap losses (Dice; soft Jaccard; Tversky, Salehi et al. 2017; focal-Tversky, Abraham & Khan 2019) as loss
modules over the fused kernels (`rgda_upsample_overlap`, include/rgda_hip.h): the bilinear upsample of the logits, the
softmax and the three sums per class happen in one row pass, the gradient in a second one; no b x C x H x W tensor is
ever written.  The sums run over the valid pixels of the whole batch (of this rank, in a data-parallel run).
"""
import torch

from .. import ops


class _OverlapTerm(torch.autograd.Function):
    @staticmethod
    def forward(ctx, p1, p2, label, mod):
        heads = 1 if p2 is None else 2
        a = p1.detach()
        b = a if heads == 1 else p2.detach()
        want = ctx.needs_input_grad[0] or (heads == 2 and ctx.needs_input_grad[1])
        loss, index, present, g1, g2 = ops.upsample_overlap(a, b, label, mod.alpha, mod.beta, mod.gamma, mod.smooth,
                                                            heads=heads, ignore_label=mod.ignore_label, want_grad=want,
                                                            flag=mod.flag)
        mod.index, mod.present = index, present
        if want and heads == 1:
            ctx.grads = (g1.add_(g2).to(p1.dtype), None)
        elif want:
            ctx.grads = (g1.to(p1.dtype), g2.to(p2.dtype))
        return loss[0].clone()

    @staticmethod
    def backward(ctx, grad_out):
        g1, g2 = ctx.grads
        return grad_out * g1, None if g2 is None else grad_out * g2, None, None


class TverskyLoss(torch.nn.Module):
    """forward(preds, labels) -> the term (a scalar, differentiable in the logits).  preds: one logit tensor (b, c, h, w)
    or a list of two heads (the term is then the mean over the heads), at the labels' resolution or below it (upsampled
    bilinearly, align_corners=True); labels: int64 (b, H, W), `ignore_label` = no pixel.  With TP, FP, FN the soft counts
    of a class over the valid pixels of the batch, T = (TP + smooth) / (TP + smooth + alpha FP + beta FN + 1e-7) and the
    loss is the mean of (1 - T)^gamma over the classes that occur in the labels; 1 <= gamma <= 8.  After a call `index`
    (f32 [heads, c], T per class, 0 for an absent class) and `present` (int32 [c], the class's valid pixels) stay on the
    device; `flag_value()` is the deferred check of the labels' range."""

    def __init__(self, alpha, beta, gamma=1.0, smooth=0.0, ignore_label=-1):
        super().__init__()
        self.alpha, self.beta, self.gamma, self.smooth = ops.overlap_params(alpha, beta, gamma, smooth, type(self).__name__)
        self.ignore_label = int(ignore_label)
        self.flag = None
        self.index = self.present = None

    def forward(self, preds, labels):
        heads = list(preds) if isinstance(preds, (list, tuple)) else [preds]
        if len(heads) not in (1, 2):
            raise ValueError(f'{type(self).__name__}: {len(heads)} predictions; one tensor or a list of two')
        ops._need_cuda(*heads, labels)
        if self.flag is None or self.flag.device != heads[0].device:
            self.flag = torch.zeros(1, dtype=torch.int32, device=heads[0].device)
        return _OverlapTerm.apply(heads[0], heads[1] if len(heads) == 2 else None, labels, self)

    def flag_value(self):
        """Deferred check (host sync): bit 0 = a label outside [0, c) that is not ignore_label was treated as ignored."""
        return 0 if self.flag is None else int(self.flag.item())


class DiceLoss(TverskyLoss):
    """1 - 2 TP / (2 TP + FP + FN) per class: TverskyLoss(0.5, 0.5)."""

    def __init__(self, gamma=1.0, smooth=0.0, ignore_label=-1):
        super().__init__(0.5, 0.5, gamma, smooth, ignore_label)


class JaccardLoss(TverskyLoss):
    """1 - TP / (TP + FP + FN) per class, the soft IoU: TverskyLoss(1, 1)."""

    def __init__(self, gamma=1.0, smooth=0.0, ignore_label=-1):
        super().__init__(1.0, 1.0, gamma, smooth, ignore_label)
