"""CoralLoss -- mirror of regda/gast/coral.py::CoralLoss (Deep CORAL, eq. 1 of arXiv:1607.01719) on rgda_coral_loss.

The forward computes the loss and both input gradients in one call (the kernel needs the covariance difference D for
both); backward scales the stored gradients by the incoming one.  The gradients are bf16 (the precision of the
feature gradient the fused steps hand to the instance-norm backward)."""
import torch

from .. import ops


def _rows(x):
    """(n, d) rows, or the pixels of an NCHW (b, d, h, w) map: -> (row count, d)"""
    return (x.shape[0], x.shape[1]) if x.dim() == 2 else (x.shape[0] * x.shape[2] * x.shape[3], x.shape[1])


def _as_input(g, shape):
    """pixel-major bf16 rows -> f32 in the input's shape"""
    if len(shape) == 2:
        return g.float()
    b, d, h, w = shape
    return g.float().view(b, h, w, d).permute(0, 3, 1, 2)


class _Coral(torch.autograd.Function):
    @staticmethod
    def forward(ctx, source, target):
        want = ctx.needs_input_grad
        gs = torch.empty(_rows(source), dtype=torch.bfloat16, device=source.device) if want[0] else None
        gt = torch.empty(_rows(target), dtype=torch.bfloat16, device=target.device) if want[1] else None
        loss = ops.coral_loss(source.detach(), target.detach(), 1.0, dfeat_s=gs, dfeat_t=gt)
        ctx.save_for_backward(gs, gt)
        ctx.shapes = (source.shape, target.shape)
        return loss.view(())

    @staticmethod
    def backward(ctx, g):
        gs, gt = ctx.saved_tensors
        ss, ts = ctx.shapes
        return (None if gs is None else g * _as_input(gs, ss), None if gt is None else g * _as_input(gt, ts))


class CoralLoss(torch.nn.Module):
    def __init__(self, is_sqrt=False):
        super().__init__()
        if is_sqrt:
            raise NotImplementedError('CoralLoss(is_sqrt=True) is not provided (the reference recipe uses is_sqrt=False)')
        self.is_sqrt = is_sqrt

    def forward(self, source, target):
        """source (ns, d), target (nt, d) -> the scalar sum((Cs - Ct)^2) / (4 d^2).  NCHW (b, d, h, w) maps are taken
        too (their pixels are the rows: what Aligner.align_domain hands over, without the permuted copy)."""
        assert source.dim() == target.dim() and source.dim() in (2, 4) and source.shape[1] == target.shape[1]
        return _Coral.apply(source, target)
