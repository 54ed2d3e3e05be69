"""CoralLoss -- mirror of regda/gast/coral.py::CoralLoss (Deep CORAL, eq. 1 of arXiv:1607.01719) on rgda_coral_loss.

The forward computes the loss and both input gradients in one call (the kernel needs the covariance difference D for
both); backward scales the stored gradients by the incoming one.  The gradients are bf16 (the precision of the
feature gradient the fused steps hand to the instance-norm backward)."""
import torch

from .. import ops
from ._rowsgrad import rows_loss


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
        return rows_loss(lambda s, t, gs, gt: ops.coral_loss(s, t, 1.0, dfeat_s=gs, dfeat_t=gt), source, target)
