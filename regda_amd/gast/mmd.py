"""MMDLoss -- mirror of regda/gast/mmd.py::MMDLoss (multi-kernel RBF maximum mean discrepancy, and the linear form) on
rgda_mmd_loss.

Only the bandwidth is detached in the reference (`l2_distance.data`, mmd.py:34): the pairwise distances are
differentiable, so the loss trains the features.  The forward computes the loss and both input gradients in one call
(the kernel needs the pair weights for both); backward scales the stored gradients by the incoming one.  The gradients
are bf16 (the precision of the feature gradient the fused steps hand to the instance-norm backward).  The reference
forms an (n, n, d) tensor; the kernel works from the Gram product and serves up to n = 32768 rows."""
import torch

from .. import ops
from ._rowsgrad import rows_loss


class MMDLoss(torch.nn.Module):
    def __init__(self, kernel_type='rbf', kernel_mul=2.0, kernel_num=5, fix_sigma=None, **kwargs):
        super().__init__()
        if kernel_type not in ops.MMD_KERNEL_TYPES:
            raise ValueError(f"MMDLoss: kernel_type {kernel_type!r}; served are 'rbf' and 'linear'")
        self.kernel_num = kernel_num
        self.kernel_mul = kernel_mul
        self.fix_sigma = fix_sigma
        self.kernel_type = kernel_type
        self.ext_params = kwargs

    def forward(self, source, target):
        """source (ns, d), target (nt, d) -> the scalar MMD (mmd.py:46-58); ns != nt is served.  NCHW (b, d, h, w) maps
        are taken too (their pixels are the rows, without the permuted copy)."""
        assert source.dim() == target.dim() and source.dim() in (2, 4) and source.shape[1] == target.shape[1]
        return rows_loss(lambda s, t, gs, gt: ops.mmd_loss(s, t, 1.0, self.kernel_type, self.kernel_mul, self.kernel_num,
                                                           self.fix_sigma, dfeat_s=gs, dfeat_t=gt), source, target)
