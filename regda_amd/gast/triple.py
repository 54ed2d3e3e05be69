"""TripletLoss -- mirror of regda/gast/triple.py::TripletLoss (batch-hard triplet loss, Hermans et al.,
arXiv:1703.07737) on rgda_triplet_loss.

The reference materialises the (n, n) distance matrix and walks its rows in Python, two boolean-indexed reductions per
row.  The kernel mines the hardest positive and negative of every row inside the epilogue of one bf16 MFMA Gram pass (the
matrix is never stored), recomputes the two selected distances in fp32 from the unrounded rows and forms the gradient --
three rows per anchor -- in the same call; backward scales the stored gradient by the incoming one.  The gradient is
bf16 (the precision of the feature gradient the fused steps hand to the instance-norm backward).  Up to n = 16384 rows.

Two differences in behaviour: with fewer than two distinct labels the reference raises (`min()` of an empty tensor),
here the loss and the gradient are 0; and `ignore_label` (an extension, None by default: every value is a label, as in
the reference) removes the rows of that label from the anchors and the candidates."""
import torch

from .. import ops
from ._rowsgrad import rows_loss


class TripletLoss(torch.nn.Module):
    def __init__(self, margin=0.3, ignore_label=None):
        super().__init__()
        if margin < 0:
            raise ValueError('TripletLoss: margin must be >= 0')
        self.margin = margin
        self.ignore_label = ignore_label

    def forward(self, inputs, targets):
        """inputs (n, k) rows, targets int64 (n) -> the scalar loss (triple.py:30-55).  An NCHW (b, k, h, w) map is taken
        too (its pixels are the rows, without the permuted copy), with targets of b * h * w elements."""
        assert inputs.dim() in (2, 4)
        return rows_loss(lambda x, g: ops.triplet_loss(x, targets, self.margin, self.ignore_label, dfeat=g)[0], inputs)
