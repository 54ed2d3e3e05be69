"""ClassWareWhitening -- mirror of regda/gast/class_ware_whiten.py::ClassWareWhitening on rgda_whiten_loss: for every
class and every group of channels, mean((S - I)^2) of the covariance S of the class's pixel rows, summed.

The forward computes the loss and the input gradient in one call (the kernel has the S - I blocks at hand); backward
scales the stored gradient by the incoming one.  The gradient is bf16 (the precision of the feature gradient the
fused steps hand to the instance-norm backward)."""
import torch

from .. import ops
from ._rowsgrad import rows_loss


class ClassWareWhitening(torch.nn.Module):
    def __init__(self, class_ids=(), groups=1, ignore_label=-1):
        """class_ids, groups: the reference's constructor.  Served: class_ids == range(C) (what Aligner builds; anything
        else is refused here) with 6 <= C <= 16 and 32, 64, 96 or 128 channels per group (refused at the call, so that
        an Aligner can be built for any class_num, as before).  ignore_label (not in the reference, which compares
        labels with the class ids only): the label of the pixels that belong to no class; any other label outside
        range(C) sets the kernel's range flag."""
        super().__init__()
        assert groups >= 1
        ids = list(class_ids)
        if ids != list(range(len(ids))):
            raise NotImplementedError(f'ClassWareWhitening(class_ids={ids}): served are class_ids = range(C) with '
                                      f'6 <= C <= 16')
        self.class_ids = class_ids
        self.groups = groups
        self.ignore_label = ignore_label

    def forward(self, feats, labels):
        """feats (b, k, h, w); labels (b, 1, h, w) or (b, h, w) int64 at feature resolution -> the scalar sum of the
        whitening terms of every class and group."""
        assert len(feats.shape) == 4 and len(labels.shape) >= 3
        assert feats.shape[1] % self.groups == 0
        C = len(list(self.class_ids))
        if not 6 <= C <= 16:
            raise NotImplementedError(f'ClassWareWhitening: {C} classes; served are class_ids = range(C) with 6 <= C <= 16')
        s = feats.shape[1] // self.groups
        if s not in ops.WHITEN_BLOCKS:
            raise NotImplementedError(f'ClassWareWhitening: {s} channels per group (k = {feats.shape[1]}, groups = '
                                      f'{self.groups}); served are {ops.WHITEN_BLOCKS} channels per group')
        labels = labels.long()
        return rows_loss(lambda x, g: ops.whiten_loss(x, labels, C, self.groups, self.ignore_label, 1.0, dfeat=g), feats)
