"""SAW -- mirror of regda/gast/SAW.py::SAW (semantic-aware whitening, Peng et al., CVPR 2022) on rgda_saw_loss: for
every selected class the channels are ranked by the magnitude of the classifier weight, the C channels of one rank,
each scaled by the sigmoid of its magnitude, form a group, and the off-diagonal covariances of every group are
penalised above a margin.

The forward computes the loss and the input gradient in one call; backward scales the stored gradient by the incoming
one.  The gradient is bf16 (the precision of the feature gradient the fused steps hand to the instance-norm backward);
its rows are as wide as the feature map, so the module serves channel counts that are multiples of 8 (ops.saw_loss with
a padded buffer serves any).  The classifier is a constant of the loss, as in the reference (it reads `state_dict()`).
Where the reference's `torch.sort` leaves the order of equal magnitudes unspecified, the lower channel index ranks
first."""
import torch

from .. import ops
from ._rowsgrad import rows_loss


def classifier_weight(classifyer):
    """The relevance weights as the reference finds them (SAW.py:79-90): the last `state_dict()` entry whose key contains
    "weight", squeezed -- or, as an extension, an (n_cls, k) tensor itself."""
    if isinstance(classifyer, torch.Tensor):
        w = classifyer
    else:
        w = None
        sd = classifyer.state_dict()
        for key in sd.keys():
            if 'weight' in key:
                w = sd[key]
        if w is None:
            raise ValueError('SAW: the classifier has no "weight" entry in its state_dict()')
        w = w.squeeze()
    if w.dim() != 2:
        raise ValueError(f'SAW: the classifier weight is {tuple(w.shape)} after squeeze(); an (n_cls, k) matrix is needed')
    return w.detach()


class SAW(torch.nn.Module):
    def __init__(self, classifyer, selected_classes, relax_denom=2.0):
        """classifyer, selected_classes, relax_denom: the reference's constructor.  classifyer: a module (its weight is
        read at every forward) or an (n_cls, k) tensor; len(selected_classes) in (2, 4, 6, 8, 16)."""
        super().__init__()
        self.selected_classes = [int(c) for c in selected_classes]
        self.C = len(self.selected_classes)
        if self.C not in ops.SAW_CLASS_COUNTS:
            raise ValueError(f'SAW: {self.C} selected classes; served are {ops.SAW_CLASS_COUNTS}')
        if len(set(self.selected_classes)) != self.C:
            raise ValueError(f'SAW: selected_classes {self.selected_classes} repeats a class')
        self.classifyer = classifyer
        self.relax_denom = relax_denom
        self.num_off_diagonal = self.C * (self.C - 1) // 2
        self.margin = ops.saw_margin(self.C, relax_denom)

    def get_mask_matrix(self):
        """(eye, the strict upper-triangle mask, margin, the number of off-diagonal pairs), as in the reference; the
        kernel needs none of them."""
        i = torch.eye(self.C, self.C)
        reversal_i = torch.ones(self.C, self.C).triu(diagonal=1)
        return i, reversal_i, self.margin, reversal_i.sum()

    def forward(self, x):
        """x (b, k, h, w) -> the loss, shape (1,) as in the reference, differentiable w.r.t. x only"""
        assert x.dim() == 4
        w = classifier_weight(self.classifyer)
        if w.shape[1] != x.shape[1]:
            raise ValueError(f'SAW: the classifier has {w.shape[1]} input channels, the features {x.shape[1]}')
        w = w.to(x.device)
        sel, rd = self.selected_classes, self.relax_denom
        return rows_loss(lambda f, g: ops.saw_loss(f, w, sel, rd, 1.0, dfeat=g), x).view(1)
