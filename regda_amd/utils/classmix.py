"""Cross-domain ClassMix (regda/utils/classmix.py:17-53) on rgda_domain_mix: the pixels of a random subset of the classes
are pasted from the source batch over the target batch, one launch."""
import torch

from .. import ops


def draw_class_ids(class_num=7, ratio=0.5):
    """The reference's draw (classmix.py:42): `torch.randperm(class_num)[:int(class_num * ratio)]` from torch's global
    CPU generator, so the same seed gives the same classes."""
    return torch.randperm(class_num)[: int(class_num * ratio)]


def classmix(data_s, targets_s, data_t, targets_t, ratio=0.5, class_num=7, ignore_label=-1, class_ids=None):
    """data_s, data_t f32 (b,3,h,w) and targets_s, targets_t (b,h,w) or (b,1,h,w) on the GPU -> clones
    (data_s, targets_s (b,h,w) long, data_t mixed, targets_t (b,h,w) long mixed), the reference's return tuple.
    class_ids: the classes to paste; None draws them as the reference does (draw_class_ids).
    One difference, on the tensor that is NOT mixed: the reference's index2onehot writes class_num over the
    ignore_label pixels of the targets_s it returns (tools.py:413, a side effect on the clone); here the returned
    targets_s is the unchanged clone."""
    if class_ids is None:
        class_ids = draw_class_ids(class_num, ratio)
    data_s, targets_s, data_t, targets_t = data_s.clone(), targets_s.clone().long(), data_t.clone(), targets_t.clone().long()
    if targets_s.dim() == 4:
        targets_s = targets_s.squeeze(dim=1)
    if targets_t.dim() == 4:
        targets_t = targets_t.squeeze(dim=1)
    ops.domain_mix(data_s, targets_s, data_t, label_t=targets_t, classes=[int(c) for c in class_ids],
                   ignore_label=ignore_label, class_num=class_num)
    return data_s, targets_s, data_t, targets_t
