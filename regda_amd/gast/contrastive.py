"""PixelContrastLoss -- mirror of regda/gast/contrastive.py::PixelContrastLoss (the pixel-wise supervised contrast of
Wang et al., ICCV 2021, with hard-anchor sampling) on rgda_pixel_contrast_select / rgda_pixel_contrast_loss.

The reference walks images and classes in Python (`unique`, `nonzero`, `randperm`, a dense (N, N) mask algebra).  Here
the device sorts the pixels of every image by (class, hard / easy) once; the host reads the 2 C counts per image back
(ONE host sync per call), derives the anchors, n_view and the keep counts, and takes the reference's `torch.randperm`
draws in the reference's order -- so a run seeded like the reference selects the reference's pixels; the device gathers
the rows and computes the loss and the feature gradient in one call.  The gradient is bf16 (the precision of the
feature gradient the fused steps hand to the instance-norm backward).

In `_hard_anchor_sampling` of the reference the arguments arrive swapped in name (`y_hat` is the downscaled label, `y`
the prediction); the behaviour is mirrored, not the names: anchors are classes of the LABEL, a pixel is hard when the
prediction differs from it.  Features are not normalised, as in the reference."""
import torch

from .. import ops
from ._rowsgrad import rows_loss


def plan_anchors(counts, max_samples=1024, max_views=100, generator=None):
    """The host side of `_hard_anchor_sampling` (contrastive.py:49-98) on CPU tensors.

    counts: integer (b, C, 2), the pixels per (image, class, hard / easy).  A class of an image with MORE than max_views
    pixels is an anchor (images in order, classes ascending); n_view = min(max_samples // A, max_views); the keep counts
    follow contrastive.py:82-90; per anchor `torch.randperm(num_hard)[:hard_keep]` then `torch.randperm(num_easy)
    [:easy_keep]` are drawn (the zero-length ones too) from `generator` (None: the global CPU generator).
    -> (anchors int32 [A, 3] = (image, class, hard_keep), ranks int32 [A, n_view]: the first hard_keep index the hard
    list, the rest the easy list), or (None, None) when no class qualifies."""
    cnt = torch.as_tensor(counts).to('cpu', torch.int64)
    b, C, _ = cnt.shape
    found = [(i, c) for i in range(b) for c in range(C) if int(cnt[i, c].sum()) > max_views]
    if not found:
        return None, None
    n_view = min(max_samples // len(found), max_views)
    if n_view < 1:
        raise ValueError(f'PixelContrastLoss: {len(found)} anchors leave no view within max_samples = {max_samples}')
    anchors = torch.empty(len(found), 3, dtype=torch.int32)
    ranks = torch.empty(len(found), n_view, dtype=torch.int32)
    for a, (i, c) in enumerate(found):
        num_hard, num_easy = int(cnt[i, c, 0]), int(cnt[i, c, 1])
        if num_hard >= n_view / 2 and num_easy >= n_view / 2:
            hard_keep = n_view // 2
            easy_keep = n_view - hard_keep
        elif num_hard >= n_view / 2:
            easy_keep = num_easy
            hard_keep = n_view - easy_keep
        elif num_easy >= n_view / 2:
            hard_keep = num_hard
            easy_keep = n_view - hard_keep
        else:       # more than max_views >= n_view pixels in two lists: one of them holds at least n_view / 2
            raise AssertionError((num_hard, num_easy, n_view))
        anchors[a] = torch.tensor([i, c, hard_keep], dtype=torch.int32)
        ranks[a, :hard_keep] = torch.randperm(num_hard, generator=generator)[:hard_keep]
        ranks[a, hard_keep:] = torch.randperm(num_easy, generator=generator)[:easy_keep]
    return anchors, ranks


def select_and_plan(labels, predict, class_num, size, ignore_label, max_samples, max_views, generator):
    """select on the device, the plan on the host -> (order, counts, anchors, ranks, flag) on the device; anchors is None
    when no class qualifies; flag int32 [1] has bit 2 set when a label outside [0, class_num) that is not ignore_label was
    seen (left on the device: reading it is the caller's sync).  One host sync here: the read-back of counts."""
    counts, order, flag = ops.pixel_contrast_select(labels, predict, class_num, size, ignore_label)
    anchors, ranks = plan_anchors(counts.cpu(), max_samples, max_views, generator)
    if anchors is None:
        return order, counts, None, None, flag
    return order, counts, anchors.to(labels.device), ranks.to(labels.device), flag


class PixelContrastLoss(torch.nn.Module):
    """class_num: the number of classes the labels take (the reference finds them with `unique`; the kernel sorts into
    2 <= class_num <= 16 classes); generator: the CPU generator of the `randperm` draws (None: the global one, as in the
    reference).  Both are extensions; the other attributes are the reference's and may be assigned afterwards.

    A difference in behaviour: the reference finds the classes with `unique`, so any label value can become an anchor;
    here a label outside [0, class_num) that is not ignore_label is treated as ignored.  It is not silent: after a
    forward, `last_flag` (int32 [1] on the device) has bit 2 set when such a label was seen; reading it costs the caller
    a sync, which is why forward does not."""

    def __init__(self, class_num=16, generator=None):
        super().__init__()
        self.temperature = 0.1
        self.base_temperature = 0.07
        self.ignore_label = -1
        self.max_samples = 1024
        self.max_views = 100
        self.eps = 1e-5
        self.class_num = class_num
        self.generator = generator
        self.last_flag = None

    def forward(self, feats, labels=None, predict=None):
        """feats f32 (b, k, h, w), labels int64 (b, H, W) (nearest-downscaled to (h, w): H % h == 0, W % w == 0), predict
        int64 (b, h, w) or f32 logits (b, class_num, h, w) -> the scalar loss (contrastive.py:145-162).  One host sync
        (the pixel counts come back for the random draws).  ValueError when no class of any image has more than
        max_views pixels (the reference fails there with an AttributeError on None)."""
        order, counts, anchors, ranks, self.last_flag = select_and_plan(
            labels, predict, self.class_num, feats.shape[2:], self.ignore_label, self.max_samples, self.max_views, self.generator)
        if anchors is None:
            raise ValueError(f'PixelContrastLoss: no class of any image has more than max_views = {self.max_views} '
                             f'labelled pixels, so there is no anchor to contrast')
        return rows_loss(lambda x, g: ops.pixel_contrast_loss(x, order, counts, anchors, ranks, self.temperature,
                                                              self.base_temperature, self.eps, dfeat=g), feats)
