"""Cross-domain CutMix (regda/utils/cutmix.py:15-31) on rgda_domain_mix: one random box of the source batch is pasted
over the target batch, one launch.  The reference's cutmix2 (a shuffle within ONE batch) is not provided: it reads and
writes the same tensor, which an in-place kernel cannot do without a race."""
import numpy as np

from .. import ops


def draw_box(image_h, image_w, alpha=1.0):
    """The reference's draw (cutmix.py:17-27) from numpy's global generator, in its order (beta, then cx, then cy) and
    its float64 arithmetic with np.round -> (y0, y1, x0, x1)."""
    lam = np.random.beta(alpha, alpha)
    cx = np.random.uniform(0, image_w)
    cy = np.random.uniform(0, image_h)
    return box_from_draw(lam, cx, cy, image_h, image_w)


def box_from_draw(lam, cx, cy, image_h, image_w):
    w = image_w * np.sqrt(1 - lam)
    h = image_h * np.sqrt(1 - lam)
    x0 = int(np.round(max(cx - w / 2, 0)))
    x1 = int(np.round(min(cx + w / 2, image_w)))
    y0 = int(np.round(max(cy - h / 2, 0)))
    y1 = int(np.round(min(cy + h / 2, image_h)))
    return y0, y1, x0, x1


def cutmix(data_s, targets_s, data_t, targets_t, alpha=1.0, box=None):
    """data_s, data_t f32 (b,3,h,w) and targets_s, targets_t int64 (b,h,w) (or (b,1,h,w)) on the GPU -> clones
    (data_s, targets_s, data_t mixed, targets_t mixed) in the shapes given, the reference's return tuple.
    box = (y0, y1, x0, x1); None draws it as the reference does (draw_box)."""
    if box is None:
        box = draw_box(data_s.shape[2], data_s.shape[3], alpha)
    data_s, targets_s, data_t, targets_t = data_s.clone(), targets_s.clone(), data_t.clone(), targets_t.clone()
    ops.domain_mix(data_s, targets_s, data_t, label_t=targets_t, box=box)
    return data_s, targets_s, data_t, targets_t
