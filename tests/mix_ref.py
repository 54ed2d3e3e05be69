"""numpy restatement of rgda_domain_mix (include/rgda_hip.h): cross-domain ClassMix / CutMix over a batch.  Works on
copies; the flag is returned.  Values are moved, never computed, so every comparison against it is bit for bit."""
import numpy as np

MIX_CLASS, MIX_BOX = 0, 1


def cond_mask(label_s, C, classes=None, box=None, ignore_label=-1):
    """-> (cond bool [N][H][W], flag): the pasted pixels, and whether a label that is read is neither a class nor
    ignore_label (class mode reads every label, box mode the labels inside the box)."""
    l = np.asarray(label_s).reshape(label_s.shape[0], label_s.shape[-2], label_s.shape[-1])
    in_range = (l >= 0) & (l < C)
    bad = ~in_range & (l != ignore_label)
    if classes is not None:
        bits = 0
        for c in classes:
            assert 0 <= int(c) < C
            bits |= 1 << int(c)
        cond = in_range & (((bits >> np.where(in_range, l, 0)) & 1) == 1)
        read = np.ones_like(cond) if bits else np.zeros_like(cond)
    else:
        y0, y1, x0, x1 = box
        assert 0 <= y0 <= y1 <= l.shape[1] and 0 <= x0 <= x1 <= l.shape[2]
        cond = np.zeros(l.shape, bool)
        cond[:, y0:y1, x0:x1] = True
        read = cond
    return cond, int((bad & read).any())


def domain_mix(img_s, label_s, img_t, label_t=None, soft_t=None, regs_t=None, C=None, classes=None, box=None,
               ignore_label=-1):
    """-> (img_t, label_t, soft_t, regs_t, flag, cond): mixed copies (None where the input is None)."""
    assert (classes is None) != (box is None)
    if C is None:
        C = soft_t.shape[1] if soft_t is not None else 32
    cond, flag = cond_mask(label_s, C, classes, box, ignore_label)
    l = np.asarray(label_s).reshape(cond.shape)
    img = np.array(img_t, copy=True)
    m3 = np.broadcast_to(cond[:, None], img.shape)
    img.view(np.uint32)[m3] = np.ascontiguousarray(img_s).view(np.uint32)[m3]      # moved as bits: NaN payloads survive
    lab = soft = regs = None
    if label_t is not None:
        lab = np.array(label_t, copy=True)
        lab.reshape(cond.shape)[cond] = l[cond]
    if soft_t is not None:
        soft = np.array(soft_t, copy=True)
        for c in range(C):
            soft[:, c][cond] = (l[cond] == c).astype(np.float32)
    if regs_t is not None:
        regs = np.array(regs_t, copy=True)
        regs.reshape(cond.shape)[cond] = 0
    return img, lab, soft, regs, flag, cond


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def golden_cases(g):
    """-> (C, kind, k, inputs, predicate kwargs, expected image, expected label) of every case of the golden."""
    for C in (6, 7):
        inp = [g['c%d_%s' % (C, n)] for n in ('img_s', 'lab_s', 'img_t', 'lab_t')]
        for k, ids in enumerate(g['c%d_class_ids' % C]):
            yield C, 'class', k, inp, dict(classes=[int(c) for c in ids]), g['c%d_class_img_out' % C][k], g['c%d_class_lab_out' % C][k]
        for k, box in enumerate(g['c%d_boxes' % C]):
            yield C, 'box', k, inp, dict(box=tuple(int(v) for v in box)), g['c%d_box_img_out' % C][k], g['c%d_box_lab_out' % C][k]
