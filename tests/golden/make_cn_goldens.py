"""Mint golden vectors at 8, 11 and 16 classes (OpenEarthMap / UAVid, an odd count, iSAID / GID-15 with background) from
the reference's OWN Python, imported behind the stubs of make_goldens.py, like make_c7_goldens.py.

Run in the build container only (needs the reference checkout):
    python tests/golden/make_cn_goldens.py
Writes cn.npz next to this file; every key carries its class count (`c8_...`, `c11_...`, `c16_...`): inputs and the
reference's outputs of pseudo_selection, Homogenizer (ties, percent at exactly the boundary), DownscaleLabel,
label_refine (with and without superpixels) and PrototypeContrastiveLoss (loss and feature gradient).  The
large DownscaleLabel case (b = 8, 512 x 512, the SSL step's shape) is not stored: `downscale_big_input(C)` rebuilds it
from a seed and the file keeps its checksum next to the reference's output.
"""
import os
import sys

import numpy as np

COUNTS = (8, 11, 16)
HERE = os.path.dirname(os.path.abspath(__file__))


def downscale_big_input(C):
    """(8, 512, 512) int64 labels in [-1, C): per 16 x 16 cell a dominant label on 150..256 of its pixels, uniform noise
    elsewhere, shuffled inside the cell, plus hand-set cells in image 0, row 0: ratio exactly 0.75 (kept), 191/256
    (dropped), a class tied with ignore (128 / 128), all ignore, the highest class C - 1 winning at 200/256 and at
    256/256, C - 1 at exactly 0.75 next to ignore, ignore at exactly 0.75, C - 1 tied with ignore, and a four-way tie."""
    rng = np.random.default_rng(20240707 + C)
    b, h, w = 8, 32, 32
    dom = rng.integers(-1, C, size=(b, h, w, 1))
    k = rng.integers(150, 257, size=(b, h, w, 1))
    noise = rng.integers(-1, C, size=(b, h, w, 256))
    cells = np.where(np.arange(256) < k, dom, noise)
    cells = rng.permuted(cells, axis=-1)

    def cell(*parts):
        v = np.concatenate([np.full(n, c, np.int64) for c, n in parts])
        assert v.size == 256
        return v

    t = C - 1
    special = [cell((2, 192), (5, 64)), cell((2, 191), (5, 65)), cell((3, 128), (-1, 128)), cell((-1, 256)),
               cell((t, 200), (0, 56)), cell((t, 256)), cell((t, 192), (-1, 64)), cell((-1, 192), (t, 64)),
               cell((t, 128), (-1, 128)), cell((0, 64), (7, 64), (t, 64), (-1, 64))]
    for x, v in enumerate(special):
        cells[0, 0, x] = v
    lab = cells.reshape(b, h, w, 16, 16).transpose(0, 1, 3, 2, 4).reshape(b, h * 16, w * 16)
    return np.ascontiguousarray(lab.astype(np.int64))


def checksum(a):
    """Order-sensitive integer checksum of a label array (detects a drifted generator)."""
    v = a.reshape(-1).astype(np.int64) + 2
    return np.int64((v * (np.arange(v.size, dtype=np.int64) % 1000003 + 1)).sum())


def _regions(rng, b, h, w, nreg):
    regs = np.zeros((b, h, w), np.int64)
    for i in range(b):
        for r in range(1, nreg + 1):
            y0, x0 = rng.integers(0, h), rng.integers(0, w)
            hh, ww = rng.integers(1, max(2, h // 2)), rng.integers(1, max(2, w // 2))
            if rng.random() > 0.2:
                regs[i, y0:y0 + hh, x0:x0 + ww] = r
    return regs


def mint(C, out):
    import torch
    from regda.utils.local_region_homog import Homogenizer
    from regda.gast.pseudo_generation import pseudo_selection
    from regda.gast.alignment import DownscaleLabel
    p = f'c{C}_'
    # ---- pseudo_selection: softmax maps, and a case where only the highest class passes its threshold
    rng = np.random.default_rng(77 + C)
    ps = []
    for (b, h, w, sharp) in [(2, 32, 32, 3.0), (1, 17, 9, 8.0)]:
        logits = rng.normal(size=(b, C, h, w)).astype(np.float32) * sharp
        ps.append(torch.softmax(torch.from_numpy(logits), 1).numpy())
    top = np.full((1, C, 1, 4), 0.05, np.float32)
    top[0, C - 1, 0, :] = [0.7, 0.65, 0.59, 0.9]
    top[0, 0, 0, 3] = 0.9                                               # two classes pass -> ambiguous
    ps.append(top)
    for i, s in enumerate(ps):
        out[f'{p}ps_in{i}'] = s
        out[f'{p}ps_out{i}'] = pseudo_selection(torch.from_numpy(s.copy()), 0.8, 0.6, 'tensor', -1).numpy().astype(np.int8)
    out[f'{p}ps_n'] = np.int64(len(ps))

    # ---- Homogenizer: label-correlated random regions, tie sets (one region of n pixels, half the highest class and half
    # class 2; half the highest class and half ignore), and percent at exactly the boundary (3 of 4 pixels, percent 0.75
    # in fp32 against 3 / (4 + 1e-5))
    rng = np.random.default_rng(2333 + C)
    cases = []
    for (b, h, w, nreg, pct) in [(2, 64, 64, 40, 0.5), (2, 64, 64, 300, 0.5)]:
        lab = rng.integers(-1, C, size=(b, h, w)).astype(np.int64)
        regs = _regions(rng, b, h, w, nreg)
        for r in range(1, nreg + 1, 2):
            lab[(regs == r) & (rng.random((b, h, w)) < 0.7)] = r % C
        cases.append((lab, regs, pct))
    for n in [2, 256]:
        side = int(np.ceil(np.sqrt(n)))
        for first, second in ((C - 1, 2), (2, C - 1), (C - 1, -1)):
            lab = np.full((1, side, side + 1), 3, np.int64)
            regs = np.zeros((1, side, side + 1), np.int64)
            fl, fr = lab.reshape(-1), regs.reshape(-1)
            fr[:n] = 1
            fl[:n // 2] = first
            fl[n // 2:n] = second
            cases.append((lab, regs, 0.5))
    for pct in (0.75, float(np.float32(3) / np.float32(4.00001))):
        lab = np.array([[[C - 1, C - 1, C - 1, 0, 5, 5, 5, 5]]], np.int64)
        regs = np.array([[[1, 1, 1, 1, 2, 2, 2, 0]]], np.int64)
        cases.append((lab, regs, pct))
    for i, (lab, regs, pct) in enumerate(cases):
        res = Homogenizer(percent=pct, class_num=C, ignore_label=-1)(torch.from_numpy(lab.copy()), torch.from_numpy(regs.copy()))
        out[f'{p}lrh_lab{i}'] = lab.astype(np.int8)
        out[f'{p}lrh_reg{i}'] = regs.astype(np.int32)
        out[f'{p}lrh_pct{i}'] = np.float64(pct)
        out[f'{p}lrh_out{i}'] = res.numpy().astype(np.int8)
    out[f'{p}lrh_n'] = np.int64(len(cases))

    # ---- DownscaleLabel: the big seeded case (output + input checksum only)
    ds = DownscaleLabel(scale_factor=16, n_classes=C, ignore_label=-1, min_ratio=0.75)
    big = downscale_big_input(C)
    out[f'{p}ds_big_sum'] = checksum(big)
    out[f'{p}ds_big_out'] = ds(torch.from_numpy(big.copy())).numpy().astype(np.int8)


class _Log:
    def info(self, *a, **k):
        pass


def mint_float(C, out):
    """label_refine (mode 'all', without and with superpixels) and PrototypeContrastiveLoss with its feature
    gradient, from the reference's Aligner and loss class at C classes (small shapes: the file stays small)."""
    import torch
    from regda.gast.alignment import Aligner
    from regda.loss import PrototypeContrastiveLoss
    p = f'c{C}_'
    torch.manual_seed(500 + C)
    b, k, h, w, H = 1, 64, 4, 4, 32
    al = Aligner(logger=_Log(), feat_channels=k, class_num=C, ignore_label=-1, decay=0.996, resume=None)
    protos = torch.randn(C, k)
    al.prototypes = protos.clone()
    feat_t = torch.randn(b, k, h, w)
    p1, p2 = torch.randn(b, C, h, w) * 2, torch.randn(b, C, h, w) * 2
    soft = torch.softmax(torch.randn(b, C, H, H) * 3, 1)
    sup = _regions(np.random.default_rng(17 + C), b, H, H, 23)
    sup[0, 20:25, 4:15] = 31                     # the largest id of the batch: ignored
    sup_t = torch.from_numpy(sup).reshape(b, 1, H, H)
    out.update({p + 'rf_feat': feat_t.numpy(), p + 'rf_protos': protos.numpy(), p + 'rf_p1': p1.numpy(),
                p + 'rf_p2': p2.numpy(), p + 'rf_soft': soft.numpy(), p + 'rf_sup': sup.astype(np.int8),
                p + 'rf_out': al.label_refine(None, feat_t, [p1, p2], soft, refine=True, mode='all', temp=2.0).numpy(),
                p + 'rf_out_sup': al.label_refine(sup_t, feat_t, [p1, p2], soft, refine=True, mode='all', temp=2.0).numpy()})
    b, K, h, w = 2, 64, 5, 7
    feat = (torch.randn(b, K, h, w) * 1.5 + 0.2).requires_grad_(True)
    protos = torch.randn(C, K)
    lab = torch.randint(0, C, (b, h, w))
    lab[torch.rand(b, h, w) < 0.3] = -1
    loss = PrototypeContrastiveLoss(temperature=8.0, ignore_label=-1)(protos, feat, lab)
    loss.backward()
    out.update({p + 'pcl_feat': feat.detach().numpy(), p + 'pcl_protos': protos.numpy(), p + 'pcl_lab': lab.numpy().astype(np.int8),
                p + 'pcl_loss': loss.detach().numpy(), p + 'pcl_gfeat': feat.grad.numpy()})


def main():
    sys.path.insert(0, HERE)
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    import _refstubs
    _refstubs.install()
    out = {}
    for C in COUNTS:
        mint(C, out)
        mint_float(C, out)
    np.savez_compressed(os.path.join(HERE, 'cn.npz'), **out)
    print('wrote cn.npz', len(out), 'arrays')


if __name__ == '__main__':
    main()
