"""Mint the seven-class (LoveDA: NUM_CLASSES = 7, regda/datasets/loveda.py) golden vectors from the reference's OWN
Python, imported behind the stubs of make_goldens.py.

Run in the build container only (needs the reference checkout):
    python tests/golden/make_c7_goldens.py
Writes c7.npz next to this file: inputs and the reference's outputs of pseudo_selection, Homogenizer and DownscaleLabel
at class_num = 7.  The large DownscaleLabel case (b = 8, 512 x 512, the SSL step's shape) is not stored: its input is
rebuilt from a seed by `downscale_big_input` (imported by tests/test_seven_class_gpu.py), and the file keeps its
checksum next to the reference's output.
"""
import os
import sys

import numpy as np

C = 7
HERE = os.path.dirname(os.path.abspath(__file__))


def downscale_big_input():
    """(8, 512, 512) int64 labels in [-1, 7): per 16 x 16 cell a dominant label (class 0..6 or -1) on 150..256 of its
    pixels, uniform noise elsewhere, shuffled inside the cell -- many cells land on either side of the 0.75 ratio --
    plus hand-set cells in image 0, row 0: ratio exactly 0.75 (kept), 191/256 (dropped), class 3 tied with ignore
    (128 / 128), all ignore, class 6 winning at 200/256 and at 256/256, class 6 at exactly 0.75 next to ignore."""
    rng = np.random.default_rng(20240707)
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

    special = [cell((2, 192), (5, 64)), cell((2, 191), (5, 65)), cell((3, 128), (-1, 128)), cell((-1, 256)),
               cell((6, 200), (0, 56)), cell((6, 256)), cell((6, 192), (-1, 64)), cell((-1, 192), (6, 64)),
               cell((6, 128), (-1, 128)), cell((0, 64), (1, 64), (6, 64), (-1, 64))]
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


def main():
    sys.path.insert(0, HERE)
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    import torch
    import _refstubs
    _refstubs.install()
    from regda.utils.local_region_homog import Homogenizer
    from regda.gast.pseudo_generation import pseudo_selection
    from regda.gast.alignment import DownscaleLabel

    out = {}
    # ---- pseudo_selection at 7 classes: softmax maps, and a case where only class 6 passes its threshold
    rng = np.random.default_rng(77)
    ps = []
    for (b, h, w, sharp) in [(2, 32, 32, 3.0), (1, 17, 9, 8.0), (2, 16, 16, 0.5)]:
        logits = rng.normal(size=(b, C, h, w)).astype(np.float32) * sharp
        ps.append(torch.softmax(torch.from_numpy(logits), 1).numpy())
    six = np.full((1, C, 1, 4), 0.05, np.float32)
    six[0, 6, 0, :] = [0.7, 0.65, 0.59, 0.9]
    six[0, 0, 0, 3] = 0.9                                               # two classes pass -> ambiguous
    ps.append(six)
    for i, p in enumerate(ps):
        out[f'ps_in{i}'] = p
        out[f'ps_out{i}'] = pseudo_selection(torch.from_numpy(p.copy()), 0.8, 0.6, 'tensor', -1).numpy().astype(np.int8)
    out['ps_n'] = np.int64(len(ps))

    # ---- Homogenizer at 7 classes: label-correlated random regions, then tie sets (one region of n pixels, half class 6
    # and half class 2; half class 6 and half ignore) at n in {2, 254, 256, 258}
    rng = np.random.default_rng(2333)
    cases = []
    for (b, h, w, nreg, pct) in [(2, 64, 64, 40, 0.5), (3, 48, 80, 25, 0.9), (2, 64, 64, 300, 0.5)]:
        lab = rng.integers(-1, C, size=(b, h, w)).astype(np.int64)
        regs = _regions(rng, b, h, w, nreg)
        for r in range(1, nreg + 1, 2):
            lab[(regs == r) & (rng.random((b, h, w)) < 0.7)] = r % C
        cases.append((lab, regs, pct))
    for n in [2, 254, 256, 258]:
        side = int(np.ceil(np.sqrt(n)))
        for first, second in ((6, 2), (2, 6), (6, -1)):
            lab = np.full((1, side, side + 1), 3, np.int64)
            regs = np.zeros((1, side, side + 1), np.int64)
            fl, fr = lab.reshape(-1), regs.reshape(-1)
            fr[:n] = 1
            fl[:n // 2] = first
            fl[n // 2:n] = second
            cases.append((lab, regs, 0.5))
    for i, (lab, regs, pct) in enumerate(cases):
        res = Homogenizer(percent=pct, class_num=C, ignore_label=-1)(torch.from_numpy(lab.copy()), torch.from_numpy(regs.copy()))
        out[f'lrh_lab{i}'] = lab.astype(np.int8)
        out[f'lrh_reg{i}'] = regs.astype(np.int32)
        out[f'lrh_pct{i}'] = np.float64(pct)
        out[f'lrh_out{i}'] = res.numpy().astype(np.int8)
    out['lrh_n'] = np.int64(len(cases))

    # ---- DownscaleLabel at 7 classes: the big seeded case (output + input checksum only)
    ds = DownscaleLabel(scale_factor=16, n_classes=C, ignore_label=-1, min_ratio=0.75)
    big = downscale_big_input()
    out['ds_big_sum'] = checksum(big)
    out['ds_big_out'] = ds(torch.from_numpy(big.copy())).numpy().astype(np.int8)
    np.savez_compressed(os.path.join(HERE, 'c7.npz'), **out)
    print('wrote c7.npz', len(out), 'arrays')


if __name__ == '__main__':
    main()
