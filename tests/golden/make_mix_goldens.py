"""Mint tests/golden/mix.npz from the reference's OWN classmix and cutmix (regda/utils/classmix.py, cutmix.py), run on
the CPU through tests/golden/_refstubs.py (`.cuda()` is a no-op there; cv2 is stubbed where it is absent).

Run in the build container only (needs the reference checkout):  python tests/golden/make_mix_goldens.py
Data only: seeds, the drawn class ids and boxes, inputs and the reference's outputs.
  Tiles are 2 x 3 x 24 x 20 with C = 6 and C = 7; source labels are blocky with ignore_label pixels, images are small
  integers as floats (exact, compressible).
  classmix: per (C, seed) torch.manual_seed(seed) -> the reference's outputs; the class ids are read off the same seed
  (torch.randperm(C)[:int(C * ratio)], classmix.py:42).  The targets_s the reference returns carries C at the
  ignore_label pixels (tools.py:413 writes into the clone); it is stored as the reference returned it.
  cutmix: per seed np.random.seed(seed) -> outputs; the box is read off a coordinate image run under the same seed.
Every case has a non-empty pasted set and a non-empty untouched set (asserted)."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _refstubs  # noqa: E402

N, H, W = 2, 24, 20
IGNORE = -1
RATIO = 0.5
CLASS_SEEDS = (0, 1, 2, 3)
BOX_SEEDS = (0, 1, 2, 3, 4, 5)


def inputs(rng, C):
    img_s = rng.integers(-300, 300, (N, 3, H, W)).astype(np.float32) / 4
    img_t = rng.integers(-300, 300, (N, 3, H, W)).astype(np.float32) / 4
    lab_s = np.kron(rng.integers(-1, C, (N, H // 4, W // 4)), np.ones((4, 4), np.int64))
    lab_s[:, ::5, 1::3] = rng.integers(-1, C, lab_s[:, ::5, 1::3].shape)         # ragged pixels inside the blocks
    lab_t = rng.integers(-1, C, (N, H, W)).astype(np.int64)
    return img_s, lab_s.astype(np.int64), img_t, lab_t


def main():
    _refstubs.install()
    from regda.utils.classmix import classmix
    from regda.utils.cutmix import cutmix
    rng = np.random.default_rng(20261017)
    out = dict(ignore_label=np.int64(IGNORE), ratio=np.float64(RATIO), class_seeds=np.array(CLASS_SEEDS, np.int64),
               box_seeds=np.array(BOX_SEEDS, np.int64))
    for C in (6, 7):
        img_s, lab_s, img_t, lab_t = inputs(rng, C)
        out.update({'c%d_img_s' % C: img_s, 'c%d_lab_s' % C: lab_s, 'c%d_img_t' % C: img_t, 'c%d_lab_t' % C: lab_t})
        t = [torch.from_numpy(a) for a in (img_s, lab_s[:, None], img_t, lab_t[:, None])]
        ids, o_img, o_lab, o_lab_s = [], [], [], []
        for seed in CLASS_SEEDS:
            torch.manual_seed(seed)
            drawn = torch.randperm(C)[: int(C * RATIO)].numpy()
            torch.manual_seed(seed)
            ds, ts, dt, tt = classmix(*t, ratio=RATIO, class_num=C, ignore_label=IGNORE)
            assert torch.equal(ds, t[0]) and torch.equal(t[1], torch.from_numpy(lab_s[:, None]))     # inputs untouched
            pasted = np.isin(lab_s, drawn)
            assert pasted.any() and not pasted.all(), (C, seed)
            assert tt.shape == (N, H, W) and tt.dtype == torch.int64
            ids.append(drawn)
            o_img.append(dt.numpy())
            o_lab.append(tt.numpy())
            o_lab_s.append(ts.numpy())
        out.update({'c%d_class_ids' % C: np.stack(ids).astype(np.int64), 'c%d_class_img_out' % C: np.stack(o_img),
                    'c%d_class_lab_out' % C: np.stack(o_lab), 'c%d_class_lab_s_out' % C: np.stack(o_lab_s)})
        coord = torch.arange(N * 3 * H * W, dtype=torch.float32).view(N, 3, H, W)
        t3 = [torch.from_numpy(a) for a in (img_s, lab_s, img_t, lab_t)]         # cutmix indexes (b, h, w) targets
        boxes, o_img, o_lab = [], [], []
        for seed in BOX_SEEDS:
            np.random.seed(seed)
            _, _, dc, _ = cutmix(coord, t3[1], -torch.ones_like(coord), t3[3], alpha=1.0)
            ys, xs = np.nonzero((dc[0, 0] >= 0).numpy())
            assert ys.size and ys.size < H * W, seed
            box = (ys.min(), ys.max() + 1, xs.min(), xs.max() + 1)
            assert ys.size == (box[1] - box[0]) * (box[3] - box[2])
            np.random.seed(seed)
            ds, ts, dt, tt = cutmix(*t3, alpha=1.0)
            assert torch.equal(ds, t3[0]) and torch.equal(ts, t3[1])
            boxes.append(box)
            o_img.append(dt.numpy())
            o_lab.append(tt.numpy())
        out.update({'c%d_boxes' % C: np.array(boxes, np.int64), 'c%d_box_img_out' % C: np.stack(o_img),
                    'c%d_box_lab_out' % C: np.stack(o_lab)})
    path = os.path.join(HERE, 'mix.npz')
    np.savez_compressed(path, **out)
    print('wrote %s (%d bytes)' % (path, os.path.getsize(path)))
    for C in (6, 7):
        print(C, out['c%d_class_ids' % C].tolist(), out['c%d_boxes' % C].tolist())


if __name__ == '__main__':
    main()
