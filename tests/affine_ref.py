"""CPU restatement of rgda_augment_affine (include/rgda_hip.h) in numpy integers: one affine map per sample, bilinear
image taps with 8-bit weights, nearest labels and regions, the soft planes with the image's taps and weights (in fp64
here: the kernel's f32 sum is compared within its rounding).  Used by tests/test_affine_*.py."""
import numpy as np

A_MAX = 131072


def make_row(cy, cx, m, fill=(0, 0, 0)):
    """(cy, cx) the centre in raw-tile pixels (pixel centre k at k + 0.5), m the 2 x 2 output-to-source matrix."""
    a = [int(round(float(v) * 32768)) for v in (m[0][0], m[0][1], m[1][0], m[1][1])]
    return [int(round(cy * 65536)), int(round(cx * 65536))] + a + [fill[0] | fill[1] << 8 | fill[2] << 16, 0]


def dihedral_row(y0, x0, d, ho, wo):
    """The row that equals rgda_augment_tiles' (y0, x0, d): d = t | fr << 1 | fc << 2."""
    sr, sc = (-1 if d & 2 else 1), (-1 if d & 4 else 1)
    m = [[0, sr], [sc, 0]] if d & 1 else [[sr, 0], [0, sc]]
    return make_row(y0 + ho / 2, x0 + wo / 2, m)


def rot(s, theta):
    """(1/s) [[cos, -sin], [sin, cos]], theta in degrees."""
    c, sn = np.cos(np.deg2rad(theta)), np.sin(np.deg2rad(theta))
    return np.array([[c, -sn], [sn, c]]) / s


def row_valid(row, hi, wi):
    cy, cx, a00, a01, a10, a11, fill, z = (int(v) for v in row)
    return (max(abs(a00), abs(a01), abs(a10), abs(a11)) <= A_MAX and 0 <= cy <= hi * 65536 and 0 <= cx <= wi * 65536
            and z == 0 and 0 <= fill < 1 << 24)


def coords(row, ho, wo):
    """-> (Y, X) int64 [ho][wo]: the source coordinate of every output pixel in 1/65536 pixel."""
    cy, cx, a00, a01, a10, a11 = (int(v) for v in row[:6])
    u = (2 * np.arange(ho, dtype=np.int64) + 1 - ho)[:, None]
    v = (2 * np.arange(wo, dtype=np.int64) + 1 - wo)[None, :]
    return cy + a00 * u + a01 * v, cx + a10 * u + a11 * v


def _gather(plane, y, x, outside):
    """plane [H][W] at integer (y, x) [ho][wo]; `outside` where (y, x) is not in the plane."""
    h, w = plane.shape
    ok = (y >= 0) & (y < h) & (x >= 0) & (x < w)
    return np.where(ok, plane[np.clip(y, 0, h - 1), np.clip(x, 0, w - 1)], outside)


def warp_one(row, size, img, lut, label=None, label_lut=None, ignore_label=-1, soft=None, regs=None):
    """One sample: img uint8 [H][W][3], label uint8 [H][W], soft f32 [C][H][W], regs int32 [H][W] (numpy).
    -> dict(image f32 [3][ho][wo], byte uint8 [3][ho][wo], label int64, soft f64 [C][ho][wo], regs int64 [1][ho][wo],
            inframe bool [ho][wo]: the nearest source pixel lies inside the input, exact bool: fx = fy = 0)."""
    ho, wo = size
    hi, wi = img.shape[:2]
    Y, X = coords(row, ho, wo)
    Yp, Xp = Y - 32768, X - 32768
    y, x = Yp >> 16, Xp >> 16
    fy, fx = (Yp & 0xFFFF) >> 8, (Xp & 0xFFFF) >> 8
    w = [(256 - fx) * (256 - fy), fx * (256 - fy), (256 - fx) * fy, fx * fy]
    taps = [(y, x), (y, x + 1), (y + 1, x), (y + 1, x + 1)]
    fill = int(row[6])
    out = {'byte': np.empty((3, ho, wo), np.uint8), 'image': np.empty((3, ho, wo), np.float32)}
    for ch in range(3):
        plane = img[:, :, ch].astype(np.int64)
        acc = sum(wk * _gather(plane, ty, tx, (fill >> (8 * ch)) & 255) for wk, (ty, tx) in zip(w, taps))
        out['byte'][ch] = (acc + 32768) >> 16
        out['image'][ch] = lut[ch][out['byte'][ch]]
    ny, nx = Y >> 16, X >> 16
    out['inframe'] = (ny >= 0) & (ny < hi) & (nx >= 0) & (nx < wi)
    out['exact'] = (fx == 0) & (fy == 0)
    if label is not None:
        out['label'] = np.where(out['inframe'], label_lut.astype(np.int64)[_gather(label.astype(np.int64), ny, nx, 0)],
                                ignore_label)
    if regs is not None:
        out['regs'] = _gather(regs.astype(np.int64), ny, nx, 0)[None]
    if soft is not None:
        out['soft'] = np.stack([sum(wk.astype(np.float64) * _gather(p.astype(np.float64), ty, tx, 0.0)
                                    for wk, (ty, tx) in zip(w, taps)) / 65536.0 for p in soft])
    return out


def augment(img, params, size, lut, label=None, label_lut=None, ignore_label=-1, soft=None, regs=None):
    """The kernel's outputs for numpy inputs of N samples; a row that fails the row check gives None in every list.
    -> {name: [per-sample array or None]}."""
    res = {}
    for n in range(img.shape[0]):
        one = None
        if row_valid(params[n], img.shape[1], img.shape[2]):
            one = warp_one(params[n], size, img[n], lut, None if label is None else label[n], label_lut, ignore_label,
                           None if soft is None else soft[n], None if regs is None else regs[n])
        for k in ('image', 'byte', 'label', 'soft', 'regs', 'inframe', 'exact'):
            res.setdefault(k, []).append(None if one is None else one.get(k))
    return res
