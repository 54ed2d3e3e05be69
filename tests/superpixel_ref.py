"""CPU restatement of rgda_superpixels / rgda_region_shrink (include/rgda_hip.h) in plain numpy: the integer SLIC of the
specification there (vectorised Assign and Update), the 4-connected components by iterated minimum propagation with the
min-index root rule, and edge_shrinking as a window test.  Used by tests/test_superpixels_*.py and
scripts/dev/superpixel_bench.py.

The superpixel algorithm is this project's own (it stands in for the reference's third-party LSC / SLIC generators and
reproduces neither); `shrink` restates the reference's own edge_shrinking (regda/gast/superpixels.py:129-152) and is
checked against a golden minted from that loop (tests/golden/edge_shrink.npz)."""
import numpy as np


def update(img, labels, S, prev=None):
    """Update(labels) -> centres int64 [K][5] (cy, cx, cr, cg, cb); a centre without pixels keeps prev[k]."""
    H, W, _ = img.shape
    K = (H // S) * (W // S)
    yy, xx = np.mgrid[0:H, 0:W]
    comp = np.stack([yy, xx, img[..., 0], img[..., 1], img[..., 2]], -1).reshape(-1, 5).astype(np.int64)
    lab = labels.reshape(-1)
    n = np.bincount(lab, minlength=K).astype(np.int64)
    sums = np.stack([np.bincount(lab, weights=comp[:, c], minlength=K) for c in range(5)], -1).astype(np.int64)
    out = np.zeros((K, 5), np.int64) if prev is None else prev.copy()
    has = n > 0
    out[has] = (2 * sums[has] + n[has, None]) // (2 * n[has, None])
    return out


def grid_labels(H, W, S):
    yy, xx = np.mgrid[0:H, 0:W]
    return (yy // S) * (W // S) + xx // S


def assign(img, centres, S, m):
    """Assign(centres) -> labels int64 [H][W]: least d among the <= 9 neighbouring cells' centres, ties to the smaller k."""
    H, W, _ = img.shape
    Gy, Gx = H // S, W // S
    yy, xx = np.mgrid[0:H, 0:W]
    gy, gx = yy // S, xx // S
    px = img.astype(np.int64)
    best_d = np.full((H, W), np.iinfo(np.int64).max)
    best_k = np.full((H, W), -1, np.int64)
    for a in (-1, 0, 1):                    # ascending k: a strict `<` keeps the smaller k on equal d
        for b in (-1, 0, 1):
            cy, cx = gy + a, gx + b
            ok = (cy >= 0) & (cy < Gy) & (cx >= 0) & (cx < Gx)
            k = np.where(ok, cy * Gx + cx, 0)
            c = centres[k]
            d = ((px - c[..., 2:5]) ** 2).sum(-1) * S * S + m * m * ((yy - c[..., 0]) ** 2 + (xx - c[..., 1]) ** 2)
            # the kernel's int32 arithmetic (include/rgda_hip.h), over the candidates that exist: a slot outside the
            # grid stands in as centre 0 here, is never taken and is never computed by the kernel
            assert not ok.any() or d[ok].max() < 2 ** 31
            take = ok & (d < best_d)
            best_d = np.where(take, d, best_d)
            best_k = np.where(take, k, best_k)
    return best_k


def slic_labels(img, S, m, iters):
    """-> (labels [H][W] of the last Assign, the centres that Assign used)."""
    H, W, _ = img.shape
    centres = update(img, grid_labels(H, W, S), S)
    for it in range(1, iters + 1):
        labels = assign(img, centres, S, m)
        if it < iters:
            centres = update(img, labels, S, centres)
    return labels, centres


def components(labels):
    """-> root [H][W]: the smallest linear pixel index of each pixel's 4-connected component of equal labels."""
    H, W = labels.shape
    root = np.arange(H * W, dtype=np.int64).reshape(H, W)
    same_l = labels[:, 1:] == labels[:, :-1]
    same_u = labels[1:, :] == labels[:-1, :]
    big = np.int64(H * W)
    while True:
        new = root.copy()
        for _ in range(8):                  # a few sweeps of each direction per convergence check
            new[:, 1:] = np.minimum(new[:, 1:], np.where(same_l, new[:, :-1], big))
            new[:, :-1] = np.minimum(new[:, :-1], np.where(same_l, new[:, 1:], big))
            new[1:, :] = np.minimum(new[1:, :], np.where(same_u, new[:-1, :], big))
            new[:-1, :] = np.minimum(new[:-1, :], np.where(same_u, new[1:, :], big))
        new = new.reshape(-1)[new.reshape(-1)].reshape(H, W)      # a pixel's root's root: pointer jumping
        if np.array_equal(new, root):
            return root
        root = new


def number(root, min_area):
    """Roots -> (regs int32 [H][W], R): components below min_area become 0, the others 1..R in increasing root order."""
    flat = root.reshape(-1)
    area = np.bincount(flat, minlength=flat.size)
    kept = np.flatnonzero(area >= min_area)                       # increasing root order
    ids = np.zeros(flat.size, np.int32)
    ids[kept] = np.arange(1, kept.size + 1, dtype=np.int32)
    return ids[flat].reshape(root.shape), int(kept.size)


def superpixels(img, S=16, m=10, iters=10, min_area=None):
    """One image uint8 [H][W][3] -> (regs int32 [H][W], R)."""
    img = np.asarray(img)
    min_area = S * S // 4 if min_area is None else min_area
    labels, _ = slic_labels(img, S, m, iters)
    return number(components(labels), min_area)


def shrink(regs, win=3, fill=0):
    """edge_shrinking: regs [H][W] -> regs where the (2 win + 1)^2 window inside the image holds one id, `fill` elsewhere."""
    H, W = regs.shape
    keep = np.ones((H, W), bool)
    for dy in range(-win, win + 1):
        for dx in range(-win, win + 1):
            ys, ye = max(0, -dy), min(H, H - dy)
            xs, xe = max(0, -dx), min(W, W - dx)
            if ys >= ye or xs >= xe:
                continue
            keep[ys:ye, xs:xe] &= regs[ys:ye, xs:xe] == regs[ys + dy:ye + dy, xs + dx:xe + dx]
    return np.where(keep, regs, fill).astype(regs.dtype)


def reference_fill(H, W, region_size=16):
    """edge_shrinking's own fill value (superpixels.py:131)."""
    return int(H / region_size * W / region_size)


# ---- seeded test images (shared by the CPU and GPU tests and scripts/dev/superpixel_bench.py)
def diagonal_image(H=64, W=64):
    """Two flat colours split by the diagonal."""
    yy, xx = np.mgrid[0:H, 0:W]
    return np.where((xx * H > yy * W)[..., None], np.array([200, 60, 30]), np.array([20, 90, 160])).astype(np.uint8)


def blurred_noise(H, W, seed):
    """uint8 noise under a 3 x 3 box filter (edges replicated): smooth enough for SLIC to move, rough enough that the
    labels fragment into small components."""
    rng = np.random.default_rng(seed)
    x = np.pad(rng.integers(0, 256, (H, W, 3)).astype(np.int64), ((1, 1), (1, 1), (0, 0)), mode='edge')
    acc = sum(x[dy:dy + H, dx:dx + W] for dy in range(3) for dx in range(3))
    return (acc // 9).astype(np.uint8)


def rectangle_scene(H, W, seed, count=40, noise=6):
    """A synthetic tile: `count` flat rectangles over a flat ground, plus mild uniform noise."""
    rng = np.random.default_rng(seed)
    img = np.empty((H, W, 3), np.int64)
    img[:] = rng.integers(40, 200, 3)
    for _ in range(count):
        h, w = rng.integers(H // 16, H // 3), rng.integers(W // 16, W // 3)
        y, x = rng.integers(0, H - h), rng.integers(0, W - w)
        img[y:y + h, x:x + w] = rng.integers(0, 256, 3)
    img += rng.integers(-noise, noise + 1, img.shape)
    return np.clip(img, 0, 255).astype(np.uint8)
