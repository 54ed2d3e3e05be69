"""The contract of rgda_hist_style (include/rgda_hip.h) restated in numpy and Python integers: per-channel histogram
matching of normalised source tiles to a partner target tile, blended by blend_q / 65536.

The counts, prefix sums and the interpolation's numerator and denominator are Python integers; one fp64 division and one
fp64 addition give the matched level L[v], one fp64 product and division, rounded to fp32 once, the correction D[v].
Python's float is IEEE binary64 and its / is correctly rounded, so L is the kernel's L bit for bit.

Grey levels: the kernel computes rintf(fmaf(x, std, mean)) in fp32; here the same expression is evaluated in fp64 from the
fp32 operands.  The two can round to different levels only where the raw value lies within about 1e-4 of a half; the
inputs the tests make (`tiles`) keep |frac - 0.5| >= 0.1."""
import numpy as np

MEAN = (123.675, 116.28, 103.53)
STD = (58.395, 57.12, 57.375)
MEAN_T = (85.1, 91.7, 84.9)         # a second normalisation (the configs' SRC_MEAN / SRC_STD pattern), for the tests
STD_T = (35.8, 35.2, 36.5)
BLEND_ONE = 65536                   # RGDA_HIST_BLEND_ONE


def f32(v):
    return np.asarray(v, np.float32)


def tiles(levels, mean, std, noise=None):
    """uint8 levels (n, 3, h, w) -> the normalised fp32 tile a loader would hand over: (level - mean) / std in fp32.
    noise: sub-level offsets of |.| <= 0.4 added on the grey scale first."""
    raw = levels.astype(np.float32)
    if noise is not None:
        assert np.abs(noise).max() <= 0.4
        raw = raw + noise.astype(np.float32)
    return ((raw - f32(mean)[:, None, None]) / f32(std)[:, None, None]).astype(np.float32)


def levels_of(x, mean, std):
    """v(x) = clamp(rint(x std + mean), 0, 255) of an fp32 tile (n, 3, h, w) -> int64"""
    raw = x.astype(np.float64) * f32(std).astype(np.float64)[:, None, None] + f32(mean).astype(np.float64)[:, None, None]
    return np.clip(np.rint(raw), 0, 255).astype(np.int64)


def histogram(v):
    """the 256 counts of an integer plane, as Python integers"""
    return [int(c) for c in np.bincount(np.asarray(v).ravel(), minlength=256)]


def match_lut(hs, ht):
    """L[256] (Python floats, fp64) of a source histogram hs and a target histogram ht of the same total"""
    assert sum(hs) == sum(ht) > 0
    cs, ct, a, b = [], [], 0, 0
    for v in range(256):
        a, b = a + hs[v], b + ht[v]
        cs.append(a)
        ct.append(b)
    u = [v for v in range(256) if ht[v] > 0]
    k = len(u)
    L = [float(v) for v in range(256)]
    for v in range(256):
        if hs[v] == 0:
            continue
        below = [j for j in range(k) if ct[u[j]] <= cs[v]]
        if not below:
            L[v] = float(u[0])
        elif below[-1] == k - 1:
            L[v] = float(u[k - 1])
        else:
            j = below[-1]
            num = (cs[v] - ct[u[j]]) * (u[j + 1] - u[j])
            den = ct[u[j + 1]] - ct[u[j]]
            assert 0 <= num < 2 ** 32 and 0 < den < 2 ** 32
            L[v] = float(u[j]) + float(num) / float(den)
    return L


def correction(L, blend_q, std):
    """D[256] fp32 = (float)(beta (L[v] - v) / (double)std), beta = blend_q / 65536"""
    beta = float(blend_q) / float(BLEND_ONE)
    s = float(np.float32(std))
    return np.array([np.float32(beta * (L[v] - float(v)) / s) for v in range(256)], np.float32)


def hist_ref(xs, xt, table, mean_s=MEAN, std_s=STD, mean_t=MEAN, std_t=STD):
    """-> (out fp32 (n, 3, h, w), hist int64 (n + m, 3, 256), lut fp64 (n, 3, 256)) of fp32 tiles xs (n, 3, h, w), xt
    (m, 3, h, w) and the int32 rows {partner, blend_q, on, 0}.  A row that is off is the source as it is, its lut the
    identity."""
    n, m = xs.shape[0], xt.shape[0]
    vs, vt = levels_of(xs, mean_s, std_s), levels_of(xt, mean_t, std_t)
    hist = np.array([[histogram(v[i, c]) for c in range(3)] for v in (vs, vt) for i in range(v.shape[0])], np.int64)
    lut = np.tile(np.arange(256, dtype=np.float64), (n, 3, 1))
    out = xs.copy()
    for i in range(n):
        p, q, on = (int(t) for t in table[i, :3])
        if not on:
            continue
        assert 0 <= p < m and 0 <= q <= BLEND_ONE
        for c in range(3):
            L = match_lut(hist[i, c].tolist(), hist[n + p, c].tolist())
            lut[i, c] = L
            D = correction(L, q, std_s[c])
            out[i, c] = xs[i, c] + D[vs[i, c]]          # one fp32 addition
    assert out.dtype == np.float32
    return out, hist, lut
