"""The strong augmentation of the student's tile (include/rgda_hip.h: rgda_strong_augment) restated in fp64 numpy from
its written contract, and the forward error bound of an fp32 evaluation of that contract.

The contract: x f32 [N][3][H][W] holds v = (raw - mean_c) / std_c; row n of the table is {fb, fc, fs, theta, sigma, flags,
0, 0}, flags bit 0 "jitter", bit 1 "blur".  Both bits clear: the image is returned as it is.  Otherwise
u = (v std_c + mean_c) / 255 and, with clamp = clamp to [0, 1],
  1. u <- clamp(u fb)
  2. m = mean over the image of grey(u) = 0.299 r + 0.587 g + 0.114 b;  u <- clamp((u - m) fc + m)
  3. g = grey(u) per pixel;  u <- clamp((u - g) fs + g)
  4. u <- clamp(M u), M = T^-1 R(theta) T (YIQ)
  5. (bit 1) separable Gaussian, radius R = ceil(3 sigma), taps exp(-d^2 / (2 sigma^2)) normalised, rows then columns,
     reflection without the edge pixel
  6. v' = (255 u - mean_c) / std_c
with 1 to 4 only under bit 0.  mean, std and the table are taken as the fp32 values the entry point receives.

The bound (`strong_ref(..., bound=True)`), per element, for an evaluation that rounds every operation to fp32:
    ( K eps Mmax + |fc - 1| m_err ) 255 / std_c,     eps = 2^-24,
K the roundings on the element's longest dependency path, Mmax the largest magnitude (in units of u) of an intermediate
on that path in the fp64 run.  With j, b the two bits:
    K = 6 + 15 j + (4 R + 4) b
      3   v std, + mean, / 255
      1   u fb                                                      (j)
      3   u - m, (.) fc, + m                                        (j)
      7   grey: a coefficient's own rounding, its product, two sums (the coefficients add up to 1, so the three
          branches together err by no more than one path of 4 at the largest magnitude); u - g, (.) fs, + g    (j)
      4   hue: an entry of M rounded once, its product, two sums; Mmax covers sum_j |M_ij u_j|                  (j)
      2R+2 per blur pass: a tap rounded once, its product, 2R additions of partial sums that the positive,
          normalised taps keep below the largest input; two passes                                          (b)
      3   255 u, - mean, / std
The clamps are exact and never expand an error.  m_err, the error of the image mean of step 2 when every grey value is
evaluated in fp32 (3 + 1 + 4 roundings), rounded to a multiple of 2^-24 (half a quantum, 2^-25, each), summed exactly
and the mean rounded once to fp32:   m_err = 9 eps Mg + 2^-25,  Mg the largest magnitude on the grey path over the image.
Under a blur an element's path runs through the (2R + 1)^2 window around it: Mmax is the window's maximum."""
import numpy as np

EPS = 2.0 ** -24
GREY = np.array([0.299, 0.587, 0.114])
T_YIQ = np.array([[0.299, 0.587, 0.114], [0.596, -0.274, -0.322], [0.211, -0.523, 0.312]])
MEAN = (123.675, 116.28, 103.53)
STD = (58.395, 57.12, 57.375)


def radius(sigma):
    """R = ceil(3 sigma), the product in fp32"""
    return int(np.ceil(np.float32(3.0) * np.float32(sigma)))


def taps(sigma, R):
    d = np.arange(-R, R + 1, dtype=np.float64)
    w = np.exp(-d * d / (2.0 * float(sigma) ** 2))
    return w / w.sum()


def hue_matrix(theta):
    c, s = np.cos(float(theta)), np.sin(float(theta))
    rot = np.array([[1.0, 0.0, 0.0], [0.0, c, -s], [0.0, s, c]])
    return np.linalg.inv(T_YIQ) @ rot @ T_YIQ


def reflect_index(n, R):
    """(n, 2R + 1) source indices of the taps of every position: -1 -> 1, n -> n - 2"""
    i = np.arange(n)[:, None] + np.arange(-R, R + 1)[None, :]
    i = np.abs(i)
    return np.where(i >= n, 2 * (n - 1) - i, i)


def blur(u, sigma):
    """u [3][H][W] -> rows, then columns"""
    R = radius(sigma)
    t = taps(sigma, R)
    h = (u[:, :, reflect_index(u.shape[2], R)] * t).sum(-1)
    return (h[:, reflect_index(u.shape[1], R), :] * t[None, None, :, None]).sum(2)


def window_max(a, R):
    """a [H][W] -> the maximum over the reflected (2R + 1)^2 window of every position"""
    h = a[:, reflect_index(a.shape[1], R)].max(-1)
    return h[reflect_index(a.shape[0], R), :].max(1)


def jitter_steps(u, fb, fc, fs, theta, clamp=True, mag=None, pre=None):
    """Steps 1 to 4 on u [3][H][W]; `mag` (a list) collects the magnitudes of the intermediates, each [H][W] or [3][H][W],
    `pre` (a list) the four arrays as they stand before the clamp of each step.  -> (u, m)"""
    def cl(a):
        if pre is not None:
            pre.append(a)
        return np.clip(a, 0.0, 1.0) if clamp else a
    note = (lambda *a: mag.extend(np.abs(x) for x in a)) if mag is not None else (lambda *a: None)
    b = u * fb
    note(b)
    u = cl(b)
    note((np.abs(u) * GREY[:, None, None]).sum(0))
    m = float((u * GREY[:, None, None]).sum(0).mean())
    d = u - m
    note(d, d * fc, d * fc + m)
    u = cl(d * fc + m)
    g = (u * GREY[:, None, None]).sum(0)
    note((np.abs(u) * GREY[:, None, None]).sum(0))
    d = u - g
    note(d, d * fs, d * fs + g)
    u = cl(d * fs + g)
    M = hue_matrix(theta)
    note(np.einsum('ij,jhw->ihw', np.abs(M), np.abs(u)))
    u = cl(np.einsum('ij,jhw->ihw', M, u))
    return u, m


def strong_ref(x, table, mean=MEAN, std=STD, bound=False):
    """x f32 [N][3][H][W], table f32 [N][8] -> fp64 [N][3][H][W] (and, with `bound`, the per-element error bound of the
    module docstring, in the units of the result)."""
    x = np.asarray(x)
    table = np.asarray(table, np.float32)
    mean = np.asarray(mean, np.float32).astype(np.float64)[:, None, None]
    std = np.asarray(std, np.float32).astype(np.float64)[:, None, None]
    out = x.astype(np.float64)
    err = np.zeros(out.shape)
    for n in range(x.shape[0]):
        fb, fc, fs, theta, sigma = (float(v) for v in table[n, :5])
        flags = int(table[n, 5])
        j, b = flags & 1, (flags >> 1) & 1
        if not flags:
            continue                                    # the image as it is; the bound stays 0
        v = x[n].astype(np.float64)
        mag = [np.abs(v * std) / 255.0, np.abs(v * std + mean) / 255.0]
        u = (v * std + mean) / 255.0
        mag.append(np.abs(u))
        m_err = 0.0
        if j:
            grey_mag = max(float(np.max(a)) for a in mag)
            grey_mag = max(grey_mag, float(np.abs(u * fb).max()))
            m_err = 9 * EPS * grey_mag + 2.0 ** -25
            u, _ = jitter_steps(u, fb, fc, fs, theta, mag=mag)
            mag.append(np.abs(u))
        path = np.zeros(u.shape[1:])
        for a in mag:                                   # per pixel, over the three channels: steps 3 and 4 join them
            path = np.maximum(path, a if a.ndim == 2 else a.max(0))
        R = 0
        if b:
            R = radius(sigma)
            assert 0.0 < sigma <= 4.0 and R < u.shape[1] and R < u.shape[2]
            path = window_max(path, R)
            u = blur(u, sigma)
        res = (255.0 * u - mean) / std
        last = np.maximum(np.abs(u), np.maximum(np.abs(255.0 * u - mean) / 255.0, np.abs(res) * std / 255.0))
        K = 6 + 15 * j + (4 * R + 4) * b
        err[n] = (K * EPS * np.maximum(path[None], last) + abs(fc - 1.0) * m_err * j) * 255.0 / std
        out[n] = res
    return (out, err) if bound else out
