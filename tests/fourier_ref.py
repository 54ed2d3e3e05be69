"""The Fourier style transfer of the source tile (include/rgda_hip.h: rgda_fourier_style) restated in fp64 numpy from its
written contract, through numpy.fft -- the full-FFT form, which is deliberately NOT the kernel's algorithm -- and the
forward error bound of an fp32 evaluation of the kernel's form.

The contract, per channel on the raw grey scale: S = x_s std_s + mean_s, T = x_t std_t + mean_t of the row's partner;
F_S = fft2(S), F_T = fft2(T); on every signed frequency pair with |ky| <= b and |kx| <= b the amplitude |F_S| becomes
|F_T| and the phase of F_S is kept (phase 0 where |F_S| is exactly 0); out = (Re ifft2(.) - mean_s) / std_s.  A row with
on == 0 returns the image as it is.  mean, std are taken as the fp32 values the entry point receives.

`pruned` is the kernel's form, out_raw = S + (1 / HW) Re sum_k D(k) e^{+2 pi i (ky y / H + kx x / W)} with
D(k) = (|F_T(k)| - |F_S(k)|) F_S(k) / |F_S(k)|, as four one-dimensional passes over kx in [0, b] and ky in [-b, b]; in
float32 it sums in the kernel's order (`ordered_sum`: each of 64 lanes adds its own terms l, l + 64, ... in sequence, then
six pairwise levels join the lanes; the synthesis passes add 4 and 2 interleaved sequences).

The bound (`fourier_ref(..., bound=True)`), per element, in the units of the result.  It is NOT a worst-case bound.  With
all roundings aligned, (2b + 1)^2 bins that each carry an analysis error of order u ||S||_1 give about 1 grey level at
b = 64, two orders above what any fp32 evaluation shows, and nothing could be told from a wrong bin, which moves pixels by
about as much.  The model instead: every rounding is an independent, zero-mean error of at most u |v|, u = 2^-24, v the
rounded value, so of variance at most u^2 v^2 / 3; variances add along the computation; the bound is LAMBDA = 6 standard
deviations (each output element sums thousands of such errors: Gaussian tails, 2e-9 per element beyond 6) plus the last
four roundings at their worst case.  The roundings, pass by pass:
  rows      R[y][kx] = sum_x S[y][x] tw: per term the rounding of S, of the twiddle (fp64 sincospi of the integer-reduced
            phase, rounded once), of the product and of the partial sum it joins -- 5 events of at most
            u (|partial before| + |term|), which covers a fused and an unfused multiply-add; then one event per node of
            the six joining levels, u |node|.  The partial sums are those of the fp64 run in the kernel's order.
  columns   F[ky][kx] = sum_y R[y][kx] tw: the same count on its own terms, plus the variances of the R it reads.
  D(k)      D = |F_T| e^{i phi_S} - F_S, so |dD| <= (1 + rho) |dF_S| + |dF_T| with rho = |F_T(k)| / |F_S(k)|, THE
            CONDITIONING TERM OF THE PHASE (a small |F_S| turns an analysis error into a large phase error of an amplitude
            |F_T|); 6 roundings of its own (two moduli, difference, quotient, product, scale) of at most u (|F_T| + |F_S|).
            The factor (kx ? 2 : 1) / HW that lets the half spectrum stand for both halves scales D and its error.
  synthesis G[y][kx] = sum_ky D tw in 4 interleaved sequences, then corr[y][x] = sum_kx Re(G tw) in 2: per term 7 events
            (the sum and difference of the +ky / -ky pair, the twiddle, two multiply-adds unfused) of at most
            u A, A the sum of the magnitudes of all terms of that sum; with p the events on the longest path
            (7 ceil(b / 4) + 2, 7 ceil((b + 1) / 2) + 1) the variance is at most p u^2 A^2 / 3.
  last      s = x std + mean, s + corr, - mean, / std: u (|S| + |raw| + 2 |raw - mean|) / std, worst case.
Where |F_S(k)| = 0 on a bin of the window the bound is infinite: the phase is then a convention, not a number with an
error.  tests/test_fourier_cpu.py asserts rho <= 256 and a bound of at most 0.05 grey levels on every GPU case."""
import numpy as np

U = 2.0 ** -24
LAMBDA = 6.0
LANES = 64
MEAN = (123.675, 116.28, 103.53)
STD = (58.395, 57.12, 57.375)
MEAN_T = (85.1, 91.7, 84.9)         # a second normalisation (the configs' SRC_MEAN / SRC_STD pattern), for the tests
STD_T = (35.8, 35.2, 36.5)


def f64(v):
    """three values as the fp32 numbers the entry point receives, [3][1][1] fp64"""
    return np.asarray(v, np.float32).astype(np.float64)[:, None, None]


def signed_freq(n):
    """the signed frequency of every fft bin of a length-n axis: 0, 1, ..., -2, -1"""
    k = np.arange(n)
    return np.where(k > (n - 1) // 2, k - n, k) if n % 2 else np.where(k >= n // 2, k - n, k)


def window(h, w, b):
    """bool [h][w]: the bins with |ky| <= b and |kx| <= b (the published [c - b, c + b] of the shifted spectrum)"""
    return (np.abs(signed_freq(h))[:, None] <= b) & (np.abs(signed_freq(w))[None, :] <= b)


def swap(S, T, b):
    """S, T fp64 [H][W] -> (the raw result through the full FFT, the largest imaginary part of the inverse transform)"""
    fs, ft = np.fft.fft2(S), np.fft.fft2(T)
    a = np.abs(fs)
    phase = np.where(a == 0.0, 1.0, fs / np.where(a == 0.0, 1.0, a))
    res = np.fft.ifft2(np.where(window(*S.shape, b), np.abs(ft) * phase, fs))
    return res.real, float(np.abs(res.imag).max())


def twiddles(k, n, sign, dtype=np.float64):
    """e^{sign 2 pi i (k x mod n) / n} [len(k)][n]: the phase index reduced in integers, fp64, then rounded to `dtype`"""
    p = (np.asarray(k)[:, None] * np.arange(n)[None, :]) % n
    ang = 2.0 * np.pi * p / n
    c = np.complex64 if dtype == np.float32 else np.complex128
    return (np.cos(ang) + sign * 1j * np.sin(ang)).astype(c)


def ordered_sum(terms, events=None):
    """sum over the last axis in the analysis kernels' order: lane l adds terms l, l + 64, ... in sequence, six pairwise
    levels join the lanes (level t joins the lanes that agree modulo 64 >> t).  In the dtype of `terms`.  events: a list
    that receives the array of sum |partial before| + |term| squared over the sequence, and sum |node|^2 over the levels."""
    n = terms.shape[-1]
    j = -(-n // LANES)
    pad = np.zeros(terms.shape[:-1] + (j * LANES - n,), terms.dtype)
    t = np.concatenate([terms, pad], -1).reshape(terms.shape[:-1] + (j, LANES))
    part = np.cumsum(t, axis=-2, dtype=terms.dtype)
    lanes = part[..., -1, :]
    ev_seq = ev_tree = 0.0
    if events is not None:
        before = np.abs(part)
        before = np.concatenate([np.zeros_like(before[..., :1, :]), before[..., :-1, :]], -2)
        ev_seq = ((before + np.abs(t)) ** 2).sum((-1, -2))
    for lvl in range(1, 7):
        lanes = lanes.reshape(lanes.shape[:-1] + (2, LANES >> lvl))
        lanes = lanes[..., 0, :] + lanes[..., 1, :]
        if events is not None:
            ev_tree = ev_tree + (np.abs(lanes) ** 2).sum(-1)
    if events is not None:
        events.extend([ev_seq, ev_tree])
    return lanes[..., 0]


def interleaved_sum(terms, ways, first=None):
    """sum over the last axis in the synthesis kernels' order: `ways` sequences of every ways-th term (the first of them
    starting from `first`), joined pairwise.  In the dtype of `terms`."""
    acc = []
    for u in range(ways):
        t = terms[..., u::ways]
        if u == 0 and first is not None:
            t = np.concatenate([first[..., None], t], -1)
        acc.append(np.cumsum(t, axis=-1, dtype=terms.dtype)[..., -1] if t.shape[-1] else np.zeros(terms.shape[:-1], terms.dtype))
    while len(acc) > 1:
        acc = [acc[i] + acc[i + 1] for i in range(0, len(acc), 2)]
    return acc[0]


def analysis(X, b, dtype=np.float64, var=False):
    """X [H][W] -> F [2b + 1][b + 1] (ky = -b..b, kx = 0..b) as the kernel's two passes (and, with `var`, the model
    variance of every F in units of u^2 / 3)."""
    h, w = X.shape
    X = X.astype(dtype)
    ex = twiddles(np.arange(b + 1), w, -1, dtype)                           # [kx][x]
    ey = twiddles(np.arange(-b, b + 1), h, -1, dtype)                       # [ky][y]
    ev = [] if var else None
    R = ordered_sum(X[:, None, :] * ex[None, :, :], ev)                     # [y][kx]
    v_rows = 5.0 * ev[0] + ev[1] if var else None
    ev = [] if var else None
    F = ordered_sum(ey[:, None, :] * R.T[None, :, :], ev)                   # [ky][kx]
    if not var:
        return F
    return F, 5.0 * ev[0] + ev[1] + v_rows.sum(0)[None, :]


def pruned(S, T, b, dtype=np.float64, var=False):
    """S, T [H][W] -> the raw result in the kernel's form, in `dtype` arithmetic (float32: in the kernel's order of
    summation; and, with `var`, the model variance of the correction in units of u^2 / 3, [H][1])."""
    h, w = S.shape
    c = np.complex64 if dtype == np.float32 else np.complex128
    fs, ft = analysis(S, b, dtype, var), analysis(T, b, dtype, var)
    if var:
        (fs, vs), (ft, vt) = fs, ft
    a_s, a_t = np.abs(fs), np.abs(ft)
    scale = (np.where(np.arange(b + 1) > 0, 2.0, 1.0) * dtype(1.0 / (h * w))).astype(dtype)[None, :]
    safe = np.where(a_s > 0, a_s, 1).astype(dtype)
    D = (np.where(a_s > 0, ((a_t - a_s) / safe) * fs, a_t) * scale).astype(c)          # [ky][kx]
    ey = twiddles(np.arange(1, b + 1), h, +1, dtype)                                    # [ky > 0][y]
    p, q = D[b + 1:], D[:b][::-1]                                                       # +ky and -ky, ky = 1..b
    pairs = (p + q).real[:, :, None] * ey.real[:, None, :] - (p - q).imag[:, :, None] * ey.imag[:, None, :] \
        + 1j * ((p + q).imag[:, :, None] * ey.real[:, None, :] + (p - q).real[:, :, None] * ey.imag[:, None, :])
    pairs = np.moveaxis(pairs.astype(c), 0, -1)                                         # [kx][y][ky]
    G = interleaved_sum(pairs, 4, first=np.broadcast_to(D[b][:, None], (b + 1, h)).astype(c))       # [kx][y]
    ex = twiddles(np.arange(b + 1), w, +1, dtype)                                       # [kx][x]
    terms = G.T[:, None, :].real * ex.T[None, :, :].real - G.T[:, None, :].imag * ex.T[None, :, :].imag       # [y][x][kx]
    corr = interleaved_sum(terms.astype(dtype), 2)
    raw = S.astype(dtype) + corr
    if not var:
        return raw
    rho = a_t / np.where(a_s > 0, a_s, 1)
    with np.errstate(divide='ignore', invalid='ignore'):
        v_d = np.where(a_s > 0, (1.0 + rho) ** 2 * vs + vt + 6.0 * (a_t + a_s) ** 2, np.inf) * scale ** 2
    a_col = np.abs(D).sum(0)                                                            # [kx]: sum over ky of |D|
    v_g = (7 * -(-b // 4) + 2) * a_col ** 2                                             # every y alike
    a_row = np.abs(G).sum(0)                                                            # [y]: sum over kx of |G|
    v_corr = v_d.sum() + v_g.sum() + (7 * -(-(b + 1) // 2) + 1) * a_row ** 2
    return raw, v_corr[:, None]


def fourier_ref(xs, xt, table, mean_s=MEAN, std_s=STD, mean_t=MEAN, std_t=STD, bound=False):
    """xs f32 [N][3][H][W], xt f32 [M][3][H][W], table int32 [N][4] -> fp64 [N][3][H][W] through the full FFT (and, with
    `bound`, the per-element error bound of the module docstring, in the units of the result)."""
    xs, xt = np.asarray(xs), np.asarray(xt)
    table = np.asarray(table, np.int64)
    ms, ss, mt, st = f64(mean_s), f64(std_s), f64(mean_t), f64(std_t)
    out = xs.astype(np.float64)
    err = np.zeros(out.shape)
    for n in range(xs.shape[0]):
        partner, b, on = (int(v) for v in table[n, :3])
        if not on:
            continue                                    # the image as it is; the bound stays 0
        assert 0 <= partner < xt.shape[0] and 0 <= b <= 64 and 2 * b + 1 <= min(xs.shape[-2:])
        S = xs[n].astype(np.float64) * ss + ms
        T = xt[partner].astype(np.float64) * st + mt
        for ch in range(3):
            raw, imag = swap(S[ch], T[ch], b)
            assert imag < 1e-9                          # the result is real: the window is symmetric
            out[n, ch] = (raw - ms[ch]) / ss[ch]
            if bound:
                _, v = pruned(S[ch], T[ch], b, var=True)
                last = U * (np.abs(S[ch]) + np.abs(raw) + 2.0 * np.abs(raw - ms[ch]))
                err[n, ch] = (LAMBDA * U * np.sqrt(v / 3.0) + last) / ss[ch]
    return (out, err) if bound else out


def conditioning(xs, xt, table, mean_s=MEAN, std_s=STD, mean_t=MEAN, std_t=STD):
    """the largest |F_T(k)| / |F_S(k)| over the windows of all rows that are on"""
    worst = 0.0
    for n in range(xs.shape[0]):
        partner, b, on = (int(v) for v in table[n, :3])
        if on:
            S = xs[n].astype(np.float64) * f64(std_s) + f64(mean_s)
            T = xt[partner].astype(np.float64) * f64(std_t) + f64(mean_t)
            m = window(*S.shape[-2:], b)
            worst = max(worst, float((np.abs(np.fft.fft2(T))[:, m] / np.abs(np.fft.fft2(S))[:, m]).max()))
    return worst
