"""The stage-2 loss kernels of regda_amd/csrc/align_kernels.hip (PrototypeContrastiveLoss forward + feature gradient) and
the ASPP head kernels of regda_amd/csrc/aspp_kernels.hip (gather, scatter, dbias): a Python restatement of the host-side
decisions, a table of small cases that each name the path they are there to reach, and plain numpy references.

The restatement mirrors the two .hip files; tests/test_align_cases_cpu.py parses the constants it copies out of the
sources, so a change there that is not made here fails on a machine without a GPU.

References: the PCL loss and gradient are written out in fp64 from the fp32 inputs (normalise with the max(norm, 1e-12)
clamp, logits, log-softmax, mean over the kept pixels, the closed-form gradient); the ASPP gather is an fp32 sum in the
kernel's own order (it has one right answer per element: no multiply to contract, no fast-math), the scatter is a
round-to-nearest-even copy done on the bits, dbias an fp64 sum.

Inputs are built on the CPU from fixed seeds; nothing here needs a GPU or the library.
"""
import zlib
from collections import namedtuple

import numpy as np

# ---------------------------------------------------------------- the restatement (align_kernels.hip, common.h)
MIN_CLASSES, MAX_CLASSES = 6, 16     # RGDA_MIN_CLASSES / RGDA_MAX_CLASSES
PX = 32                              # pixels per workgroup of pcl_kernel
KC = 128                             # channels per transposed store chunk of pass 2
K_MIN, K_MAX = 8, 4096               # K a multiple of 8 (16-byte bf16 rows)
LDS_MAX = 160 * 1024                 # RGDA_LDS_MAX
LDS_ATTR = 64 * 1024                 # above: hipFuncAttributeMaxDynamicSharedMemorySize is set before the launch
FLAG_LABEL, FLAG_NONFINITE = 4, 8    # bit 2: a label outside [0, C) that is not ignore; bit 3: a poisoned loss partial
OK, ERR_ARG, ERR_WORKSPACE, ERR_LAUNCH, ERR_UNSUPPORTED = 0, -1, -2, -3, -4


def cdiv(a, b):
    return -(-a // b)


def align256(x):
    return (x + 255) & ~255


def pcl_slices(C):
    return 16 if C <= 14 else 8


def pcl_kper(C, K):
    return cdiv(K, pcl_slices(C))


def pcl_lds(C, K):
    return (C * K + pcl_slices(C) * PX * (C + 1) + PX * (C + 1)) * 4 + PX * (KC + 8) * 2


def pcl_workspace(C, K):
    return align256(C * K * 4) + 256


def pcl_flag_offset(C, K):
    """Byte offset of the int32 flag word: pn[C][K] padded to 256 B | count | flag | loss total."""
    return align256(C * K * 4) + 4


def pcl_status(C, K, lddf=None, ws_bytes=None):
    """What rgda_pcl_loss answers for (C, K, lddf) with good pointers and b, h, w, temperature > 0; lddf None: no dfeat."""
    if not MIN_CLASSES <= C <= MAX_CLASSES:
        return ERR_UNSUPPORTED
    if K < K_MIN or K > K_MAX or K & 7:
        return ERR_ARG
    if lddf is not None and (lddf & 7 or lddf < K):
        return ERR_ARG
    if pcl_lds(C, K) > LDS_MAX:
        return ERR_UNSUPPORTED
    if ws_bytes is not None and ws_bytes < pcl_workspace(C, K):
        return ERR_WORKSPACE
    return OK


def pcl_slice_shapes(C, K):
    """Per k-slice of pass 1: (terms in the 4-way unrolled sum, terms in its tail); (0, 0) is an empty slice."""
    SL, kper = pcl_slices(C), pcl_kper(C, K)
    out = []
    for s in range(SL):
        k0 = min(s * kper, K)
        n = min(k0 + kper, K) - k0
        out.append((n // 4 * 4, n % 4))
    return out


def pcl_grid(hw, b):
    return cdiv(hw, PX), b


# name, b, K, C, h, w, temperature, weight, ignore_label, lddf (None: K), loss0, special, paths
PclCase = namedtuple('PclCase', 'name b K C h w temp weight ignore lddf loss0 special paths')


def _p(name, b, K, C, h, w, paths, temp=8.0, weight=1.0, ignore=-1, lddf=None, loss0=0.0, special=None):
    return PclCase(name, b, K, C, h, w, temp, weight, ignore, lddf, loss0, special, tuple(paths))


PCL_CASES = [
    _p('k8_hw1', 1, 8, 6, 1, 1, ['empty_slices', 'one_pixel']),
    _p('k72_c15', 1, 72, 15, 3, 5, ['slices8', 'unroll_tail']),
    _p('k136_hw33', 2, 136, 6, 3, 11, ['chunk2_partial', 'block2_one_lane', 'batch2']),
    _p('k200_ld264', 1, 200, 6, 5, 9, ['lddf_gt_k', 'accumulate'], lddf=264),
    _p('c16_k2048_hw40', 1, 2048, 16, 5, 8, ['lds_attr', 'slices8']),
    _p('image_all_ignored', 2, 64, 6, 4, 9, ['image_ignored', 'batch2'], special='image1_ignored'),
    _p('zero_feature_pixel', 1, 64, 6, 4, 9, ['degenerate_pixel'], special='zero_pixel'),
    _p('sharp', 1, 64, 6, 4, 9, ['saturated_softmax'], temp=0.05),
    _p('weighted', 1, 64, 6, 4, 9, ['weight', 'loss_accumulates'], temp=2.0, weight=0.5, loss0=2.0),
    _p('ignore255', 1, 64, 6, 4, 9, ['label_flag', 'ignore255'], ignore=255, special='bad_labels'),
    _p('none_kept', 1, 64, 6, 4, 9, ['none_kept'], special='none_kept'),
    _p('nan_one', 1, 64, 6, 4, 9, ['nonfinite'], special='nan'),
    _p('inf_one', 1, 64, 6, 4, 9, ['nonfinite'], special='inf'),
    _p('nan_sixteen_blocks', 1, 32, 6, 16, 32, ['nonfinite', 'poison_wrap'], special='nan_blocks'),
    _p('poison_multiple', 1, 32, 6, 32, 32, ['nonfinite', 'poison_wrap'], special='nan_blocks'),
]
PCL_REQUIRED = ['empty_slices', 'one_pixel', 'slices8', 'unroll_tail', 'chunk2_partial', 'block2_one_lane', 'batch2',
                'lddf_gt_k', 'accumulate', 'lds_attr', 'image_ignored', 'degenerate_pixel', 'saturated_softmax', 'weight',
                'loss_accumulates', 'label_flag', 'ignore255', 'none_kept', 'nonfinite', 'poison_wrap']
PCL_FINITE = [c for c in PCL_CASES if 'nonfinite' not in c.paths and 'none_kept' not in c.paths]
NONFINITE_PIXEL = 5                  # the kept pixel that holds the NaN / Inf feature (nan_one, inf_one), channel 3
DEGENERATE_PIXEL = 7                 # the kept pixel of all-zero features (zero_feature_pixel)
SENTINEL_BITS = 0x4e9a               # bf16 bits of the columns [K, lddf): they come back bit-identical

# (name, C, K, lddf or None, short workspace) -> the status comes from pcl_status
PCL_REFUSALS = [('k12', 6, 12, None, False), ('k4104', 6, 4104, None, False), ('ld_k_plus_4', 6, 64, 68, False),
                ('ld_lt_k', 6, 64, 56, False), ('c5', 5, 64, None, False), ('c17', 17, 64, None, False),
                ('c16_k4096_lds', 16, 4096, None, False), ('short_ws', 6, 64, None, True)]


def _seed(name):
    return zlib.crc32(name.encode())


def pcl_inputs(case):
    """-> dict(feat f32 (b,K,h,w), protos f32 (C,K), lab int64 (b,h,w)).  About one pixel in six is ignored."""
    rng = np.random.default_rng(_seed('pcl:' + case.name))
    b, K, C, h, w = case.b, case.K, case.C, case.h, case.w
    feat = rng.standard_normal((b, K, h, w)).astype(np.float32)
    protos = rng.standard_normal((C, K)).astype(np.float32)
    lab = rng.integers(0, C, (b, h, w)).astype(np.int64)
    lab[rng.random((b, h, w)) < 1 / 6] = case.ignore
    flat = lab.reshape(b, -1)
    f = feat.reshape(b, K, -1)
    s = case.special
    if h * w > 1:
        flat[:, 0] = 0                                           # at least one kept pixel per image
    else:
        flat[:] = 2
    if s == 'image1_ignored':
        flat[1] = case.ignore
    elif s == 'zero_pixel':
        flat[0, DEGENERATE_PIXEL] = 1
        f[0, :, DEGENERATE_PIXEL] = 0.0
    elif s == 'bad_labels':
        flat[0, 3], flat[0, 4], flat[0, 6], flat[0, 9] = -1, C, case.ignore, 1
    elif s == 'none_kept':
        flat[:] = case.ignore
    elif s in ('nan', 'inf'):
        flat[0, NONFINITE_PIXEL] = 2
        f[0, 3, NONFINITE_PIXEL] = np.nan if s == 'nan' else np.inf
    elif s == 'nan_blocks':
        for blk in range(cdiv(h * w, PX)):                       # one NaN in a kept pixel of every 32-pixel block
            p = blk * PX + (blk * 7) % PX
            flat[0, p] = 1
            f[0, blk % K, p] = np.nan
    return dict(feat=feat, protos=protos, lab=lab)


def pcl_ref(feat, protos, lab, temp, ignore, weight=1.0):
    """fp64 from the fp32 inputs -> (loss, grad (b, hw, K) pixel-major, kept (b, hw) bool, flag bit 2).  A pixel is kept
    when its label is not ignore_label and lies in [0, C); the loss is the mean over the kept pixels (NaN when none).
    dL/df = sum_c alpha_c pn_c - beta f with alpha_c = g_c / (T nrm), beta = sum_c g_c (f . pn_c) / (T nrm^3), g = dL/dz,
    nrm = max(||f||, 1e-12): the derivative of f / ||f||, and with beta's numerator 0 at f = 0 the derivative of
    f / 1e-12 as well."""
    feat, protos = np.asarray(feat, np.float64), np.asarray(protos, np.float64)
    lab = np.asarray(lab, np.int64)
    b, K = feat.shape[:2]
    C = protos.shape[0]
    f = feat.reshape(b, K, -1).transpose(0, 2, 1)                # (b, hw, K)
    l = lab.reshape(b, -1)
    kept = (l != ignore) & (l >= 0) & (l < C)
    flag = FLAG_LABEL if ((l != ignore) & ((l < 0) | (l >= C))).any() else 0
    n = int(kept.sum())
    pn = protos / np.maximum(np.sqrt((protos * protos).sum(1, keepdims=True)), 1e-12)
    grad = np.zeros_like(f)
    if n == 0:
        return float('nan'), grad, kept, flag
    with np.errstate(all='ignore'):
        fk = f[kept]                                             # (n, K)
        lk = l[kept]
        nrm = np.maximum(np.sqrt((fk * fk).sum(1)), 1e-12)
        d = fk @ pn.T                                            # (n, C)
        z = d / nrm[:, None] / temp
        zmax = z.max(1, keepdims=True)
        lse = zmax[:, 0] + np.log(np.exp(z - zmax).sum(1))
        per = lse - z[np.arange(n), lk]
        loss = weight * per.sum() / n
        g = np.exp(z - lse[:, None])
        g[np.arange(n), lk] -= 1.0
        g *= weight / n
        alpha = g / (temp * nrm[:, None])
        beta = (g * d).sum(1) / (temp * nrm ** 3)
        grad[kept] = alpha @ pn - beta[:, None] * fk
    return float(loss), grad, kept, flag


def accumulate_old(ref_grad, name):
    """The bf16 gradient an accumulating call adds onto, as fp32 values that bf16 holds exactly: random, of the
    reference's magnitude and of either sign, so that sums which cancel most of the gradient are among the elements.  The
    bound 2^-8 |old + ref| is ONE bf16 rounding of the sum: a kernel that rounds its gradient to bf16 first and the sum
    again misses it where the two cancel."""
    rng = np.random.default_rng(_seed('old:' + name))
    scale = np.abs(ref_grad).max() / 2
    return bf16_round((rng.standard_normal(ref_grad.shape) * scale).astype(np.float32))


# ---------------------------------------------------------------- bf16 on the bits
def bf16_bits(x):
    """fp32 -> bf16 bits (uint16), round to nearest even, finite inputs."""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7fff + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def bf16_value(bits):
    return (np.asarray(bits, np.uint16).astype(np.uint32) << 16).view(np.float32)


def bf16_round(x):
    return bf16_value(bf16_bits(x)).reshape(np.shape(x))


# ---------------------------------------------------------------- the ASPP head (aspp_kernels.hip)
ASPP_TAPS = 9
PROD_DILATIONS = (6, 12, 18, 24)


def zcol(head, d, c, tap, C):
    return ((head * 4 + d) * C + c) * 9 + tap


def aspp_columns(C):
    return 72 * C                     # 2 heads x 4 dilations x C classes x 9 taps


def aspp_zc(C):
    return cdiv(aspp_columns(C), 64) * 64


def tap_offset(tap, dil):
    return (tap // 3 - 1) * dil, (tap % 3 - 1) * dil


# width: 'exact' zc = 72 C, no pad columns; 'pad64' zc = the pad up to 64; 'slice' pad64 as a column slice of a wider buffer
AsppCase = namedtuple('AsppCase', 'name N h w C dils width paths')
ASPP_CASES = [
    AsppCase('5x4_centre_only', 1, 5, 4, 6, PROD_DILATIONS, 'pad64', ('centre_only', 'pad64')),
    AsppCase('1x9', 1, 1, 9, 6, PROD_DILATIONS, 'exact', ('one_row', 'exact_width')),
    AsppCase('7x7_dil6_one_pixel', 1, 7, 7, 7, PROD_DILATIONS, 'pad64', ('dil6_one_pixel', 'c7', 'pad64')),
    AsppCase('25x25_corners', 1, 25, 25, 6, PROD_DILATIONS, 'slice', ('dil24_corners', 'slice')),
    AsppCase('13x31_n2', 2, 13, 31, 6, PROD_DILATIONS, 'pad64', ('batch2', 'pad64')),
    AsppCase('c16_exact', 1, 6, 7, 16, (1, 2, 3, 5), 'exact', ('c16', 'exact_width', 'dense_taps')),
    AsppCase('6x7_dense_slice', 2, 6, 7, 7, (1, 2, 3, 5), 'slice', ('dense_taps', 'slice', 'c7', 'batch2')),
]
ASPP_REQUIRED = ['centre_only', 'one_row', 'dil6_one_pixel', 'dil24_corners', 'batch2', 'c7', 'c16', 'dense_taps',
                 'exact_width', 'pad64', 'slice']
ASPP_SLICE_LEFT, ASPP_SLICE_RIGHT = 8, 16         # sentinel columns on either side of a 'slice' case's z / dz
ASPP_SENTINEL_BITS = 0x4e9a


def aspp_width(case):
    """-> (zc, ld, first column of the slice in its buffer)."""
    zc = aspp_columns(case.C) if case.width == 'exact' else aspp_zc(case.C)
    if case.width == 'slice':
        return zc, zc + ASPP_SLICE_LEFT + ASPP_SLICE_RIGHT, ASPP_SLICE_LEFT
    return zc, zc, 0


def tap_hits(case):
    """-> {dilation: [per off-centre tap, the number of pixels whose tap falls inside the map]}."""
    out = {}
    for dl in case.dils:
        out[dl] = [max(case.h - abs(dy), 0) * max(case.w - abs(dx), 0)
                   for dy, dx in (tap_offset(tap, dl) for tap in range(9) if tap != 4)]
    return out


def _ties(rng, shape):
    """fp32 values for the rounding copy: random, with one in four an exact tie (low 16 bits 0x8000, odd and even kept
    halves) and one in eight a value whose kept mantissa is all ones, so that rounding up carries into the exponent."""
    g = rng.standard_normal(shape).astype(np.float32)
    u = g.view(np.uint32).reshape(-1)
    kind = rng.integers(0, 8, u.size)
    u[kind < 2] = (u[kind < 2] & np.uint32(0xffff0000)) | np.uint32(0x8000)
    u[kind == 2] = (u[kind == 2] | np.uint32(0x007f0000)) | np.uint32(0xc000)
    return g


def aspp_inputs(case):
    """-> dict(z bf16 bits (M, zc) uint16, biases 8 x f32 (C,), g1, g2 f32 (N,C,h,w), dbias0 8 x f32 (C,))."""
    rng = np.random.default_rng(_seed('aspp:' + case.name))
    N, h, w, C = case.N, case.h, case.w, case.C
    zc = aspp_width(case)[0]
    z = bf16_bits(rng.standard_normal((N * h * w, zc)).astype(np.float32))
    biases = [(rng.standard_normal(C) + i).astype(np.float32) for i in range(8)]      # all eight distinct
    g1, g2 = _ties(rng, (N, C, h, w)), _ties(rng, (N, C, h, w))
    dbias0 = [rng.standard_normal(C).astype(np.float32) for _ in range(8)]
    return dict(z=z, biases=biases, g1=g1, g2=g2, dbias0=dbias0)


def gather_ref(z_bits, biases, N, h, w, C, dils):
    """-> (out1, out2) f32 (N,C,h,w): the fp32 sum in the kernel's order -- per dilation the bias, then the nine taps
    that fall inside the map (a tap outside adds nothing, not +0)."""
    z = bf16_value(z_bits).reshape(N, h, w, -1)
    outs = []
    ys, xs = np.arange(h)[:, None], np.arange(w)[None, :]
    for head in range(2):
        acc = np.zeros((N, C, h, w), np.float32)
        for d, dl in enumerate(dils):
            acc = (acc + biases[head * 4 + d].astype(np.float32)[None, :, None, None]).astype(np.float32)
            for tap in range(9):
                dy, dx = tap_offset(tap, dl)
                yy, xx = ys + dy, xs + dx
                inside = (yy >= 0) & (yy < h) & (xx >= 0) & (xx < w)                 # (h, w)
                yc, xc = np.clip(yy, 0, h - 1), np.clip(xx, 0, w - 1)
                cols = np.array([zcol(head, d, c, tap, C) for c in range(C)])
                val = z[:, yc, xc][:, :, :, cols].transpose(0, 3, 1, 2)              # (N, C, h, w)
                acc = np.where(inside[None, None], (acc + val).astype(np.float32), acc)
        outs.append(acc)
    return outs


def scatter_ref(g1, g2, N, h, w, C, dils, zc):
    """-> dz bf16 bits (M, zc): column zcol(head, d, c, tap) of pixel (n, y, x) = rne(g_head[n][c][y - dy][x - dx]) or 0
    outside the map; the pad columns [72 C, zc) are 0."""
    dz = np.zeros((N, h, w, zc), np.uint16)
    ys, xs = np.arange(h)[:, None], np.arange(w)[None, :]
    for head, g in enumerate((g1, g2)):
        gb = bf16_bits(g).reshape(N, C, h, w)
        for d, dl in enumerate(dils):
            for tap in range(9):
                dy, dx = tap_offset(tap, dl)
                yy, xx = ys - dy, xs - dx
                inside = (yy >= 0) & (yy < h) & (xx >= 0) & (xx < w)
                yc, xc = np.clip(yy, 0, h - 1), np.clip(xx, 0, w - 1)
                val = np.where(inside[None, None], gb[:, :, yc, xc], np.uint16(0))   # (N, C, h, w)
                for c in range(C):
                    dz[..., zcol(head, d, c, tap, C)] = val[:, c]
    return dz.reshape(N * h * w, zc)


def dbias_ref(g1, g2, dbias0, dtype=np.float64):
    """-> eight (C,) arrays: dbias0[head * 4 + d] + sum over (n, y, x) of g_head, the same total for the four dilations."""
    out = []
    for head, g in enumerate((g1, g2)):
        tot = g.astype(dtype).sum((0, 2, 3), dtype=dtype)
        for d in range(4):
            out.append((dbias0[head * 4 + d].astype(dtype) + tot).astype(dtype))
    return out


# ---------------------------------------------------------------- which case reaches which path
def paths_reached():
    r = {}

    def hit(path, name):
        r.setdefault(path, []).append(name)

    for c in PCL_CASES:
        hw, SL = c.h * c.w, pcl_slices(c.C)
        shapes = pcl_slice_shapes(c.C, c.K)
        x = pcl_inputs(c)
        lab = x['lab'].reshape(c.b, -1)
        kept = (lab != c.ignore) & (lab >= 0) & (lab < c.C)
        if (0, 0) in shapes:
            hit('empty_slices', c.name)
        if hw == 1:
            hit('one_pixel', c.name)
        if SL == 8:
            hit('slices8', c.name)
        if any(t for _, t in shapes) and any(u for u, _ in shapes):
            hit('unroll_tail', c.name)
        if c.K > KC and c.K % KC == 8:
            hit('chunk2_partial', c.name)
        if hw % PX == 1 and hw > PX:
            hit('block2_one_lane', c.name)
        if c.b >= 2:
            hit('batch2', c.name)
        if c.lddf is not None and c.lddf > c.K:
            hit('lddf_gt_k', c.name)
            hit('accumulate', c.name)                            # the test runs this case plain and accumulating
        if pcl_lds(c.C, c.K) > LDS_ATTR and pcl_status(c.C, c.K) == OK:
            hit('lds_attr', c.name)
        if c.b >= 2 and not kept[1].any() and kept[0].any():
            hit('image_ignored', c.name)
        f = x['feat'].reshape(c.b, c.K, -1)
        if kept.any() and np.isfinite(f).all() and ((f == 0).all(1) & kept).any():
            hit('degenerate_pixel', c.name)
        if c.temp < 0.1:
            hit('saturated_softmax', c.name)
        if c.weight != 1.0:
            hit('weight', c.name)
        if c.loss0 != 0.0:
            hit('loss_accumulates', c.name)
        bad = (lab != c.ignore) & ((lab < 0) | (lab >= c.C))
        if (lab == -1).any() and (lab == c.C).any() and bad.any():
            hit('label_flag', c.name)
        if c.ignore == 255 and (lab == 255).any():
            hit('ignore255', c.name)
        if not kept.any():
            hit('none_kept', c.name)
        nf = ~np.isfinite(f).all(1) & kept                       # (b, hw): kept pixels with a non-finite feature
        if nf.any():
            hit('nonfinite', c.name)
            blocks = {(i, p // PX) for i, p in zip(*np.nonzero(nf))}
            if len(blocks) % 16 == 0:
                hit('poison_wrap', c.name)
    for c in ASPP_CASES:
        hits = tap_hits(c)
        if not any(sum(v) for v in hits.values()):
            hit('centre_only', c.name)
        if c.h == 1:
            hit('one_row', c.name)
        if sorted(hits.get(6, [])) == [1] * 4 + [7] * 4 and not any(sum(hits[d]) for d in c.dils if d > 6):
            hit('dil6_one_pixel', c.name)
        if sorted(hits.get(24, [])) == [1] * 4 + [25] * 4:
            hit('dil24_corners', c.name)
        if c.N >= 2:
            hit('batch2', c.name)
        if c.C in (7, 16):
            hit('c%d' % c.C, c.name)
        if all(min(v) > 0 for v in hits.values()):          # every tap of every dilation lands somewhere
            hit('dense_taps', c.name)
        zc, ld, _ = aspp_width(c)
        hit('slice' if ld > zc else ('exact_width' if zc == aspp_columns(c.C) else 'pad64'), c.name)
    return r
