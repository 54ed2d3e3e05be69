"""Every convolution route: the kernel instantiations rgda_conv2d / _bneval / _bnbwd / _bnin and rgda_conv2d_wgrad dispatch
to, each with the smallest problem that reaches it and the calls the tests make on it.

ROUTES is a list of Route(name, problem, calls, groups).  `name` is the string the dispatch queries return
(rgda_conv2d_kernel / rgda_conv2d_wgrad_kernel).  `calls` are run on `problem`, each with every statistics group count
in `groups` where the call has statistics; every one of them dispatches to `name` (tests/test_conv_routes_cpu.py checks
it).  A route may appear several times (another geometry, the data-gradient mode).  The calls:
  plain, stats, res, res_stats, res_mask    rgda_conv2d (res_mask: the residual gated by a ReLU sign mask)
  ev, ev_relu                               rgda_conv2d_bneval (ev_relu: with a residual and the ReLU)
  bnbwd1, bnbwd2                            rgda_conv2d_bnbwd with relu 1 (sign from bn_y) and 2 (recomputed from bn_x)
  bnin                                      rgda_conv2d_bnin (BatchNorm + ReLU on the operand path)
  wgrad, wgrad_nows                         rgda_conv2d_wgrad with and without the split-K workspace
"""
from collections import namedtuple

import torch

Problem = namedtuple('Problem', 'N H W Cin Cout k stride pad dil mode Ho Wo')
Route = namedtuple('Route', 'name problem calls groups')


def P(N, H, W, Cin, Cout, k, stride=1, pad=None, dil=1, mode=0, Ho=None, Wo=None):
    """mode 0: (H, W) -> (Ho, Wo) by the convolution's formula.  mode 1 (the data gradient of a forward convolution from
    (Ho, Wo) to (H, W)): give Ho, Wo -- with stride 2 several forward input sizes share one output size."""
    if pad is None:
        pad = dil * (k // 2)
    if Ho is None:
        assert mode == 0
        Ho = (H + 2 * pad - dil * (k - 1) - 1) // stride + 1
        Wo = (W + 2 * pad - dil * (k - 1) - 1) // stride + 1
    return Problem(N, H, W, Cin, Cout, k, stride, pad, dil, mode, Ho, Wo)


FWD = ('plain', 'stats', 'res', 'res_stats', 'res_mask')
EPI = FWD + ('ev', 'ev_relu', 'bnbwd1', 'bnbwd2')
DGRAD = ('plain', 'res', 'res_mask', 'bnbwd1', 'bnbwd2')
WGRAD = ('wgrad', 'wgrad_nows')
STAT_CALLS = ('stats', 'res_stats', 'bnbwd1', 'bnbwd2', 'bnin')

# conv3x3_c64_kernel and conv1x1_stream_kernel have one instantiation per fused epilogue (the template's last argument,
# conv_kernels.hip's EPI_* order).  The dispatch query passes no residual and relu 1 to the fused BatchNorm backward, so
# it only ever names kinds 0, 1, 4 and 5: kinds 2 (res), 3 (res + statistics) and 6 (relu 2) are listed here by
# construction, and route_of() derives their names the same way.
EPI_KIND = {'plain': 0, 'stats': 1, 'res': 2, 'res_mask': 2, 'res_stats': 3, 'ev': 4, 'ev_relu': 4, 'bnbwd1': 5, 'bnbwd2': 6}
PER_KIND = ('conv3x3_c64_kernel<', 'conv1x1_stream_kernel<')


def _per_kind(prefix, problem, groups, dgrad=None):
    """The seven instantiations of a per-epilogue kernel on one problem (`dgrad`: the same geometry in mode 1 for the
    fused BatchNorm backward, the data gradient it serves in the step)."""
    out = []
    for kind in range(7):
        calls = tuple(c for c, k in EPI_KIND.items() if k == kind)
        p = dgrad if (dgrad is not None and kind >= 5) else problem
        out.append(Route('%s%d>' % (prefix, kind), p, calls, groups))
    return out


ROUTES = [
    # ---- conv_igemm_kernel: the generic implicit GEMM (epilogue chosen at run time: one instantiation serves every call)
    # Cout <= 64: 64 x 64 tiles; odd batch, odd map, stride 2, ragged Cout; and the stride-2 data gradient of 17 x 13 maps
    Route('conv_igemm_kernel<64, 64, 2, 2, 2, false, false>', P(3, 17, 13, 64, 40, 3, 2), EPI, (1,)),
    Route('conv_igemm_kernel<64, 64, 2, 2, 2, false, false>', P(3, 9, 7, 128, 64, 3, 2, mode=1, Ho=17, Wo=13), DGRAD, (1,)),
    Route('conv_igemm_kernel<64, 64, 2, 2, 2, false, false>', P(4, 16, 16, 64, 40, 3), EPI, (1, 2, 4)),   # one image per group
    # small maps: the 128 x 64 pipelined tile (what the PPM branches get); ragged Cout, dilation 2, 1x1 stride 2
    Route('conv_igemm_kernel<128, 64, 3, 2, 2, true, false>', P(3, 17, 13, 64, 136, 3, 2), EPI, (1,)),
    Route('conv_igemm_kernel<128, 64, 3, 2, 2, true, false>', P(2, 16, 16, 256, 136, 3, dil=2), EPI, (1, 2)),
    Route('conv_igemm_kernel<128, 64, 3, 2, 2, true, false>', P(3, 9, 7, 128, 136, 3, 2, mode=1, Ho=17, Wo=13), DGRAD, (1,)),
    Route('conv_igemm_kernel<128, 64, 3, 2, 2, true, false>', P(2, 16, 16, 64, 72, 1, 2, 0), EPI, (1, 2)),
    # 8-wave 128 x 128 tiles: 3-stage pipelined (256 - 511 tiles) and 2-stage (>= 512 tiles)
    Route('conv_igemm_kernel<128, 128, 3, 2, 4, true, false>', P(1, 128, 128, 64, 136, 1, pad=0), EPI, (1,)),
    Route('conv_igemm_kernel<128, 128, 3, 2, 4, true, false>', P(2, 64, 128, 64, 136, 1, pad=0), EPI, (1, 2)),
    Route('conv_igemm_kernel<128, 128, 2, 2, 4, false, false>', P(2, 128, 128, 64, 136, 1, pad=0), EPI, (1, 2)),
    # long K, >= 240 tiles of 128 x 256: a 48-wide map (not a multiple of 32: no halo kernel)
    Route('conv_igemm_kernel<128, 256, 3, 2, 4, true, false>', P(2, 40, 48, 512, 2048, 3), EPI, (1,)),
    Route('conv_igemm_kernel<128, 256, 3, 2, 4, true, false>', P(4, 32, 48, 512, 2048, 3), EPI, (1, 2, 4)),  # 6 tiles an image
    # BatchNorm + ReLU on the operand path of the 2-stage 128 x 128 tile: 1x1, and 3x3 stride 2 (padding on the operand path)
    Route('conv_igemm_kernel<128, 128, 2, 2, 4, false, true>', P(2, 128, 128, 64, 136, 1, pad=0), ('bnin',), (1, 2)),
    Route('conv_igemm_kernel<128, 128, 2, 2, 4, false, true>', P(8, 128, 128, 128, 256, 3, 2), ('bnin',), (1, 2, 8)),
    # ---- conv3x3_halo_kernel: long-K 3x3 on 32-wide maps, tiles of 4 / 8 image rows; odd batch, ragged Cout
    Route('conv3x3_halo_kernel<1, 4, false, 4, true>', P(7, 32, 32, 256, 136, 3), EPI, (1, 7)),
    Route('conv3x3_halo_kernel<1, 4, false, 4, true>', P(7, 32, 32, 256, 256, 3, mode=1, Ho=32, Wo=32), DGRAD, (1, 7)),
    Route('conv3x3_halo_kernel<1, 8, false, 4, true>', P(16, 32, 32, 512, 136, 3), EPI, (1, 2, 16)),
    Route('conv3x3_halo_kernel<2, 8, false, 3, true>', P(16, 32, 32, 512, 136, 3, dil=2), EPI, (1, 2, 16)),
    Route('conv3x3_halo_kernel<1, 4, true, 4, true>', P(7, 32, 32, 256, 136, 3), ('bnin',), (1, 7)),
    Route('conv3x3_halo_kernel<1, 8, true, 3, false>', P(16, 32, 32, 512, 136, 3), ('bnin',), (1, 2, 16)),
    # ---- conv3x3_halo_wide_kernel: the same on maps wider than 32 (1024 x 1024 tiles: 64 / 96 columns), 32-column bands
    Route('conv3x3_halo_wide_kernel<1, 4, 4, true, false>', P(7, 32, 64, 256, 72, 3), EPI, (1, 7)),
    Route('conv3x3_halo_wide_kernel<1, 8, 4, true, false>', P(7, 40, 96, 512, 72, 3), EPI, (1, 7)),
    Route('conv3x3_halo_wide_kernel<1, 8, 4, true, false>', P(4, 32, 64, 512, 512, 3), EPI, (1, 2, 4)),
    Route('conv3x3_halo_wide_kernel<2, 8, 3, true, false>', P(7, 40, 96, 512, 72, 3, dil=2), EPI, (1, 7)),
    Route('conv3x3_halo_wide_kernel<1, 4, 4, true, true>', P(7, 32, 64, 256, 72, 3), ('bnin',), (1, 7)),
    Route('conv3x3_halo_wide_kernel<1, 4, 4, true, true>', P(4, 32, 64, 256, 256, 3), ('bnin',), (1, 2, 4)),
    Route('conv3x3_halo_wide_kernel<1, 8, 3, false, true>', P(7, 40, 96, 512, 72, 3), ('bnin',), (1, 7)),
]
# ---- conv3x3_c64_kernel: layer 1's 64 -> 64 3x3 on 128-wide maps (weights resident, rolling window); its data gradient
ROUTES += _per_kind('conv3x3_c64_kernel<128, ', P(4, 128, 128, 64, 64, 3), (1, 2, 4),
                    dgrad=P(4, 128, 128, 64, 64, 3, mode=1, Ho=128, Wo=128))
# ---- conv1x1_stream_kernel: short-K 1x1 on large maps, 64 / 128 input channels (KC = 1 / 2); 15 tiles per workgroup,
# one image of 32 x 60 each
ROUTES += _per_kind('conv1x1_stream_kernel<1, 128, 2, 4, ', P(4, 32, 60, 64, 128, 1, pad=0), (1, 2, 4),
                    dgrad=P(4, 32, 60, 64, 128, 1, pad=0, mode=1, Ho=32, Wo=60))
ROUTES += _per_kind('conv1x1_stream_kernel<2, 128, 2, 4, ', P(4, 32, 60, 128, 256, 1, pad=0), (1, 2, 4),
                    dgrad=P(4, 32, 60, 128, 256, 1, pad=0, mode=1, Ho=32, Wo=60))
# ---- the weight gradient: generic tiles (one job per tap) and the tap-fused 3x3 kernels (64-pixel K tiles of R rows x WT).
# Every problem has enough K tiles (>= 32) for the split-K path: with the workspace ('wgrad') the pixels are split over
# several workgroups and combined through it, without it ('wgrad_nows') one workgroup walks them all
# (tests/test_conv_routes_cpu.py checks that the two calls really differ); odd K-tile counts leave a short last split.
ROUTES += [
    Route('conv_wgrad_kernel<64, 64, 2, 2, 3>', P(33, 17, 13, 64, 40, 3, 2), WGRAD, ()),
    Route('conv_wgrad_kernel<64, 128, 2, 4, 3>', P(9, 16, 16, 136, 64, 1, pad=0), WGRAD, ()),
    Route('conv_wgrad_kernel<128, 64, 4, 2, 3>', P(33, 17, 13, 64, 136, 3, 2), WGRAD, ()),
    Route('conv_wgrad_kernel<128, 128, 2, 4, 3>', P(9, 16, 16, 136, 136, 1, pad=0), WGRAD, ()),
    Route('conv_wgrad_kernel<128, 128, 2, 4, 3>', P(33, 16, 16, 128, 128, 3, 2), WGRAD, ()),
    Route('conv_wgrad_kernel<256, 128, 4, 2, 3>', P(9, 16, 16, 136, 256, 1, pad=0), WGRAD, ()),
    Route('conv_wgrad3x3_wide_kernel<64, 1, 3>', P(5, 8, 64, 128, 136, 3), WGRAD, ()),
    Route('conv_wgrad3x3_wide_kernel<64, 2, 3>', P(3, 16, 64, 128, 256, 3, dil=2), WGRAD, ()),
    Route('conv_wgrad3x3_kernel<32, 1, 2>', P(3, 32, 32, 256, 128, 3), WGRAD, ()),
    Route('conv_wgrad3x3_wide_kernel<32, 2, 3>', P(5, 16, 32, 128, 72, 3, dil=2), WGRAD, ()),
    Route('conv_wgrad3x3_kernel<16, 1, 3>', P(17, 8, 16, 64, 136, 3), WGRAD, ()),
    Route('conv_wgrad3x3_kernel<16, 2, 2>', P(17, 8, 16, 256, 136, 3, dil=2), WGRAD, ()),
]

# Calls with statistics groups that are not whole images: refused (RGDA_ERR_ARG; the dispatch query returns NULL).
# The first two went to conv3x3_halo_wide_kernel, whose tiles then straddled two groups; the others applied one
# group's BatchNorm table to halo rows of the neighbouring group.
SUB_IMAGE = [
    ('stats', P(4, 32, 64, 512, 512, 3), 32),
    ('bnin', P(4, 32, 64, 256, 256, 3), 64),
    ('bnin', P(16, 32, 32, 256, 256, 3), 64),
    ('stats', P(7, 32, 32, 256, 136, 3), 14),
    ('bnbwd1', P(4, 128, 128, 64, 64, 3, mode=1, Ho=128, Wo=128), 8),
    ('stats', P(6, 32, 40, 64, 128, 1, pad=0), 12),
    ('stats', P(3, 17, 13, 64, 40, 3, 2), 9),
    ('bnin', P(8, 128, 128, 128, 256, 3, 2), 16),
]

VARIANT = {'plain': 0, 'stats': 0, 'res': 0, 'res_stats': 0, 'res_mask': 0, 'ev': 1, 'ev_relu': 1, 'bnbwd1': 2, 'bnbwd2': 2,
           'bnin': 3}


def query(lib, variant, p, has_stats, groups):
    """rgda_conv2d_kernel for problem p (None where the call is refused)."""
    r = lib.raw('rgda_conv2d_kernel')(variant, p.N, p.H, p.W, p.Cin, p.Ho, p.Wo, p.Cout, p.k, p.k, p.stride, p.pad, p.dil,
                                      p.mode, int(has_stats), groups)
    return r.decode() if r else None


def _wgrad_desc(p):
    from regda_amd import ops
    d = ops._WgradDesc()
    d.x = d.dy = d.dw = 256                 # never dereferenced: the queries only classify and size
    d.ldx, d.lddy = (p.Cin + 7) // 8 * 8, (p.Cout + 7) // 8 * 8
    d.N, d.H, d.W, d.Cin, d.Ho, d.Wo, d.Cout = p.N, p.H, p.W, p.Cin, p.Ho, p.Wo, p.Cout
    d.kh, d.kw, d.stride, d.pad, d.dil, d.lddw, d.co_split = p.k, p.k, p.stride, p.pad, p.dil, 0, 0
    return d


def wgrad_query(lib, p):
    import ctypes
    r = lib.raw('rgda_conv2d_wgrad_kernel')(ctypes.byref(_wgrad_desc(p)))
    return r.decode() if r else None


def wgrad_workspace(lib, p):
    """rgda_conv2d_wgrad_workspace for problem p: bytes of tile counters plus the split-K partial tiles."""
    import ctypes
    return int(lib.raw('rgda_conv2d_wgrad_workspace')(ctypes.byref(_wgrad_desc(p)), 1))


WGRAD_WS_COUNTERS = 64 << 10    # RGDA_WGRAD_WS_COUNTERS (conv_kernels.hip): a workspace of only the counters = no layer is split


def route_of(lib, call, p, groups=1):
    """The instantiation a call dispatches to: the query, with the per-epilogue kernels' kind derived from the call."""
    if call in WGRAD:
        return wgrad_query(lib, p)
    name = query(lib, VARIANT[call], p, call in STAT_CALLS, groups)
    if name and name.startswith(PER_KIND):
        name = name[:name.rindex(',') + 2] + '%d>' % EPI_KIND[call]
    return name


def expand(route):
    """(call, groups) pairs of a route entry: statistics calls at every group count, the others once."""
    out = []
    for c in route.calls:
        for g in (route.groups if c in STAT_CALLS else (1,)):
            out.append((c, g))
    return out


# ---------------------------------------------------------------- the checks (torch tensors, float64, any device)
U = 2.0 ** -8           # bf16 unit roundoff: one rounding moves a value by at most U times its magnitude
U32 = 2.0 ** -24        # fp32 unit roundoff
# Most rows one workgroup folds into an fp32 partial before the fixed-point add, FOR THE PROBLEMS IN ROUTES: tiles of the
# igemm, halo and c64 kernels hold <= 256 rows, a conv1x1_stream_kernel workgroup folds its T pixel tiles of 128 rows
# (T = 15 on the stream problems above).  Not a property of the kernels: the stream kernel allows T up to 4096, so the
# bound has to be re-derived before it is used at other shapes.
PARTIAL_ROWS = 2048


def elem_violations(y, ref, mag=None, extra=None):
    """Per element |y - ref| <= 2^-8 mag + 2^-12 rms_c(ref) (+ extra): y, ref [rows][C]; mag defaults to |ref|, the
    magnitude the final bf16 rounding acts on; rms_c is the channel's RMS over all rows (absorbs the fp32 accumulation).
    -> number of violating elements."""
    y, ref = y.double(), ref.double()
    rms = ref.pow(2).mean(0, keepdim=True).sqrt()
    bound = U * (ref.abs() if mag is None else mag) + 2.0 ** -12 * rms
    if extra is not None:
        bound = bound + extra
    return int(((y - ref).abs() > bound).sum())


def group_sums(rows, groups, weight=None):
    """fp64 per-group, per-channel (sum, sum of squares) of [rows][C] -- or (sum v, sum v * weight)."""
    v = rows.double().reshape(groups, -1, rows.shape[-1])
    w = v if weight is None else weight.double().reshape(groups, -1, rows.shape[-1])
    return torch.stack([v.sum(1), (v * w).sum(1)], 1), torch.stack([v.abs().sum(1), (v * w).abs().sum(1)], 1)


def stat_violations(got, ref, absref, rows_per_group, frac, partial_rows=PARTIAL_ROWS):
    """Fused statistics [groups][2][C] against fp64 sums of the stored values: fp32 partials of at most `partial_rows` rows
    (a sum of n terms errs by at most (n - 1) 2^-24 times the sum of their magnitudes), then each partial rounded to the
    2^-frac fixed-point step.  -> number of violating (group, sum, channel) entries."""
    n = min(rows_per_group, partial_rows) + 8
    bound = U32 * n * absref + rows_per_group * 2.0 ** -frac
    return int(((got.double() - ref).abs() > bound).sum())


def relerr(a, b):
    """The suite's older whole-tensor measure: max |a - b| / max |b|."""
    return float((a - b).abs().max() / (b.abs().max() + 1e-30))
