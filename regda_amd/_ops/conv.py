"""The convolution stack: forward routes, fused BatchNorm epilogues and operands, weight gradients, the stem
(csrc/conv_kernels.hip; stem_im2col, a neighbour from csrc/norm_kernels.hip, sits with the stem it serves).
The weight-gradient workspace lives here and nowhere else: recorded plans hold its addresses.  bench.py
replaces conv2d, conv2d_wgrad, conv2d_bneval, conv2d_bnbwd, conv2d_wgrad_grouped, conv2d_bnin and conv2d_grouped
on regda_amd.ops, so the library calls those seven as attributes of regda_amd.ops only."""
import ctypes

import torch

from .._lib import lib
from .base import _ld, _p, _stat, _stream


# --------------------------------------------------------------------------- conv stack
# Activations are torch.bfloat16 2-D tensors [N*H*W, ld] ("PxC"); a view with a column offset is
# expressed by passing a slice of the buffer (data_ptr of the slice) and its row stride.


def conv2d(x, w, y, N, H, W, Ho, Wo, kh, kw, stride, pad, dil, mode=0, res=None, stats=None, stat_groups=1,
           res_mask=None):
    """x [N*H*W, Cin(view)], w bf16 [Cout, kh*kw, Cin] contiguous, y [N*Ho*Wo, Cout(view)].
    stats: rgda_stat_t (int64) [stat_groups][8][2][Cout] accumulators (zeroed by the caller; ops.new_stats)."""
    Cout, taps, Cin = w.shape
    assert taps == kh * kw and x.shape[1] == Cin and y.shape[1] == Cout
    lib().call('rgda_conv2d', x.data_ptr(), _ld(x), w.data_ptr(), y.data_ptr(), _ld(y), _p(res),
               _ld(res) if res is not None else 0, _p(res_mask), _stat(stats), stat_groups, N, H, W, Cin, Ho, Wo, Cout, kh, kw, stride,
               pad, dil, mode, _stream())


class _ConvDesc(ctypes.Structure):
    _fields_ = [(k, ctypes.c_void_p) for k in ('x', 'wgt', 'y', 'res', 'res_relu_mask', 'stats')] + \
               [(k, ctypes.c_int) for k in ('ldx', 'ldy', 'ldres', 'stat_groups', 'N', 'H', 'W', 'Cin', 'Ho', 'Wo', 'Cout', 'kh',
                                            'kw', 'stride', 'pad', 'dil', 'mode')]


def _conv_descs(items):
    arr = (_ConvDesc * len(items))()
    for d, it in zip(arr, items):
        x, w, y, N, H, W, Ho, Wo, kh, kw, stride, pad, dil = it[:13]
        mode = it[13] if len(it) > 13 else 0
        res = it[14] if len(it) > 14 else None
        stats = it[15] if len(it) > 15 else None
        stat_groups = it[16] if len(it) > 16 else 1
        res_mask = it[17] if len(it) > 17 else None
        Cout, taps, Cin = w.shape
        assert taps == kh * kw and x.shape[1] == Cin and y.shape[1] == Cout
        d.x, d.wgt, d.y, d.res, d.res_relu_mask, d.stats = x.data_ptr(), w.data_ptr(), y.data_ptr(), _p(res), _p(res_mask), _stat(stats)
        d.ldx, d.ldy, d.ldres, d.stat_groups = _ld(x), _ld(y), (_ld(res) if res is not None else 0), stat_groups
        d.N, d.H, d.W, d.Cin, d.Ho, d.Wo, d.Cout = N, H, W, Cin, Ho, Wo, Cout
        d.kh, d.kw, d.stride, d.pad, d.dil, d.mode = kh, kw, stride, pad, dil, mode
    return arr


def conv2d_grouped(items):
    """items: list of tuples holding conv2d's arguments (x, w, y, N, H, W, Ho, Wo, kh, kw, stride, pad, dil[, mode[, res[, stats
    [, stat_groups[, res_mask]]]]]) -- INDEPENDENT convolutions; the small-tile ones share launches (rgda_conv2d_grouped)."""
    if not items:
        return
    arr = _conv_descs(items)
    lib().call('rgda_conv2d_grouped', ctypes.cast(arr, ctypes.c_void_p), len(items), _stream())


def conv2d_grouped_launches(items):
    """Kernel launches conv2d_grouped(items) makes; raises where it would fail."""
    arr = _conv_descs(items)
    n = lib().size('rgda_conv2d_grouped_launches', ctypes.cast(arr, ctypes.c_void_p), len(items))
    if n < 0:
        raise ValueError('rgda_conv2d_grouped: status %d' % n)
    return n


def conv2d_bneval(x, w, y, N, H, W, Ho, Wo, kh, kw, stride, pad, dil, rm, rv, gamma, beta, relu, res=None, eps=1e-5):
    """conv + inference-mode BN (+ residual + ReLU) in one kernel (the EMA teacher's units)."""
    Cout, taps, Cin = w.shape
    assert taps == kh * kw and x.shape[1] == Cin and y.shape[1] == Cout
    lib().call('rgda_conv2d_bneval', x.data_ptr(), _ld(x), w.data_ptr(), y.data_ptr(), _ld(y), _p(res),
               _ld(res) if res is not None else 0, rm.data_ptr(), rv.data_ptr(), gamma.data_ptr(), beta.data_ptr(), eps,
               int(relu), N, H, W, Cin, Ho, Wo, Cout, kh, kw, stride, pad, dil, _stream())


def conv2d_bnbwd(x, w, y, N, H, W, Ho, Wo, kh, kw, stride, pad, dil, mode, res, sums, groups, bn_y, bn_x, bn_mi, relu,
                 nscale=None, rows_per_image=0, relu_mask=None, res_mask=None, bn_gamma=None, bn_beta=None):
    """conv2d whose epilogue also accumulates the BN-backward sums of the consumer of `y` (see rgda_conv2d_bnbwd).
    relu: False / True, or 2 = the ReLU sign recomputed from bn_x (needs bn_gamma, bn_beta)."""
    Cout, taps, Cin = w.shape
    assert taps == kh * kw and x.shape[1] == Cin and y.shape[1] == Cout
    lib().call('rgda_conv2d_bnbwd', x.data_ptr(), _ld(x), w.data_ptr(), y.data_ptr(), _ld(y), _p(res),
               _ld(res) if res is not None else 0, _p(res_mask), _stat(sums), groups, _p(bn_y), _ld(bn_y) if bn_y is not None else 0,
               _p(relu_mask), bn_x.data_ptr(), _ld(bn_x), bn_mi.data_ptr(), _p(nscale), rows_per_image, int(relu),
               _p(bn_gamma), _p(bn_beta), N, H, W, Cin, Ho, Wo, Cout, kh, kw, stride, pad, dil, mode, _stream())


class _BnOperand(ctypes.Structure):
    _fields_ = [('stats', ctypes.c_void_p), ('gamma', ctypes.c_void_p), ('beta', ctypes.c_void_p), ('mi', ctypes.c_void_p),
                ('running_mean', ctypes.c_void_p), ('running_var', ctypes.c_void_p), ('num_batches_tracked', ctypes.c_void_p),
                ('eps', ctypes.c_float), ('momentum', ctypes.c_float), ('groups', ctypes.c_int), ('relu', ctypes.c_int)]


def bn_operand(stats, gamma, beta, mi=None, rm=None, rv=None, nbt=None, groups=1, relu=True, eps=1e-5, momentum=0.1):
    """rgda_bn_operand: a BatchNorm (+ ReLU) that runs on its consumer's operand path.  stats: the producing convolution's
    accumulators [groups][8][2][C] (int64); mi (out) f32 [groups][2][C].  Returns a pointer object for conv2d_bnin /
    maxpool_fwd_bnin (host memory holding device pointers; the caller keeps the tensors alive)."""
    d = _BnOperand(_stat(stats), gamma.data_ptr(), beta.data_ptr(), _p(mi), _p(rm), _p(rv), _p(nbt), eps, momentum,
                   int(groups), int(bool(relu)))
    return ctypes.cast(ctypes.pointer(d), ctypes.c_void_p)


def conv2d_bnin_supported(M, Cout, Cin, kh, kw, stride, pad, dil, H, W, Ho, Wo, groups):
    """0 = not served, 1 = served, 2 = served and faster than the apply pass it replaces."""
    return lib().size('rgda_conv2d_bnin_supported', M, Cout, Cin, kh, kw, stride, pad, dil, H, W, Ho, Wo, groups)


def conv2d_bnin(bnop, x, w, y, N, H, W, Ho, Wo, kh, kw, stride, pad, dil, res=None, stats=None, stat_groups=1):
    """conv2d (forward) over  relu(BatchNorm(x))  of the producing convolution's RAW output x, applied on the operand path
    (rgda_conv2d_bnin; bnop from bn_operand()).  Raises ValueError where no kernel carries the transform."""
    Cout, taps, Cin = w.shape
    assert taps == kh * kw and x.shape[1] == Cin and y.shape[1] == Cout
    lib().call('rgda_conv2d_bnin', bnop, x.data_ptr(), _ld(x), w.data_ptr(), y.data_ptr(), _ld(y), _p(res),
               _ld(res) if res is not None else 0, _stat(stats), stat_groups, N, H, W, Cin, Ho, Wo, Cout, kh, kw, stride, pad,
               dil, _stream())


def conv2d_wgrad(x, dy, dw, N, H, W, Ho, Wo, kh, kw, stride, pad, dil):
    """dw f32 [Cout, kh*kw, Cin] contiguous, accumulated."""
    Cout, taps, Cin = dw.shape
    assert dw.is_contiguous() and dw.dtype == torch.float32
    conv2d_wgrad_grouped([(x, dy, dw, N, H, W, Ho, Wo, kh, kw, stride, pad, dil)])


class _WgradDesc(ctypes.Structure):
    _fields_ = [('x', ctypes.c_void_p), ('dy', ctypes.c_void_p), ('dw', ctypes.c_void_p), ('ldx', ctypes.c_int),
                ('lddy', ctypes.c_int)] + [(k, ctypes.c_int) for k in
                                           ('N', 'H', 'W', 'Cin', 'Ho', 'Wo', 'Cout', 'kh', 'kw', 'stride', 'pad', 'dil',
                                            'lddw', 'co_split')]


_WGRAD_WS = {}          # (device index, raw stream) -> workspace of the weight-gradient launches issued on that stream
_WGRAD_WS_OLD = []      # outgrown workspaces stay allocated: a recorded plan (regda_amd/plan.py) may hold their address


def _wgrad_ws(nbytes, device):
    """The split-K workspace of the current stream (rgda_conv2d_wgrad: counters zeroed once, calls ordered on one
    stream share it).  Grown on demand; never freed."""
    key = (device.index, _stream())
    ws = _WGRAD_WS.get(key)
    if ws is None or ws.numel() < nbytes:
        if ws is not None:
            _WGRAD_WS_OLD.append(ws)
        ws = torch.empty(max(nbytes, 32 << 20), dtype=torch.uint8, device=device)
        ws[:65536].zero_()
        _WGRAD_WS[key] = ws
    return ws


def conv2d_wgrad_grouped(items):
    """items: list of (x, dy, dw, N, H, W, Ho, Wo, kh, kw, stride, pad, dil) -- the arguments of conv2d_wgrad.
    Layers that map to the same kernel share a launch (rgda_conv2d_wgrad_grouped)."""
    if not items:
        return
    arr = (_WgradDesc * len(items))()
    for d, (x, dy, dw, N, H, W, Ho, Wo, kh, kw, stride, pad, dil) in zip(arr, items):
        # dw: [Cout, taps, Cin], dense or a channel slice of a wider [Cout, taps, C] tensor (lddw = its row stride); for a
        # 1x1 layer also [S, T, Cin] with T > 1: the layer's S * T output rows are T stacked filters of S channels
        # ([t][s] order) and land channel-major in that tensor (co_split = S)
        S, T, Cin = dw.shape
        assert dw.dtype == torch.float32 and dw.stride(2) == 1 and dw.stride(0) == T * dw.stride(1)
        stacked = kh * kw == 1 and T > 1
        assert stacked or T == kh * kw
        Cout = S * T if stacked else S
        d.x, d.dy, d.dw, d.ldx, d.lddy = x.data_ptr(), dy.data_ptr(), dw.data_ptr(), _ld(x), _ld(dy)
        d.N, d.H, d.W, d.Cin, d.Ho, d.Wo, d.Cout = N, H, W, Cin, Ho, Wo, Cout
        d.kh, d.kw, d.stride, d.pad, d.dil = kh, kw, stride, pad, dil
        d.lddw, d.co_split = dw.stride(1), (S if stacked else 0)
    L = lib()
    ap = ctypes.cast(arr, ctypes.c_void_p)
    ws = _wgrad_ws(L.size('rgda_conv2d_wgrad_workspace', ap, len(items)), items[0][0].device)
    L.call('rgda_conv2d_wgrad_grouped', ap, len(items), ws.data_ptr(), ws.numel(), _stream())


def stem_conv(img, wb, y, stats, N, H, W, Ho, Wo, stat_groups=1):
    """The 7x7 / stride-2 stem straight from the NCHW fp32 image (rgda_stem_conv; Wo % 64 == 0): y [N*Ho*Wo, 64(view)]
    bf16, wb the padded bf16 stem weights [64, 1, 192], stats as for conv2d."""
    lib().call('rgda_stem_conv', img.data_ptr(), wb.data_ptr(), y.data_ptr(), _ld(y), _stat(stats), stat_groups, N, H, W, Ho, Wo,
               _stream())


def stem_conv_bneval(img, wb, y, rm, rv, gamma, beta, relu, N, H, W, Ho, Wo, eps=1e-5):
    lib().call('rgda_stem_conv_bneval', img.data_ptr(), wb.data_ptr(), y.data_ptr(), _ld(y), rm.data_ptr(), rv.data_ptr(),
               gamma.data_ptr(), beta.data_ptr(), eps, int(relu), N, H, W, Ho, Wo, _stream())


def stem_im2col(img, col, N, H, W, Ho, Wo):
    lib().call('rgda_stem_im2col', img.data_ptr(), col.data_ptr(), N, H, W, Ho, Wo, col.shape[1], _stream())


_STEM_WS = {}           # (device index, raw stream) -> workspace of rgda_stem_wgrad on that stream (grown on demand, never freed)
_STEM_WS_OLD = []


def stem_wgrad(img, dy, dw, N, H, W, Ho, Wo):
    """The stem's weight gradient straight from the NCHW fp32 image (rgda_stem_wgrad; Wo % 64 == 0): dw f32 [64, 147]
    (contiguous, accumulated), dy bf16 [N*Ho*Wo, 64(view)]."""
    assert dw.is_contiguous() and dw.dtype == torch.float32 and dw.numel() == 64 * 147 and img.is_contiguous()
    L = lib()
    nbytes = L.size('rgda_stem_wgrad_workspace', N, H, W)
    if nbytes == 0:
        raise ValueError('rgda_stem_wgrad: geometry not served (Wo % 64 != 0): use stem_im2col + conv2d_wgrad')
    key = (img.device.index, _stream())
    ws = _STEM_WS.get(key)
    if ws is None or ws.numel() < nbytes:
        if ws is not None:
            _STEM_WS_OLD.append(ws)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=img.device)
        _STEM_WS[key] = ws
    L.call('rgda_stem_wgrad', img.data_ptr(), dy.data_ptr(), _ld(dy), dw.data_ptr(), ws.data_ptr(), ws.numel(), N, H, W, Ho, Wo,
           _stream())
