"""BatchNorm, pooling, InstanceNorm, the spatial mixes and the classifier (csrc/norm_kernels.hip), with their small
neighbours: group_mix and sparse_mix (csrc/mix_kernels.hip), the ASPP head of Classifier_Module
(csrc/aspp_kernels.hip) and the TransNorm layers (csrc/transnorm_kernels.hip; regda/trans_norm.py)."""
import ctypes

import torch

from .._lib import lib
from .base import _ld, _need_cuda, _p, _stat, _stream, _ws
from .feature import _feat_rows


def bn_stats(x, stats, M, C):
    lib().call('rgda_bn_stats', x.data_ptr(), _ld(x), _stat(stats), M, C, _stream())


def bn_finalize(stats, mi, rm, rv, nbt, M, C, eps=1e-5, momentum=0.1, groups=1):
    lib().call('rgda_bn_finalize', _stat(stats), mi.data_ptr(), _p(rm), _p(rv), _p(nbt), M, C, groups, eps, momentum,
               _stream())


def bn_apply(x, mi, gamma, beta, y, M, C, relu, res=None, nscale=None, rows_per_image=0, groups=1):
    lib().call('rgda_bn_apply', x.data_ptr(), _ld(x), mi.data_ptr(), gamma.data_ptr(), beta.data_ptr(), _p(res),
               _ld(res) if res is not None else 0, _p(nscale), rows_per_image, y.data_ptr(), _ld(y), M, C,
               int(relu), groups, _stream())


def bn_train_apply(x, stats, mi, rm, rv, nbt, gamma, beta, y, M, C, relu, res=None, nscale=None, rows_per_image=0,
                   groups=1, eps=1e-5, momentum=0.1, relu_mask=None):
    lib().call('rgda_bn_train_apply', x.data_ptr(), _ld(x), _stat(stats), mi.data_ptr(), _p(rm), _p(rv), _p(nbt),
               gamma.data_ptr(), beta.data_ptr(), _p(res), _ld(res) if res is not None else 0, _p(nscale),
               rows_per_image, y.data_ptr(), _ld(y), _p(relu_mask), M, C, int(relu), groups, eps, momentum, _stream())


def bn_bwd_reduce(g, y, x, mi, sums, M, C, relu, nscale=None, rows_per_image=0, groups=1, relu_mask=None, gamma=None,
                  beta=None):
    """relu: False / True ([y > 0] from relu_mask or y), or 2 = the sign recomputed from x (needs gamma, beta)."""
    lib().call('rgda_bn_bwd_reduce', g.data_ptr(), _ld(g), _p(y), _ld(y) if y is not None else 0, _p(relu_mask),
               x.data_ptr(), _ld(x),
               mi.data_ptr(), _p(nscale), rows_per_image, _stat(sums), M, C, int(relu), _p(gamma), _p(beta), groups, _stream())


def bn_bwd_apply(g, y, x, mi, gamma, sums, dx, M, C, relu, gmask=None, dgamma=None, dbeta=None, nscale=None,
                 rows_per_image=0, groups=1, relu_mask=None, beta=None, act_out=None):
    """relu == 2: the ReLU sign from x (needs beta); act_out (bf16 [M, C(view)]) then receives relu(BatchNorm(x))."""
    lib().call('rgda_bn_bwd_apply', g.data_ptr(), _ld(g), _p(y), _ld(y) if y is not None else 0, _p(relu_mask),
               x.data_ptr(), _ld(x),
               mi.data_ptr(), gamma.data_ptr(), _p(nscale), rows_per_image, _stat(sums), dx.data_ptr(), _ld(dx),
               _p(gmask), _ld(gmask) if gmask is not None else 0, _p(dgamma), _p(dbeta), M, C, int(relu), _p(beta),
               _p(act_out), _ld(act_out) if act_out is not None else 0, groups, _stream())


class _BnSmallFwd(ctypes.Structure):
    _fields_ = [(k, ctypes.c_void_p) for k in ('x', 'y', 'relu_mask', 'gamma', 'beta', 'mi', 'running_mean', 'running_var',
                                               'num_batches_tracked')] + [('M', ctypes.c_int64)] + \
               [(k, ctypes.c_int) for k in ('ldx', 'ldy', 'C', 'groups', 'relu')] + [('eps', ctypes.c_float), ('momentum', ctypes.c_float)]


class _BnSmallBwd(ctypes.Structure):
    _fields_ = [(k, ctypes.c_void_p) for k in ('g', 'y', 'relu_mask', 'x', 'dx', 'mi', 'gamma', 'dgamma', 'dbeta')] + \
               [('M', ctypes.c_int64)] + [(k, ctypes.c_int) for k in ('ldg', 'ldy', 'ldx', 'lddx', 'C', 'groups', 'relu')]


BN_SMALL_MAX_ROWS = 320         # rows of one statistics group the small-map BatchNorm kernels take (include/rgda_hip.h)


def bn_train_small(items, eps=1e-5, momentum=0.1):
    """Train-mode BatchNorm (+ ReLU) of several SMALL maps in one launch (rgda_bn_train_small).  items: (x, y, mi, rm, rv, nbt,
    gamma, beta, M, C, relu, groups, relu_mask) -- the tensors of bn_train_apply, without the convolution's accumulators (the
    kernel sums the stored values itself)."""
    if not items:
        return
    arr = (_BnSmallFwd * len(items))()
    for d, (x, y, mi, rm, rv, nbt, gamma, beta, M, C, relu, groups, rmask) in zip(arr, items):
        d.x, d.y, d.relu_mask, d.gamma, d.beta, d.mi = x.data_ptr(), y.data_ptr(), _p(rmask), gamma.data_ptr(), beta.data_ptr(), mi.data_ptr()
        d.running_mean, d.running_var, d.num_batches_tracked = _p(rm), _p(rv), _p(nbt)
        d.M, d.ldx, d.ldy, d.C, d.groups, d.relu, d.eps, d.momentum = M, _ld(x), _ld(y), C, groups, int(bool(relu)), eps, momentum
    lib().call('rgda_bn_train_small', ctypes.cast(arr, ctypes.c_void_p), len(items), _stream())


def bn_bwd_small(items):
    """BatchNorm backward (reduce + apply) of several SMALL maps in one launch (rgda_bn_bwd_small).  items: (g, y, x, mi, gamma,
    dx, dgamma, dbeta, M, C, relu, groups, relu_mask)."""
    if not items:
        return
    arr = (_BnSmallBwd * len(items))()
    for d, (g, y, x, mi, gamma, dx, dgamma, dbeta, M, C, relu, groups, rmask) in zip(arr, items):
        d.g, d.y, d.relu_mask, d.x, d.dx, d.mi, d.gamma = g.data_ptr(), _p(y), _p(rmask), x.data_ptr(), dx.data_ptr(), mi.data_ptr(), gamma.data_ptr()
        d.dgamma, d.dbeta = _p(dgamma), _p(dbeta)
        d.M, d.ldg, d.ldy, d.ldx, d.lddx = M, _ld(g), (_ld(y) if y is not None else 0), _ld(x), _ld(dx)
        d.C, d.groups, d.relu = C, groups, int(bool(relu))
    lib().call('rgda_bn_bwd_small', ctypes.cast(arr, ctypes.c_void_p), len(items), _stream())


def maxpool_fwd(x, y, idx, N, H, W, C, Ho, Wo):
    lib().call('rgda_maxpool_fwd', x.data_ptr(), y.data_ptr(), idx.data_ptr(), N, H, W, C, Ho, Wo, _stream())


def maxpool_fwd_bnin(bnop, x, y, idx, N, H, W, C, Ho, Wo):
    """MaxPool over relu(BatchNorm(x)) of the RAW stem convolution output (rgda_maxpool_fwd_bnin)."""
    lib().call('rgda_maxpool_fwd_bnin', bnop, x.data_ptr(), y.data_ptr(), idx.data_ptr(), N, H, W, C, Ho, Wo, _stream())


def maxpool_bwd(gy, idx, gx, N, H, W, C, Ho, Wo):
    lib().call('rgda_maxpool_bwd', gy.data_ptr(), idx.data_ptr(), gx.data_ptr(), N, H, W, C, Ho, Wo, _stream())


def instnorm_fwd(x, y0, y1, feat, mi, N, HW, C, eps=1e-5):
    ldy = _ld(y0) if y0 is not None else (_ld(y1) if y1 is not None else 0)
    lib().call('rgda_instnorm_fwd', x.data_ptr(), _ld(x), _p(y0), _p(y1), ldy, _p(feat), mi.data_ptr(), N, HW, C, eps,
               _stream())


def instnorm_bwd(ga, gb, gc, x, mi, dx, N, HW, C):
    ldg = _ld(ga) if ga is not None else (_ld(gb) if gb is not None else 0)
    lib().call('rgda_instnorm_bwd', _p(ga), _p(gb), ldg, _p(gc), _ld(gc) if gc is not None else 0, x.data_ptr(),
               _ld(x), mi.data_ptr(), dx.data_ptr(), _ld(dx), N, HW, C, _stream())


def spatial_mix_multi(ins, mats, out, N, I, C):
    """out[n][i][:] = sum_q mats[q][i,:] @ ins[q][n]  (q <= 4 sources, bf16 out)."""
    import ctypes
    n = len(ins)
    P = (ctypes.c_void_p * n)(*[t.data_ptr() for t in ins])
    L = (ctypes.c_int * n)(*[_ld(t) for t in ins])
    Mt = (ctypes.c_void_p * n)(*[m.data_ptr() for m in mats])
    J = (ctypes.c_int * n)(*[m.shape[1] for m in mats])
    for m in mats:
        assert m.shape[0] == I and m.is_contiguous() and m.dtype == torch.float32
    lib().call('rgda_spatial_mix_multi', n, P, L, Mt, J, out.data_ptr(), _ld(out), N, I, C, _stream())


def spatial_mix(inp, Mx, out, N, I, J, C, accumulate=False):
    assert Mx.shape == (I, J) and Mx.is_contiguous() and Mx.dtype == torch.float32
    lib().call('rgda_spatial_mix', inp.data_ptr(), _ld(inp), Mx.data_ptr(), out.data_ptr(), _ld(out), N, I, J, C,
               int(accumulate), int(out.dtype == torch.float32), _stream())


def group_mix(inp, W, out, G, I, J, C):
    """out[g][i][:] = sum_j W[i][j] * inp[g][j][:] for G groups of J consecutive rows (bf16 or f32 tensors)."""
    assert W.shape == (I, J) and W.is_contiguous() and W.dtype == torch.float32
    assert inp.shape[0] == G * J and out.shape[0] == G * I
    lib().call('rgda_group_mix', inp.data_ptr(), _ld(inp), int(inp.dtype == torch.float32), W.data_ptr(),
               out.data_ptr(), _ld(out), int(out.dtype == torch.float32), G, I, J, C, _stream())


def sparse_mix(ins, csr, outs, N, C):
    """outs[q][n][i][:] = sum_k vals[k] * ins[cols[k] >> 24][n][cols[k] & 0xffffff][:] over the CSR rows, which are
    split in order over the (<= 4) image-major output tensors.  csr = (rowptr int32, cols int32, vals f32) on the
    device; ins: <= 4 tensors of one dtype; outs: a tensor or a list of tensors of one dtype."""
    import ctypes
    rowptr, cols, vals = csr
    outs = [outs] if torch.is_tensor(outs) else list(outs)
    assert rowptr.dtype == torch.int32 and cols.dtype == torch.int32 and vals.dtype == torch.float32
    rows = [o.shape[0] // N for o in outs]
    assert rowptr.numel() == sum(rows) + 1 and all(o.shape[0] == N * r for o, r in zip(outs, rows))
    n, m = len(ins), len(outs)
    P = (ctypes.c_void_p * n)(*[t.data_ptr() for t in ins])
    L = (ctypes.c_int * n)(*[_ld(t) for t in ins])
    J = (ctypes.c_int * n)(*[t.shape[0] // N for t in ins])
    O = (ctypes.c_void_p * m)(*[t.data_ptr() for t in outs])
    OL = (ctypes.c_int * m)(*[_ld(t) for t in outs])
    OR = (ctypes.c_int * m)(*rows)
    lib().call('rgda_sparse_mix', n, P, L, J, int(ins[0].dtype == torch.float32), rowptr.data_ptr(), cols.data_ptr(),
               vals.data_ptr(), m, O, OL, OR, int(outs[0].dtype == torch.float32), N, C, _stream())


def classifier_fwd(hidden, w, bias, logits, N, HW, C, ncls):
    lib().call('rgda_classifier_fwd', hidden.data_ptr(), _ld(hidden), w.data_ptr(), bias.data_ptr(), logits.data_ptr(),
               N, HW, C, ncls, _stream())


def classifier_bwd(hidden, w, glogits, dhidden, dw, db, N, HW, C, ncls):
    L = lib()
    ws = _ws(L.size('rgda_classifier_bwd_workspace', N * HW, C, ncls), hidden.device)
    L.call('rgda_classifier_bwd', hidden.data_ptr(), _ld(hidden), w.data_ptr(), glogits.data_ptr(),
           dhidden.data_ptr(), _ld(dhidden), dw.data_ptr(), db.data_ptr(), N, HW, C, ncls, ws.data_ptr(), ws.numel(),
           _stream())


def _ptr_array(tensors):
    import ctypes
    return (ctypes.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])


def aspp_gather(z, biases, out1, out2, N, h, w, C, dils):
    """z bf16 [N*h*w, >= 72*C]; biases: eight f32 [C] tensors ([head][dilation]); out1/out2 f32 (N,C,h,w)."""
    import ctypes
    assert len(biases) == 8 and len(dils) == 4
    P = _ptr_array(biases)
    D = (ctypes.c_int * 4)(*[int(d) for d in dils])
    lib().call('rgda_aspp_gather', z.data_ptr(), _ld(z), ctypes.cast(P, ctypes.c_void_p), out1.data_ptr(),
               out2.data_ptr(), N, h, w, C, ctypes.cast(D, ctypes.c_void_p), _stream())


def aspp_scatter(g1, g2, dz, dbiases, N, h, w, C, dils):
    """g1/g2 f32 (N,C,h,w) contiguous -> dz bf16 [N*h*w, zc]; dbiases: eight f32 [C] tensors, accumulated."""
    import ctypes
    assert len(dbiases) == 8 and len(dils) == 4 and g1.is_contiguous() and g2.is_contiguous()
    P = _ptr_array(dbiases)
    D = (ctypes.c_int * 4)(*[int(d) for d in dils])
    lib().call('rgda_aspp_scatter', g1.data_ptr(), g2.data_ptr(), dz.data_ptr(), _ld(dz), dz.shape[1],
               ctypes.cast(P, ctypes.c_void_p), N, h, w, C, ctypes.cast(D, ctypes.c_void_p), _stream())


TRANSNORM_PLANE_MIN = 16      # s >= 16: threads along the planes; below: along the channels (csrc/transnorm_kernels.hip)


def _plane_view(x, who):
    """_feat_rows for a normalisation layer -> (f32 tensor, n, C, s, ld_channel, ld_sample): an NCHW map as there, or
    (n, C) rows read in place (s = 1) when the channels are contiguous, so that a column or row slice is not copied."""
    if x.dim() == 2:
        if x.dtype != torch.float32 or (x.shape[1] > 1 and x.stride(1) != 1) or (x.shape[0] > 1 and x.stride(0) < x.shape[1]):
            x = x.float().contiguous()
        n, C = x.shape
        return x, n, C, 1, 1, (x.stride(0) if n > 1 else C)
    x, n, s, ldc, ldb, C = _feat_rows(x, who)
    return x, n, C, s, ldc, ldb


def _plane_out(out, like, who):
    """The strides of an output map: `out` when given (f32, the shape of `like`, planes contiguous), else a new
    contiguous tensor -> (tensor, ld_channel, ld_sample)."""
    if out is None:
        out = torch.empty(like.shape, dtype=torch.float32, device=like.device)
    assert out.shape == like.shape and out.dtype == torch.float32 and out.is_cuda, (who, out.shape, out.dtype)
    o, n, C, s, ldc, ldb = _plane_view(out, who)
    if o.data_ptr() != out.data_ptr():
        raise ValueError(f'{who}: the output buffer needs contiguous planes (strides {out.stride()})')
    return out, ldc, ldb


def transnorm_forward(x, n_src, weight, bias, running, eps=1e-5, momentum=0.1, training=True, out=None):
    """_TransNorm.forward (regda/trans_norm.py:169-230) on rgda_transnorm_fwd.  x f32 (n, C, h, w) or (n, C), read in
    place through its strides when its planes are contiguous; the first n_src samples are the source half.  weight / bias
    f32 [C] or None; running: (running_mean_source, running_var_source, running_mean_target, running_var_target) f32 [C],
    updated in place when training, or None (training only).  Returns (y, saved): y f32 of x's shape (`out` when given: a
    buffer with contiguous planes, written in place) and saved f32 [5, C] = mean_s, rstd_s, mean_t, rstd_t, alpha for
    transnorm_backward."""
    _need_cuda(x, weight, bias, out, *(running or ()))
    x, n, C, s, ldc, ldb = _plane_view(x.detach(), 'transnorm_forward')
    y, ldcy, ldby = _plane_out(out, x, 'transnorm_forward')
    for t in (weight, bias) + tuple(running or ()):
        assert t is None or (t.dtype == torch.float32 and t.is_contiguous() and t.numel() == C), 'transnorm: f32 [C] vectors'
    rm_s, rv_s, rm_t, rv_t = running if running is not None else (None,) * 4
    saved = torch.empty((5, C), dtype=torch.float32, device=x.device)
    L = lib()
    ws = _ws(L.size('rgda_transnorm_fwd_workspace', n, int(n_src), C, s, int(bool(training))), x.device)
    L.call('rgda_transnorm_fwd', x.data_ptr(), n, int(n_src), C, s, ldc, ldb, _p(weight), _p(bias), _p(rm_s), _p(rv_s),
           _p(rm_t), _p(rv_t), float(eps), float(momentum), int(bool(training)), y.data_ptr(), ldcy, ldby, saved.data_ptr(),
           ws.data_ptr(), ws.numel(), _stream())
    return y, saved


def transnorm_backward(g, x, saved, n_src, weight, training=True, need_dx=True, need_dparams=True, dx=None):
    """The gradient of transnorm_forward (rgda_transnorm_bwd): g, x f32 of one shape, read in place like x there; saved:
    the forward's block.  Returns (dx, dweight, dbias): dx f32 of x's shape (`dx` when given) or None without need_dx,
    dweight / dbias f32 [C] or None without need_dparams."""
    _need_cuda(g, x, saved, weight, dx)
    assert g.shape == x.shape, (g.shape, x.shape)
    x, n, C, s, ldc, ldb = _plane_view(x.detach(), 'transnorm_backward')
    g, _, _, _, ldcg, ldbg = _plane_view(g.detach(), 'transnorm_backward')
    assert saved.shape == (5, C) and saved.dtype == torch.float32 and saved.is_contiguous()
    assert weight is None or (weight.dtype == torch.float32 and weight.is_contiguous() and weight.numel() == C)
    ldcd = ldbd = 0
    if need_dx or dx is not None:
        dx, ldcd, ldbd = _plane_out(dx, x, 'transnorm_backward')
    dw = db = None
    if need_dparams:
        dw = torch.empty(C, dtype=torch.float32, device=x.device)
        db = torch.empty(C, dtype=torch.float32, device=x.device)
    L = lib()
    ws = _ws(L.size('rgda_transnorm_bwd_workspace', n, int(n_src), C, s, int(bool(training))), x.device)
    L.call('rgda_transnorm_bwd', g.data_ptr(), ldcg, ldbg, x.data_ptr(), n, int(n_src), C, s, ldc, ldb, _p(weight),
           saved.data_ptr(), int(bool(training)), _p(dx), ldcd, ldbd, _p(dw), _p(db), ws.data_ptr(), ws.numel(), _stream())
    return dx, dw, db
