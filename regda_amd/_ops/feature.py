"""Stage-2 feature-space losses on one row scaffold (the Python side of csrc/feat_rows.h): prototype contrast
(csrc/align_kernels.hip), CORAL (csrc/coral_kernels.hip), MMD (csrc/mmd_kernels.hip), class-aware whitening
(csrc/whiten_kernels.hip), pixel contrast (csrc/contrast_kernels.hip) and the batch-hard triplet loss
(csrc/triplet_kernels.hip) -- small files of one or two entry points each, grouped."""
import torch

from .._lib import lib
from .base import _H, _need_cuda, _stream, _ws, _ws_unless


def _feat_rows(x, who):
    """The rows of a feature loss -> (f32 tensor, b, hw, ld_channel, ld_image, k): an NCHW (b, k, h, w) map, read in
    place through its channel and image strides when the pixels of an image are contiguous (NCHW, channel slices, batch
    slices) and copied otherwise (another dtype, channels-last); or (n, k) rows (n images of one pixel)."""
    if x.dim() == 2:
        x = x.contiguous().float()
        n, k = x.shape
        return x, n, 1, 1, k, k
    assert x.dim() == 4, f'{who}: NCHW (b, k, h, w) features or (n, k) rows'
    x = x.float()
    b, k, h, w = x.shape
    ldb, ldc = x.stride(0), x.stride(1)
    if not ((w == 1 or x.stride(3) == 1) and (h == 1 or x.stride(2) == w) and ldc >= h * w and (b == 1 or ldb >= ldc * k)):
        x = x.contiguous()
        ldb, ldc = k * h * w, h * w
    return x, b, h * w, ldc, ldb, k


def _grad_rows(g, n):
    """an optional gradient buffer: bf16 [n, >= k] pixel-major rows -> (pointer, leading dimension)"""
    if g is None:
        return 0, 0
    assert g.dtype == torch.bfloat16 and g.dim() == 2 and g.shape[0] == n and g.stride(1) == 1, (g.dtype, g.shape, n)
    return g.data_ptr(), g.stride(0)


def _loss_out(loss, device):
    return torch.zeros(1, device=device) if loss is None else loss


def pcl_flag(ws, class_num, k):
    """The int32 flag word of a workspace that rgda_pcl_loss has used (one host sync): bit 2 (value 4) a label outside
    [0, class_num) that is not ignore_label, bit 3 (value 8) a kept pixel whose loss is not finite (the loss reads NaN)."""
    off = (int(class_num) * int(k) * 4 + 255) // 256 * 256 + 4
    return int(ws[off:off + 4].view(torch.int32).item())


def pcl_loss(feat, labels, protos, temperature=8.0, ignore_label=-1, weight=1.0, loss=None, dfeat=None, accumulate=False,
             ws=None):
    """PrototypeContrastiveLoss forward (+ gradient w.r.t. feat into `dfeat` bf16 [b*h*w, K] when given).
    Returns the (accumulating) fp32 loss tensor.  `ws`: a caller-owned uint8 workspace of at least
    rgda_pcl_loss_workspace(C, K) bytes, whose flag word pcl_flag() reads afterwards; nothing here synchronises."""
    _need_cuda(feat, labels, protos)
    feat = feat.contiguous().float()
    b, K, h, w = feat.shape
    labels = labels.contiguous().view(b, h, w)
    assert labels.dtype == torch.int64 and protos.is_contiguous() and protos.dtype == torch.float32
    C = protos.shape[0]
    loss = _loss_out(loss, feat.device)
    L = lib()
    ws = _ws_unless(ws, feat.device, 'rgda_pcl_loss_workspace', C, K)
    assert ws.dtype == torch.uint8 and ws.is_cuda and ws.is_contiguous()
    L.call('rgda_pcl_loss', feat.data_ptr(), labels.data_ptr(), protos.data_ptr(), loss.data_ptr(),
           *_grad_rows(dfeat, b * h * w), int(bool(accumulate)), b, K, C, h, w, ignore_label, float(temperature),
           float(weight), ws.data_ptr(), ws.numel(), _stream())
    return loss


def coral_loss(feat_s, feat_t, weight=1.0, loss=None, dfeat_s=None, dfeat_t=None, accumulate=False):
    """CoralLoss(feat_s rows, feat_t rows) (regda/gast/coral.py, is_sqrt=False) as Aligner.align_domain computes it:
    feat_s / feat_t f32 NCHW (b, d, h, w) (the pixels are the rows) or (n, d).  loss (f32[1]) += weight * CORAL;
    dfeat_s / dfeat_t (optional) bf16 [n, >= d] pixel-major rows: (+)= weight * d CORAL / d feat (rgda_coral_loss).
    Returns the (accumulating) fp32 loss tensor."""
    _need_cuda(feat_s, feat_t, dfeat_s, dfeat_t)
    xs, bs, hws, lcs, lbs, d = _feat_rows(feat_s, 'coral_loss')
    xt, bt, hwt, lct, lbt, dt = _feat_rows(feat_t, 'coral_loss')
    if d != dt:
        raise ValueError(f'coral_loss: feature dimensions differ ({d} vs {dt})')
    loss = _loss_out(loss, xs.device)
    L = lib()
    ws = _ws(L.size('rgda_coral_loss_workspace', bs * hws, bt * hwt, d), xs.device)
    L.call('rgda_coral_loss', xs.data_ptr(), bs, hws, lcs, lbs, xt.data_ptr(), bt, hwt, lct, lbt, d, loss.data_ptr(),
           *_grad_rows(dfeat_s, bs * hws), *_grad_rows(dfeat_t, bt * hwt), int(bool(accumulate)), float(weight),
           ws.data_ptr(), ws.numel(), _stream())
    return loss


MMD_KERNEL_TYPES = {'rbf': _H['RGDA_MMD_RBF'], 'linear': _H['RGDA_MMD_LINEAR']}      # kernel_type of rgda_mmd_loss


def mmd_loss(feat_s, feat_t, weight=1.0, kernel_type='rbf', kernel_mul=2.0, kernel_num=5, fix_sigma=None, loss=None,
             dfeat_s=None, dfeat_t=None, accumulate=False):
    """MMDLoss(kernel_type, kernel_mul, kernel_num, fix_sigma)(feat_s rows, feat_t rows) (regda/gast/mmd.py):
    feat_s / feat_t f32 NCHW (b, d, h, w) (the pixels are the rows; batch slices of one map are read in place) or (n, d).
    loss (f32[1]) += weight * MMD; dfeat_s / dfeat_t (optional) bf16 [n, >= d] pixel-major rows:
    (+)= weight * d MMD / d feat (rgda_mmd_loss).  fix_sigma None or 0: the bandwidth is the mean pairwise squared
    distance, computed on the device.  Returns the (accumulating) fp32 loss tensor."""
    if kernel_type not in MMD_KERNEL_TYPES:
        raise ValueError(f"mmd_loss: kernel_type {kernel_type!r}; served are 'rbf' and 'linear'")
    _need_cuda(feat_s, feat_t, dfeat_s, dfeat_t)
    xs, bs, hws, lcs, lbs, d = _feat_rows(feat_s, 'mmd_loss')
    xt, bt, hwt, lct, lbt, dt = _feat_rows(feat_t, 'mmd_loss')
    if d != dt:
        raise ValueError(f'mmd_loss: feature dimensions differ ({d} vs {dt})')
    loss = _loss_out(loss, xs.device)
    L = lib()
    nbytes = L.size('rgda_mmd_loss_workspace', bs * hws, bt * hwt, d)
    if kernel_type == 'linear' and nbytes:
        nbytes = (12 * d + 255) // 256 * 256          # the linear form needs the means only (include/rgda_hip.h)
    ws = _ws(nbytes, xs.device)
    L.call('rgda_mmd_loss', xs.data_ptr(), bs, hws, lcs, lbs, xt.data_ptr(), bt, hwt, lct, lbt, d,
           MMD_KERNEL_TYPES[kernel_type], float(kernel_mul), int(kernel_num), float(fix_sigma or 0.0), loss.data_ptr(),
           *_grad_rows(dfeat_s, bs * hws), *_grad_rows(dfeat_t, bt * hwt), int(bool(accumulate)), float(weight),
           ws.data_ptr(), ws.numel(), _stream())
    return loss


WHITEN_BLOCKS = (32, 64, 96, 128)      # channels per group rgda_whiten_loss serves


def whiten_loss(feat, labels, class_num, groups, ignore_label=-1, weight=1.0, loss=None, dfeat=None, accumulate=False,
                check=False, return_ws=False):
    """ClassWareWhitening(range(class_num), groups)(feat, labels) (regda/gast/class_ware_whiten.py): feat f32
    (b, k, h, w), read in place through its channel and image strides when the pixels of an image are contiguous (NCHW,
    channel slices, batch slices), copied otherwise (another dtype, channels-last); labels int64 (b, h, w) or
    (b, 1, h, w) at feature resolution.  loss (f32[1]) += weight * L; dfeat
    (optional) bf16 [b*h*w, >= k] pixel-major rows: (+)= weight * dL / dfeat (rgda_whiten_loss; accumulate=False
    writes every row).  check=True reads the label-range flag back (one host sync) and raises ValueError on a label
    outside [0, class_num) that is not ignore_label.  Returns the (accumulating) fp32 loss tensor (and the workspace
    with return_ws: int32 word 0 is the flag, words 1..16 the per-class pixel counts)."""
    _need_cuda(feat, labels, dfeat)
    assert feat.dim() == 4, 'whiten_loss: NCHW (b, k, h, w) features'
    feat, b, hw, ldc, ldb, k = _feat_rows(feat, 'whiten_loss')
    assert labels.dtype == torch.int64 and labels.numel() == b * hw, (labels.dtype, labels.shape, feat.shape)
    labels = labels.contiguous().view(-1)
    loss = _loss_out(loss, feat.device)
    L = lib()
    ws = _ws(L.size('rgda_whiten_loss_workspace', b * hw, k, int(class_num), int(groups)), feat.device)
    L.call('rgda_whiten_loss', feat.data_ptr(), b, hw, ldc, ldb, labels.data_ptr(), k, int(class_num),
           int(groups), int(ignore_label), loss.data_ptr(), *_grad_rows(dfeat, b * hw), int(bool(accumulate)),
           float(weight), ws.data_ptr(), ws.numel(), _stream())
    if check and int(ws[:4].view(torch.int32).item()) & 4:
        raise ValueError('whiten_loss: a label is outside [0, class_num) and is not ignore_label')
    return (loss, ws) if return_ws else loss


PIXEL_CONTRAST_MAX_ROWS = 4096      # N = anchors * views rgda_pixel_contrast_loss serves


def pixel_contrast_select(labels, predict, class_num, size, ignore_label=-1, check=False):
    """The selection tables of PixelContrastLoss (regda/gast/contrastive.py): labels int64 (b, H, W), read at the
    nearest-downscaled positions of the (h, w) = size grid (H % h == 0 and W % w == 0); predict int64 (b, h, w), or f32
    logits (b, class_num, h, w) whose argmax is taken (the lowest index on ties).
    -> counts int32 [b, class_num, 2] (hard: predict != label, easy), order int32 [b, h*w] (per image the pixel indices
    stably sorted by (class, easy), ignored pixels last), flag int32 [1] (bit 2: a label outside [0, class_num) that is
    not ignore_label; check=True reads it back -- one host sync -- and raises ValueError)."""
    _need_cuda(labels, predict)
    h, w = int(size[0]), int(size[1])
    assert labels.dtype == torch.int64 and labels.dim() == 3, (labels.dtype, labels.shape)
    labels = labels.contiguous()
    b, H, W = labels.shape
    C = int(class_num)
    if predict.dtype == torch.int64:
        kind = 0
        assert predict.numel() == b * h * w, (predict.shape, (b, h, w))
    else:
        kind = 1
        assert predict.dtype == torch.float32 and tuple(predict.shape) == (b, C, h, w), (predict.dtype, predict.shape)
    predict = predict.contiguous()
    counts = torch.empty(b, C, 2, dtype=torch.int32, device=labels.device)
    order = torch.empty(b, h * w, dtype=torch.int32, device=labels.device)
    flag = torch.zeros(1, dtype=torch.int32, device=labels.device)
    lib().call('rgda_pixel_contrast_select', labels.data_ptr(), predict.data_ptr(), kind, b, C, H, W, h, w,
               int(ignore_label), counts.data_ptr(), order.data_ptr(), flag.data_ptr(), _stream())
    if check and int(flag.item()) & 4:
        raise ValueError('pixel_contrast_select: a label is outside [0, class_num) and is not ignore_label')
    return counts, order, flag


def pixel_contrast_loss(feat, order, counts, anchors, ranks, temperature=0.1, base_temperature=0.07, eps=1e-5, weight=1.0,
                        loss=None, dfeat=None, accumulate=False):
    """PixelContrastLoss._contrastive on the rows the tables select (rgda_pixel_contrast_loss): feat f32 (b, k, h, w),
    read in place through its channel and image strides; order / counts from pixel_contrast_select; anchors int32
    [A, 3] (image, class, hard_keep) and ranks int32 [A, n_view] from gast.contrastive.plan_anchors, on the device.
    loss (f32[1]) += weight * L; dfeat (optional) bf16 [b*h*w, >= k] pixel-major rows: (+)= weight * dL / dfeat
    (accumulate=False writes every row, the unselected ones as zeros).  Returns the (accumulating) fp32 loss tensor."""
    _need_cuda(feat, order, counts, anchors, ranks, dfeat)
    assert feat.dim() == 4, 'pixel_contrast_loss: NCHW (b, k, h, w) features'
    feat, b, hw, ldc, ldb, k = _feat_rows(feat, 'pixel_contrast_loss')
    C = counts.shape[1]
    for t in (order, counts, anchors, ranks):
        assert t.dtype == torch.int32 and t.is_contiguous(), (t.dtype, t.shape)
    assert tuple(order.shape) == (b, hw) and tuple(counts.shape) == (b, C, 2), (order.shape, counts.shape)
    A, n_view = ranks.shape
    assert tuple(anchors.shape) == (A, 3), anchors.shape
    loss = _loss_out(loss, feat.device)
    L = lib()
    ws = _ws(L.size('rgda_pixel_contrast_loss_workspace', A * n_view, k), feat.device)
    L.call('rgda_pixel_contrast_loss', feat.data_ptr(), b, hw, ldc, ldb, k, C, order.data_ptr(), counts.data_ptr(),
           anchors.data_ptr(), A, ranks.data_ptr(), n_view, float(temperature), float(base_temperature), float(eps),
           loss.data_ptr(), *_grad_rows(dfeat, b * hw), int(bool(accumulate)), float(weight), ws.data_ptr(), ws.numel(),
           _stream())
    return loss


TRIPLET_MAX_ROWS = 16384      # n rgda_triplet_loss serves


def _triplet_np(n):
    return (n + 127) // 128 * 128


def triplet_loss(feat, labels, margin=0.3, ignore_label=None, weight=1.0, loss=None, dfeat=None, accumulate=False,
                 return_ws=False):
    """TripletLoss(margin)(rows of feat, labels) (regda/gast/triple.py: batch-hard mining) on rgda_triplet_loss: feat f32
    NCHW (b, k, h, w) (the pixels are the rows; read in place through its channel and image strides) or (n, k) rows;
    labels int64 with n elements.  ignore_label None: every value is a label, as in the reference; an integer: rows with
    that label are neither anchors nor candidates and the mean runs over the others.  loss (f32[1]) += weight * L;
    dfeat (optional) bf16 [n, >= k] pixel-major rows: (+)= weight * dL / dfeat (accumulate=False writes every row).
    Fewer than two distinct labels among the valid rows: loss and gradient 0 (decided on the device).
    Returns (loss, stats): the (accumulating) fp32 loss tensor and int32 [2] on the device, (m = the rows the mean ran
    over, the number of positive hinges) -- a view of this call's workspace (with return_ws the workspace itself is
    returned as a third value; triplet_tables reads it)."""
    _need_cuda(feat, labels, dfeat)
    feat, b, hw, ldc, ldb, k = _feat_rows(feat, 'triplet_loss')
    n = b * hw
    assert labels.dtype == torch.int64 and labels.numel() == n, (labels.dtype, labels.shape, feat.shape)
    labels = labels.contiguous().view(-1)
    loss = _loss_out(loss, feat.device)
    L = lib()
    ws = _ws(L.size('rgda_triplet_loss_workspace', n, k), feat.device)
    L.call('rgda_triplet_loss', feat.data_ptr(), b, hw, ldc, ldb, labels.data_ptr(), k, float(margin),
           int(ignore_label is not None), int(ignore_label or 0), loss.data_ptr(),
           *_grad_rows(dfeat, n), int(bool(accumulate)), float(weight), ws.data_ptr(), ws.numel(), _stream())
    stats = ws[:8].view(torch.int32)
    return (loss, stats, ws) if return_ws else (loss, stats)


def triplet_tables(ws, n):
    """The per-row tables rgda_triplet_loss left in its workspace (the layout of include/rgda_hip.h), for diagnostics and
    tests: -> dict of [n] tensors: p, n (the selected positive / negative, -1: none), d_ap, d_an (0 where the pair carries
    no gradient), hinge."""
    v = _triplet_np(n) * 4
    def table(j, dtype):
        return ws[256 + j * v:256 + (j + 1) * v].view(dtype)[:n]
    return dict(p=table(2, torch.int32), n=table(3, torch.int32), d_ap=table(6, torch.float32),
                d_an=table(7, torch.float32), hinge=table(8, torch.float32))
