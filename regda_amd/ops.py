"""Thin tensor-level wrappers over the C ABI (include/rgda_hip.h).

Everything here takes/returns CUDA(ROCm) torch tensors, enqueues on
`torch.cuda.current_stream()` and never synchronises.  PyTorch is plumbing
(device memory + streams); the arithmetic is in librgda_hip.so.
"""
import ctypes
import math

import torch

from ._lib import lib


# The class counts every class-specific kernel serves (regda_amd/csrc/common.h: with_classes); other counts return
# RGDA_ERR_UNSUPPORTED, raised here as ValueError.
MIN_CLASSES, MAX_CLASSES = 6, 16


def check_class_count(c, who='class_num'):
    """ValueError unless MIN_CLASSES <= c <= MAX_CLASSES."""
    if not MIN_CLASSES <= int(c) <= MAX_CLASSES:
        raise ValueError(f'{who}: {c} classes; the kernels serve {MIN_CLASSES} <= class_num <= {MAX_CLASSES}')


_LDS_LOSS_ROW, _LDS_PCL, _LDS_REFINE = 0, 1, 2      # rgda_class_lds `which` (include/rgda_hip.h)


def check_step_shape(c, k, H, W, who='step'):
    """ValueError where a training step at c classes, k prototype channels and H x W tiles (logits at output stride 16)
    would reach a kernel that cannot serve it -- so that a step refuses before its first launch, never halfway.  The
    LDS needs and limits are the library's own (rgda_class_lds).  k None: a step without prototypes, the row pass only."""
    check_class_count(c, who)
    L = lib()
    w = (int(W) + 15) // 16
    row, lim = L.size('rgda_class_lds', _LDS_LOSS_ROW, c, w, W), L.size('rgda_class_lds_limit', _LDS_LOSS_ROW)
    if row > lim:
        raise ValueError(f'{who}: {c} classes at {W}-pixel rows need {row} B of LDS in the fused upsample + loss row pass, '
                         f'above its limit of {lim} B (16 classes: W <= 1008; 1024 x 1024 tiles serve up to 15)')
    if k is None:
        return
    for which, name in ((_LDS_PCL, 'PrototypeContrastiveLoss'), (_LDS_REFINE, 'label_refine')):
        need, lim = L.size('rgda_class_lds', which, c, k, 0), L.size('rgda_class_lds_limit', which)
        if need > lim:
            raise ValueError(f'{who}: {c} prototypes of {k} channels need {need} B of LDS in {name}, above the {lim} B '
                             f'of gfx950 (16 classes serve k = 2048)')


_STREAM = None      # cached raw hipStream_t of the stream selected with use_stream() (saves ~8 us per launch)


def _stream():
    return _STREAM if _STREAM is not None else torch.cuda.current_stream().cuda_stream


class use_stream:
    """`with ops.use_stream(s):` = `with torch.cuda.stream(s):` + caches the raw handle for the launches inside."""

    def __init__(self, stream):
        self.stream = stream
        self.ctx = torch.cuda.stream(stream)

    def __enter__(self):
        global _STREAM
        self.prev = _STREAM
        self.ctx.__enter__()
        _STREAM = self.stream.cuda_stream
        return self.stream

    def __exit__(self, *a):
        global _STREAM
        _STREAM = self.prev
        return self.ctx.__exit__(*a)


def _p(t):
    return 0 if t is None else t.data_ptr()


STAT_FRAC_FWD, STAT_FRAC_BWD = 26, 40       # RGDA_STAT_FRAC_FWD / _BWD (include/rgda_hip.h, checked by tests/test_abi.py)


def new_stats(*shape, device='cuda'):
    """A zeroed per-channel accumulator, rgda_stat_t[...][RGDA_STAT_REPLICAS][2][C] (64-bit fixed point)."""
    return torch.zeros(*shape, dtype=torch.int64, device=device)


def stats_value(stats, backward=False):
    """Accumulators -> float64 values (sum over nothing: the caller still adds up the replica axis)."""
    return stats.double() * 2.0 ** -(STAT_FRAC_BWD if backward else STAT_FRAC_FWD)


def _stat(t):
    if t is not None and t.dtype != torch.int64:
        raise TypeError('BatchNorm statistic accumulators are int64 fixed point (ops.new_stats), got %s' % t.dtype)
    return _p(t)


def _need_cuda(*ts):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise RuntimeError('regda_amd kernels run on the GPU only (there is no CPU fallback); '
                               'got a CPU tensor')


def _ws(nbytes, device):
    return torch.empty(max(int(nbytes), 16), dtype=torch.uint8, device=device)


def pseudo_select(soft, cutoff_top=0.8, cutoff_low=0.6, ignore_label=-1, classmax_ws=None, check=True):
    """soft (b,c,h,w) f32 -> (b,h,w) int64.  `classmax_ws`: workspace already holding the per-class
    maxima (from label_refine).  check=True reads the range flag back (one host sync, like the
    reference's assert, pseudo_generation.py:71)."""
    _need_cuda(soft)
    assert soft.dim() == 4 and soft.dtype == torch.float32
    soft = soft.contiguous()
    b, c, h, w = soft.shape
    out = torch.empty((b, h, w), dtype=torch.int64, device=soft.device)
    if out.numel() == 0:
        return out
    L = lib()
    if classmax_ws is None:
        ws = _ws(L.size('rgda_pseudo_select_workspace', b, c), soft.device)
        ready = 0
    else:
        ws, ready = classmax_ws, 1
    L.call('rgda_pseudo_select', soft.data_ptr(), out.data_ptr(), b, c, h * w, cutoff_top, cutoff_low,
           ignore_label, ready, ws.data_ptr(), ws.numel(), _stream())
    if check and h * w > 0:
        flag = ws[b * c * 4: b * c * 4 + 4].view(torch.int32)
        assert int(flag.item()) == 0, 'pseudo_selection: probabilities must lie in [0, 1]'
    return out


def lrh(labels, regions, percent, class_num, ignore_label, max_regions=4096, check=True, ws=None):
    """Homogenizer.forward.  labels/regions (b,h,w) int64 -> (b,h,w) int64 (bit-exact)."""
    _need_cuda(labels, regions)
    assert labels.dim() == 3
    assert labels.dtype == torch.int64 and regions.dtype == torch.int64 and labels.shape == regions.shape
    labels, regions = labels.contiguous(), regions.contiguous()
    b, h, w = labels.shape
    out = torch.empty_like(labels)
    if labels.numel() == 0:
        return out
    L = lib()
    need = L.size('rgda_lrh_workspace', b, max_regions, class_num)
    if ws is None or ws.numel() < need:
        ws = _ws(need, labels.device)
    L.call('rgda_lrh', labels.data_ptr(), regions.data_ptr(), out.data_ptr(), b, h * w, class_num, ignore_label,
           float(percent), max_regions, ws.data_ptr(), ws.numel(), _stream())
    if check and h * w > 0:
        off = (b * max_regions * class_num + b * max_regions) * 4
        flag = int(ws[off:off + 4].view(torch.int32).item())
        if flag & 1:
            raise ValueError(f'Homogenizer: a region id is outside [0, max_regions={max_regions})')
        if flag & 2:
            raise ValueError('Homogenizer: a label is outside [0, class_num) and is not ignore_label')
    return out


def pseudo_lrh(soft, classmax_ws, regions, cutoff_top, cutoff_low, percent, class_num, ignore_label, max_regions=4096, ws=None):
    """LRH(pseudo_selection(soft), regions) in one pass (rgda_pseudo_lrh): soft (b,c,h,w) f32, classmax_ws = the workspace
    holding the per-class maxima (label_refine(return_ws=True) / pseudo_select), regions (b,h,w) int64 -> (b,h,w) int64,
    and the workspace (flag word at byte offset (b*R*C + b*R)*4, as for lrh)."""
    _need_cuda(soft, regions)
    soft, regions = soft.contiguous(), regions.contiguous()
    b, c, h, w = soft.shape
    assert regions.shape == (b, h, w) and regions.dtype == torch.int64 and soft.dtype == torch.float32
    out = torch.empty((b, h, w), dtype=torch.int64, device=soft.device)
    L = lib()
    need = L.size('rgda_pseudo_lrh_workspace', b, h * w, max_regions, class_num)
    if ws is None or ws.numel() < need:
        ws = _ws(need, soft.device)
    L.call('rgda_pseudo_lrh', soft.data_ptr(), classmax_ws.data_ptr(), regions.data_ptr(), out.data_ptr(), b, h * w, class_num,
           cutoff_top, cutoff_low, ignore_label, float(percent), max_regions, ws.data_ptr(), ws.numel(), _stream())
    return out, ws


def masks_to_regions(masks, areas, area_threshold=1024):
    """masks (K,H,W) uint8 / bool, areas (K,) int64 -> (H,W) int32 region map (local_region_homog.py:51-56)."""
    _need_cuda(masks, areas)
    K, H, W = masks.shape
    masks = masks.contiguous().to(torch.uint8) if masks.dtype != torch.uint8 else masks.contiguous()
    areas = areas.contiguous().to(torch.int64)
    assert areas.shape == (K,)
    out = torch.empty((H, W), dtype=torch.int32, device=masks.device)
    if H * W == 0:
        return out
    lib().call('rgda_masks_to_regions', masks.data_ptr() if K else 0, areas.data_ptr() if K else 0, out.data_ptr(), K, H * W,
               int(area_threshold), _stream())
    return out


def label_refine(feat, protos, p1, p2, soft, temp=2.0, out=None, return_ws=False, views=3, return_sim=False):
    """views: bit 0 = prototype view, bit 1 = prediction view (3 = mode 'all'); inputs of a view that is off may be None.
    return_sim (with return_ws and the prototype view): also the similarity map 1 / pearson_dist (b,c,h,w) at the base of
    the workspace, what proto_pixel_weight takes as `sim` -> (out, classmax workspace, sim)."""
    pview, lview = bool(views & 1), bool(views & 2)
    assert views in (1, 2, 3)
    soft = soft.contiguous().float()
    _need_cuda(soft)
    b, c = soft.shape[:2]
    H, W = soft.shape[-2:]
    k = 4
    if pview:
        _need_cuda(feat, protos)
        feat, protos = feat.contiguous().float(), protos.contiguous().float()
        k = feat.shape[1]
        h, w = feat.shape[-2:]
        assert feat.shape[0] == b and protos.shape == (c, k)
    if lview:
        _need_cuda(p1, p2)
        p1, p2 = p1.contiguous().float(), p2.contiguous().float()
        h, w = p1.shape[-2:]
        assert p1.shape == (b, c, h, w) and p2.shape == (b, c, h, w)
        assert not pview or feat.shape[-2:] == (h, w)
    if out is None:
        out = torch.empty_like(soft)
    L = lib()
    ws = _ws(L.size('rgda_label_refine_workspace', b, c, h, w), soft.device)
    if views == 3:
        L.call('rgda_label_refine', feat.data_ptr(), protos.data_ptr(), p1.data_ptr(), p2.data_ptr(), soft.data_ptr(),
               out.data_ptr(), b, k, c, h, w, H, W, float(temp), ws.data_ptr(), ws.numel(), _stream())
    else:
        L.call('rgda_label_refine_views', _p(feat if pview else None), _p(protos if pview else None),
               _p(p1 if lview else None), _p(p2 if lview else None), soft.data_ptr(), out.data_ptr(), b, k, c, h, w, H, W,
               float(temp), views, ws.data_ptr(), ws.numel(), _stream())
    if return_ws:
        off = L.size('rgda_label_refine_classmax_offset', b, c, h, w)
        if return_sim:
            assert pview
            return out, ws[off:], ws[:b * c * h * w * 4].view(torch.float32).view(b, c, h, w)
        return out, ws[off:]
    return out


def label_refine_sup(feat, protos, p1, p2, soft, label_t_sup, temp=2.0, views=3, max_regions=65536, out=None, check=True,
                     return_ws=False):
    """label_refine with the superpixel view (rgda_label_refine_sup; alignment.py:238-258).  label_t_sup: int64 ids, b*H*W
    of them in any shape; views 3 = mode 'all', 0 = mode 's' (no other inputs needed).  check=True reads the range flag back
    (one host sync)."""
    pview, lview = bool(views & 1), bool(views & 2)
    assert views in (0, 1, 2, 3)
    soft = soft.contiguous().float()
    _need_cuda(soft, label_t_sup)
    b, c = soft.shape[:2]
    H, W = soft.shape[-2:]
    assert label_t_sup.dtype == torch.int64 and label_t_sup.numel() == b * H * W
    label_t_sup = label_t_sup.contiguous()
    k, h, w = 4, 1, 1
    if pview:
        _need_cuda(feat, protos)
        feat, protos = feat.contiguous().float(), protos.contiguous().float()
        k = feat.shape[1]
        h, w = feat.shape[-2:]
        assert feat.shape[0] == b and protos.shape == (c, k)
    if lview:
        _need_cuda(p1, p2)
        p1, p2 = p1.contiguous().float(), p2.contiguous().float()
        h, w = p1.shape[-2:]
        assert p1.shape == (b, c, h, w) and p2.shape == (b, c, h, w)
        assert not pview or feat.shape[-2:] == (h, w)
    if out is None:
        out = torch.empty_like(soft)
    L = lib()
    ws = _ws(L.size('rgda_label_refine_sup_workspace', b, c, h, w, max_regions), soft.device)
    L.call('rgda_label_refine_sup', _p(feat if pview else None), _p(protos if pview else None), _p(p1 if lview else None),
           _p(p2 if lview else None), soft.data_ptr(), label_t_sup.data_ptr(), out.data_ptr(), b, k, c, h, w, H, W,
           float(temp), views, max_regions, ws.data_ptr(), ws.numel(), _stream())
    if check:
        off = L.size('rgda_label_refine_sup_flag_offset', b, c, h, w, max_regions)
        if int(ws[off + 4:off + 8].view(torch.int32).item()):
            raise ValueError(f'label_refine: a superpixel id is outside [0, max_regions={max_regions})')
    if return_ws:
        off = L.size('rgda_label_refine_classmax_offset', b, c, h, w)
        return out, ws[off:]
    return out


def proto_flag_index(class_num, k):
    """Index (in float32 elements) of the int32 flag word behind sums[c][k] and cnt[c] in the statistics buffer of
    rgda_proto_stats / the workspace of rgda_proto_update: bit 2 is set by a label outside [0, class_num) that is not
    ignore_label."""
    return int(class_num) * int(k) + int(class_num)


def _proto_check(buf, class_num, k):
    i = proto_flag_index(class_num, k)
    if int(buf.view(torch.int32)[i].item()) & 2:
        raise ValueError('update_prototype: a label is outside [0, class_num) and is not ignore_label')


def proto_update(feat, label, protos, scale=16, ignore_label=-1, min_ratio=0.75, decay=0.996, check=False):
    """In-place EMA update of `protos`; returns the downscaled label (b,1,h,w) int64.  check=True reads the range flag
    back (one host sync) and raises ValueError for a label outside [0, class_num) that is not ignore_label, like
    ops.lrh; the default leaves the call enqueue-only."""
    _need_cuda(feat, label, protos)
    feat = feat.contiguous().float()
    label = label.contiguous()
    if label.dim() == 4:
        label = label.squeeze(1)
    assert protos.is_contiguous() and protos.dtype == torch.float32 and label.dtype == torch.int64
    b, k, h, w = feat.shape
    c = protos.shape[0]
    assert label.shape == (b, h * scale, w * scale), (label.shape, feat.shape)
    ds = torch.empty((b, 1, h, w), dtype=torch.int64, device=feat.device)
    L = lib()
    ws = _ws(L.size('rgda_proto_update_workspace', c, k), feat.device)
    L.call('rgda_proto_update', feat.data_ptr(), label.data_ptr(), protos.data_ptr(), ds.data_ptr(), b, k, c, h, w,
           scale, ignore_label, float(min_ratio), float(decay), ws.data_ptr(), ws.numel(), _stream())
    if check:
        _proto_check(ws[:(proto_flag_index(c, k) + 1) * 4].view(torch.float32), c, k)
    return ds


def downscale_label(label, class_num, scale=16, ignore_label=-1, min_ratio=0.75):
    """DownscaleLabel on its own: (b,H,W) or (b,1,H,W) int64 -> (b,1,H/scale,W/scale) int64.  The kernel fuses the
    downscale with the prototype pass, so it runs against a dummy 4-channel feature map and dummy prototypes, whose
    update is thrown away."""
    if label.dim() == 4:
        label = label.squeeze(1)
    b, H, W = label.shape
    feat = torch.zeros((b, 4, H // scale, W // scale), device=label.device)
    return proto_update(feat, label, torch.zeros((class_num, 4), device=label.device), scale, ignore_label, min_ratio, 0.5)


def proto_stats(feat, label, scale=16, ignore_label=-1, min_ratio=0.75, class_num=6, stats=None, check=False):
    """The sufficient statistics of update_prototype for data-parallel ranks (rgda_proto_stats): returns (stats, ds) --
    `stats` a float32 buffer whose first class_num * k + class_num elements are sums[c][k] and cnt[c] (what the ranks
    all-reduce), ds the downscaled label (b,1,h,w) int64.  The int32 flag word sits at element proto_flag_index(class_num,
    k); check=True reads it back (one host sync) and raises ValueError for an out-of-range label."""
    _need_cuda(feat, label)
    feat = feat.contiguous().float()
    label = label.contiguous()
    if label.dim() == 4:
        label = label.squeeze(1)
    assert label.dtype == torch.int64
    b, k, h, w = feat.shape
    assert label.shape == (b, h * scale, w * scale), (label.shape, feat.shape)
    ds = torch.empty((b, 1, h, w), dtype=torch.int64, device=feat.device)
    L = lib()
    nbytes = L.size('rgda_proto_update_workspace', class_num, k)
    if stats is None:
        stats = torch.empty((nbytes + 3) // 4, dtype=torch.float32, device=feat.device)
    assert stats.is_contiguous() and stats.dtype == torch.float32 and stats.numel() * 4 >= nbytes
    L.call('rgda_proto_stats', feat.data_ptr(), label.data_ptr(), ds.data_ptr(), b, k, class_num, h, w, scale, ignore_label,
           float(min_ratio), stats.data_ptr(), stats.numel() * 4, _stream())
    if check:
        _proto_check(stats, class_num, k)
    return stats, ds


def proto_apply(protos, stats, decay=0.996):
    """protos <- EMA(protos, sums / (cnt + 1e-7), kept where cnt < 1) from (all-reduced) statistics (rgda_proto_apply)."""
    _need_cuda(protos, stats)
    assert protos.is_contiguous() and protos.dtype == torch.float32 and stats.dtype == torch.float32
    c, k = protos.shape
    assert stats.numel() >= c * k + c
    lib().call('rgda_proto_apply', protos.data_ptr(), stats.data_ptr(), c, k, float(decay), _stream())


def fill_zero(t):
    """t.zero_() as a kernel of this library (contiguous tensor, 16-byte aligned storage)."""
    assert t.is_contiguous()
    lib().call('rgda_fill_zero', t.data_ptr(), t.numel() * t.element_size(), _stream())


def copy_multi(pairs):
    """[(dst, src), ...] (<= 4 pairs of contiguous tensors of equal byte size, multiples of 16) in ONE launch."""
    n = len(pairs)
    for d, s_ in pairs:
        assert d.is_contiguous() and s_.is_contiguous() and d.numel() * d.element_size() == s_.numel() * s_.element_size()
    D = (ctypes.c_void_p * n)(*[d.data_ptr() for d, _ in pairs])
    S = (ctypes.c_void_p * n)(*[s_.data_ptr() for _, s_ in pairs])
    B = (ctypes.c_size_t * n)(*[d.numel() * d.element_size() for d, _ in pairs])
    lib().call('rgda_copy_multi', n, ctypes.cast(D, ctypes.c_void_p), ctypes.cast(S, ctypes.c_void_p), ctypes.cast(B, ctypes.c_void_p),
               _stream())


def set_f32(t, value):
    lib().call('rgda_set_f32', t.data_ptr(), float(value), _stream())


def dropout_mask(out, p, seed):
    """out (f32, contiguous) = Dropout keep mask scaled by 1 / (1 - p), drawn from (seed, element index)."""
    lib().call('rgda_dropout_mask', out.data_ptr(), out.numel(), float(p), int(seed) & 0xFFFFFFFFFFFFFFFF, _stream())


def _upsample_operands(p1, p2, label, class_weight, want_grad, g1, g2):
    """The operands of a fused upsample + loss call: f32 contiguous logits, the int64 label, the loss and gradient
    outputs (g1 / g2 allocated unless given; None without gradients), the class weights."""
    p1, p2 = p1.contiguous().float(), p2.contiguous().float()
    label = label.contiguous()
    assert label.dtype == torch.int64
    loss = torch.empty(1, dtype=torch.float32, device=p1.device)
    if want_grad:
        g1 = torch.empty_like(p1) if g1 is None else g1
        g2 = torch.empty_like(p2) if g2 is None else g2
        assert g1.is_contiguous() and g2.is_contiguous() and g1.shape == p1.shape and g2.shape == p2.shape
    else:
        g1 = g2 = None
    cw = None if class_weight is None else class_weight.contiguous().float()
    return p1, p2, label, cw, loss, g1, g2


def upsample_ce(p1, p2, label, ignore_label=-1, class_weight=None, want_grad=True, g1=None, g2=None):
    """-> (loss f32[1], g1, g2) ; g = d loss / d p (None if not want_grad; written into the given g1 / g2 when passed)."""
    _need_cuda(p1, p2, label)
    p1, p2, label, cw, loss, g1, g2 = _upsample_operands(p1, p2, label, class_weight, want_grad, g1, g2)
    b, c, h, w = p1.shape
    H, W = label.shape[-2:]
    L = lib()
    ws = _ws(L.size('rgda_upsample_ce_workspace', b, c, h, w, H, W), p1.device)
    L.call('rgda_upsample_ce', p1.data_ptr(), p2.data_ptr(), label.data_ptr(), _p(cw), loss.data_ptr(), _p(g1),
           _p(g2), b, c, h, w, H, W, ignore_label, ws.data_ptr(), ws.numel(), _stream())
    return loss, g1, g2


# enum rgda_loss_kind (include/rgda_hip.h); 'gdp' is served by upsample_gdp (rgda_upsample_gdp), not by upsample_loss
LOSS_KINDS = {'ohem': 1, 'focal': 2, 'ghm': 3, 'ups': 4, 'uvem': 5, 'gdp': 6}


def upsample_loss(kind, p1, p2, label, soft=None, class_weight=None, acc_sum=None, m=0.2, t=0.7, gamma=4.0,
                  thresh=0.0, momentum=0.0, ignore_label=-1, want_grad=True, g1=None, g2=None, heads=2):
    """loss_calc(multi=True) with OhemCrossEntropy / FocalLoss / GHMLoss / UPSLoss / UVEMLoss (`kind` a key of
    LOSS_KINDS; rgda_upsample_loss) -> (loss f32[1], g1, g2).  soft: the full-resolution soft label (UPS / UVEM);
    acc_sum: GHM's device state f32[30], updated in place; class_weight: None or f32[2, C] (OHEM, UPS, UVEM).
    heads=1: one loss_fn call on one prediction (p2 must be p1; the gradient is then g1 + g2)."""
    _need_cuda(p1, p2, label, soft, class_weight, acc_sum)
    p1, p2, label, cw, loss, g1, g2 = _upsample_operands(p1, p2, label, class_weight, want_grad, g1, g2)
    b, c, h, w = p1.shape
    H, W = label.shape[-2:]
    if soft is not None:
        soft = soft.contiguous().float()
        assert soft.shape == (b, c, H, W)
    if acc_sum is not None:
        assert acc_sum.dtype == torch.float32 and acc_sum.is_contiguous() and acc_sum.numel() == 30
    k = LOSS_KINDS[kind]
    L = lib()
    ws = _ws(L.size('rgda_upsample_loss_workspace', k, b, c, h, w, H, W), p1.device)
    if heads == 1:
        p2 = p1
    L.call('rgda_upsample_loss', k, heads, p1.data_ptr(), p2.data_ptr(), label.data_ptr(), _p(soft), _p(cw), _p(acc_sum),
           float(m), float(t), float(gamma), float(thresh), float(momentum), loss.data_ptr(), _p(g1), _p(g2), b, c, h,
           w, H, W, ignore_label, ws.data_ptr(), ws.numel(), _stream())
    return loss, g1, g2


def upsample_gdp(p1, p2, label, acc_sum, bins_weight, pixel_weight=None, class_weight=None, momentum=0.99,
                 ignore_label=-1, want_grad=True, g1=None, g2=None, heads=2):
    """loss_calc(multi=True) with GDPLoss(bins=30) (rgda_upsample_gdp; balance.py:218-303) -> (loss f32[1], g1, g2).
    acc_sum: the loss's device state f32[30], updated in place once per head; bins_weight: f32[30], receives the bin
    weights of the last head call.  pixel_weight: None or f32[b*H*W], the prototype weight of every label pixel
    (proto_pixel_weight; prototype_refine), shared by both heads; class_weight: None or f32[2, C] (class_balance).
    heads=1: one call on one prediction (the gradient is then g1 + g2)."""
    _need_cuda(p1, p2, label, pixel_weight, class_weight, acc_sum, bins_weight)
    p1, p2, label, cw, loss, g1, g2 = _upsample_operands(p1, p2, label, class_weight, want_grad, g1, g2)
    b, c, h, w = p1.shape
    H, W = label.shape[-2:]
    for t in (acc_sum, bins_weight):
        assert t.dtype == torch.float32 and t.is_contiguous() and t.numel() == 30
    if pixel_weight is not None:
        assert pixel_weight.dtype == torch.float32 and pixel_weight.is_contiguous() and pixel_weight.numel() == b * H * W
    if cw is not None:
        assert cw.shape == (2, c)
    L = lib()
    ws = _ws(L.size('rgda_upsample_gdp_workspace', b, c, h, w, H, W), p1.device)
    if heads == 1:
        p2 = p1
    L.call('rgda_upsample_gdp', heads, p1.data_ptr(), p2.data_ptr(), label.data_ptr(), _p(pixel_weight), _p(cw),
           acc_sum.data_ptr(), bins_weight.data_ptr(), float(momentum), loss.data_ptr(), _p(g1), _p(g2), b, c, h, w, H, W,
           ignore_label, ws.data_ptr(), ws.numel(), _stream())
    return loss, g1, g2


REG_ENT, REG_KLD = 1, 2         # enum rgda_reg_term (include/rgda_hip.h)


def _pixel_map(t, b, H, W, who):
    """A caller's per-pixel weight map, (b, 1, H, W) or (b, H, W), as contiguous f32 (None stays None)."""
    if t is None:
        return None
    if tuple(t.shape) not in ((b, 1, H, W), (b, H, W)):
        raise ValueError(f'{who}: weight of shape {tuple(t.shape)}, expected ({b}, 1, {H}, {W}) or ({b}, {H}, {W})')
    return t.contiguous().float()


def upsample_reg(p1, p2, label=None, w_ent=None, w_kld=None, terms=REG_ENT | REG_KLD, lambda_ent=1.0, lambda_kld=1.0,
                 size=None, ignore_label=-1, want_grad=True, g1=None, g2=None, accumulate=False, empty_is_zero=False,
                 heads=2, loss=None):
    """IAST's entropy and KLD-to-uniform regularisers on the upsampled logits (rgda_upsample_reg; tools.py:376-398)
    -> (loss f32[2] = (ent, kld) unscaled, g1, g2).  w_ent / w_kld: a weight map (b, 1, H, W) or (b, H, W), or None =
    derived from `label` (int64 (b, H, W)): entropy on the ignored pixels, KLD on the labelled ones.  g1 / g2 receive
    (accumulate: are added) the gradient of 0.5 * (lambda_ent * ent + lambda_kld * kld) per head.  size: (H, W) when
    there is no label to take it from.  heads=1: one prediction (p2 must be p1; the gradient is then g1 + g2)."""
    _need_cuda(p1, p2, label, w_ent, w_kld)
    p1, p2 = p1.contiguous().float(), p2.contiguous().float()
    b, c, h, w = p1.shape
    if not 1 <= int(terms) <= (REG_ENT | REG_KLD):
        raise ValueError(f'upsample_reg: terms {terms!r}; REG_ENT, REG_KLD or both')
    derives = bool(terms & REG_ENT and w_ent is None) or bool(terms & REG_KLD and w_kld is None)
    if derives and label is None:
        raise ValueError('upsample_reg: a term without a weight map derives its mask from `label`, which is missing')
    # (H, W): given, else the label's, else that of the map of a term that is on (one exists: nothing is derived)
    used = [t for t, on in ((label, True), (w_ent, terms & REG_ENT), (w_kld, terms & REG_KLD)) if on and t is not None]
    H, W = (int(v) for v in (size if size is not None else used[0].shape[-2:]))
    if label is not None:
        if label.dtype != torch.int64 or tuple(label.shape) != (b, H, W):
            raise ValueError(f'upsample_reg: label {label.dtype} {tuple(label.shape)}, expected int64 ({b}, {H}, {W})')
        label = label.contiguous()
    w_ent, w_kld = _pixel_map(w_ent, b, H, W, 'upsample_reg'), _pixel_map(w_kld, b, H, W, 'upsample_reg')
    loss = torch.empty(2, dtype=torch.float32, device=p1.device) if loss is None else loss
    if want_grad:
        assert not accumulate or (g1 is not None and g2 is not None), 'accumulate adds onto given gradients'
        g1 = torch.empty_like(p1) if g1 is None else g1
        g2 = torch.empty_like(p2) if g2 is None else g2
        assert g1.is_contiguous() and g2.is_contiguous() and g1.shape == p1.shape and g2.shape == p2.shape
    else:
        g1 = g2 = None
    L = lib()
    ws = _ws(L.size('rgda_upsample_reg_workspace', b, c, h, w, H, W), p1.device)
    if heads == 1:
        p2 = p1
    L.call('rgda_upsample_reg', heads, p1.data_ptr(), p2.data_ptr(), _p(label), _p(w_ent), _p(w_kld), int(terms),
           float(lambda_ent), float(lambda_kld), int(bool(accumulate)), int(bool(empty_is_zero)), loss.data_ptr(), _p(g1),
           _p(g2), b, c, h, w, H, W, ignore_label, ws.data_ptr(), ws.numel(), _stream())
    return loss, g1, g2


PYCDA_MAX_LEVELS = 6


def pycda_sizes(sizes):
    """The level sizes of upsample_pycda as a tuple of ints; ValueError unless they are 1 to 6 powers of two in [2, 256],
    strictly increasing, optionally followed by one 0 (the whole image) -- what rgda_upsample_pycda refuses."""
    try:
        sizes = tuple(int(s) for s in sizes)
    except TypeError:
        raise ValueError(f'pycda sizes: {sizes!r} is not a sequence of ints') from None
    if not 1 <= len(sizes) <= PYCDA_MAX_LEVELS:
        raise ValueError(f'pycda sizes: {len(sizes)} levels; 1 to {PYCDA_MAX_LEVELS}')
    finite = sizes[:-1] if sizes[-1] == 0 else sizes
    for i, s in enumerate(finite):
        if s < 2 or s > 256 or s & (s - 1):
            raise ValueError(f'pycda sizes: {s}; a finite size is a power of two in [2, 256], 0 (the image) comes last')
        if i and s <= finite[i - 1]:
            raise ValueError(f'pycda sizes: {sizes} are not strictly increasing')
    return sizes


def upsample_pycda_workspace(p, soft_shape, sizes):
    """The workspace of upsample_pycda for logits like `p` and soft labels of shape `soft_shape`: a step allocates it
    once per shape and passes it as `ws=`."""
    sizes = pycda_sizes(sizes)
    b, c, h, w = p.shape
    H, W = (int(v) for v in soft_shape[-2:])
    arr = (ctypes.c_int * len(sizes))(*sizes)
    n = lib().size('rgda_upsample_pycda_workspace', b, c, h, w, H, W, arr, len(sizes))
    if n == 0:
        raise ValueError(f'upsample_pycda: no workspace for logits {tuple(p.shape)}, soft labels {tuple(soft_shape)}, sizes {sizes}')
    return _ws(n, p.device)


def upsample_pycda(p1, p2, soft, sizes, thresh=0.5, level_weight=None, weight=1.0, g1=None, g2=None, accumulate=False,
                   flag=None, want_grad=True, heads=2, loss=None, n_active=None, ws=None):
    """PyCDA's region pyramid term on the upsampled logits (rgda_upsample_pycda, include/rgda_hip.h)
    -> (loss f32[1 + L] = total, then the levels, unscaled; n_active int32[L]; g1; g2).  soft: the teacher's
    probabilities (b, c, H, W); sizes: the levels' region sides, powers of two in [2, 256], strictly increasing, optionally
    followed by 0 = the whole image; level_weight: L floats (default 1 / L each).  g1 / g2 receive (accumulate: are added)
    the gradient of 0.5 * weight * total per head.  flag: a device int32 word whose bit 0 is raised by a soft value
    outside [0, 1].  heads=1: one prediction (p2 must be p1; the gradient is then g1 + g2).  ValueError for what the
    entry point refuses."""
    _need_cuda(p1, p2, soft, flag)
    sizes = pycda_sizes(sizes)
    p1, p2 = p1.contiguous().float(), p2.contiguous().float()
    b, c, h, w = p1.shape
    if soft.dim() != 4 or soft.dtype != torch.float32 or tuple(soft.shape[:2]) != (b, c):
        raise ValueError(f'upsample_pycda: soft {soft.dtype} {tuple(soft.shape)}, expected float32 ({b}, {c}, H, W)')
    soft = soft.contiguous()
    H, W = soft.shape[-2:]
    nl = len(sizes)
    lw = None
    if level_weight is not None:
        if len(level_weight) != nl:
            raise ValueError(f'upsample_pycda: {len(level_weight)} level weights for {nl} levels')
        lw = (ctypes.c_float * nl)(*(float(v) for v in level_weight))
    if flag is not None:
        assert flag.dtype == torch.int32 and flag.numel() >= 1
    loss = torch.empty(1 + nl, dtype=torch.float32, device=p1.device) if loss is None else loss
    n_active = torch.empty(nl, dtype=torch.int32, device=p1.device) if n_active is None else n_active
    assert loss.dtype == torch.float32 and loss.numel() == 1 + nl and n_active.dtype == torch.int32 and n_active.numel() == nl
    if want_grad:
        assert not accumulate or (g1 is not None and g2 is not None), 'accumulate adds onto given gradients'
        g1 = torch.empty_like(p1) if g1 is None else g1
        g2 = torch.empty_like(p2) if g2 is None else g2
        assert g1.is_contiguous() and g2.is_contiguous() and g1.shape == p1.shape and g2.shape == p2.shape
    else:
        g1 = g2 = None
    L = lib()
    arr = (ctypes.c_int * nl)(*sizes)
    if ws is None:
        ws = _ws(L.size('rgda_upsample_pycda_workspace', b, c, h, w, H, W, arr, nl), p1.device)
    if heads == 1:
        p2 = p1
    L.call('rgda_upsample_pycda', heads, p1.data_ptr(), p2.data_ptr(), soft.data_ptr(), arr, lw, nl, float(thresh),
           float(weight), int(bool(accumulate)), loss.data_ptr(), n_active.data_ptr(), _p(g1), _p(g2), _p(flag), b, c, h, w,
           H, W, ws.data_ptr(), ws.numel(), _stream())
    return loss, n_active, g1, g2


def overlap_params(alpha=0.5, beta=0.5, gamma=1.0, smooth=0.0, who='upsample_overlap'):
    """The four parameters of the overlap term as floats; ValueError unless alpha, beta, smooth are finite and >= 0 and
    1 <= gamma <= 8 -- what rgda_upsample_overlap refuses."""
    try:
        alpha, beta, gamma, smooth = float(alpha), float(beta), float(gamma), float(smooth)
    except (TypeError, ValueError):
        raise ValueError(f'{who}: alpha, beta, gamma, smooth must be numbers') from None
    for name, v in (('alpha', alpha), ('beta', beta), ('smooth', smooth)):
        if not (math.isfinite(v) and v >= 0.0):
            raise ValueError(f'{who}: {name} {v!r}; finite and >= 0')
    if not 1.0 <= gamma <= 8.0:
        raise ValueError(f'{who}: gamma {gamma!r} outside [1, 8]')
    return alpha, beta, gamma, smooth


def upsample_overlap_workspace(p, label_shape):
    """The workspace of upsample_overlap for logits like `p` and labels of shape `label_shape`: a step allocates it once
    per shape and passes it as `ws=`."""
    b, c, h, w = p.shape
    H, W = (int(v) for v in label_shape[-2:])
    n = lib().size('rgda_upsample_overlap_workspace', b, c, h, w, H, W)
    if n == 0:
        raise ValueError(f'upsample_overlap: no workspace for logits {tuple(p.shape)}, labels {tuple(label_shape)}')
    return _ws(n, p.device)


def upsample_overlap(p1, p2, label, alpha=.5, beta=.5, gamma=1., smooth=0., weight=1., heads=2, ignore_label=-1, g1=None,
                     g2=None, accumulate=False, want_grad=True, loss=None, index=None, present=None, flag=None, ws=None):
    """The Dice / soft Jaccard / Tversky / focal-Tversky overlap term of the upsampled logits against hard labels
    (rgda_upsample_overlap, include/rgda_hip.h) -> (loss f32[1], unscaled; index f32 [heads, c] = the per-class soft
    overlap index T_c, 0 for an absent class; present int32 [c] = the class's valid pixels; g1; g2).  With N = TP + smooth
    and M = alpha FP + beta FN + 1e-7 summed over the valid pixels of the batch, T = N / (N + M) and the loss is the mean
    of (1 - T)^gamma over the classes that occur, then over the heads.  alpha = beta = 0.5: Dice, 1: Jaccard.  g1 / g2
    receive (accumulate: are added) the gradient of 0.5 * weight * loss per head.  flag: a device int32 word whose bit 0 is
    raised by a label outside [0, c) that is not ignore_label (it counts as ignored).  heads=1: one prediction (p2 must
    be p1; the gradient is then g1 + g2).  ValueError for what the entry point refuses."""
    _need_cuda(p1, p2, label, flag)
    alpha, beta, gamma, smooth = overlap_params(alpha, beta, gamma, smooth)
    weight = float(weight)
    if not (math.isfinite(weight) and weight >= 0.0):
        raise ValueError(f'upsample_overlap: weight {weight!r}; finite and >= 0')
    if heads not in (1, 2):
        raise ValueError(f'upsample_overlap: heads {heads!r}; 1 or 2')
    if p1.dim() != 4 or p2.shape != p1.shape:
        raise ValueError(f'upsample_overlap: logits {tuple(p1.shape)} and {tuple(p2.shape)}, expected two (b, c, h, w)')
    p1, p2 = p1.contiguous().float(), p2.contiguous().float()
    b, c, h, w = p1.shape
    if label.dim() != 3 or label.dtype != torch.int64 or label.shape[0] != b:
        raise ValueError(f'upsample_overlap: label {label.dtype} {tuple(label.shape)}, expected int64 ({b}, H, W)')
    label = label.contiguous()
    H, W = label.shape[-2:]
    dev = p1.device
    if flag is not None:
        assert flag.dtype == torch.int32 and flag.numel() >= 1
    loss = torch.empty(1, dtype=torch.float32, device=dev) if loss is None else loss
    index = torch.empty(heads, c, dtype=torch.float32, device=dev) if index is None else index
    present = torch.empty(c, dtype=torch.int32, device=dev) if present is None else present
    assert loss.dtype == torch.float32 and loss.numel() == 1
    assert index.dtype == torch.float32 and index.is_contiguous() and tuple(index.shape) == (heads, c)
    assert present.dtype == torch.int32 and present.is_contiguous() and present.numel() == c
    if want_grad:
        assert not accumulate or (g1 is not None and g2 is not None), 'accumulate adds onto given gradients'
        g1 = torch.empty_like(p1) if g1 is None else g1
        g2 = torch.empty_like(p2) if g2 is None else g2
        assert g1.is_contiguous() and g2.is_contiguous() and g1.shape == p1.shape and g2.shape == p2.shape
    else:
        g1 = g2 = None
    L = lib()
    if ws is None:
        ws = upsample_overlap_workspace(p1, label.shape)
    if heads == 1:
        p2 = p1
    L.call('rgda_upsample_overlap', heads, p1.data_ptr(), p2.data_ptr(), label.data_ptr(), alpha, beta, gamma, smooth,
           weight, int(bool(accumulate)), loss.data_ptr(), index.data_ptr(), present.data_ptr(), _p(g1), _p(g2), _p(flag), b,
           c, h, w, H, W, int(ignore_label), ws.data_ptr(), ws.numel(), _stream())
    return loss, index, present, g1, g2


IAST_BINS = 0x7C01      # RGDA_IAST_BINS: the non-negative fp16 bit patterns 0 .. 0x7C00


def _align256(x):
    return (x + 255) & ~255


def iast_workspace(n, c, H, W, device):
    check_class_count(c, 'iast')
    return _ws(lib().size('rgda_iast_workspace', n, c, H, W), device)


def iast_views(ws, n, c, H, W):
    """The pieces of an IAST workspace -> (hist int32 [c, IAST_BINS], maxp f32 [n, H, W], arg uint8 [n, H, W])."""
    npix = n * H * W
    o1 = _align256(c * IAST_BINS * 4)
    o2 = o1 + _align256(npix * 4)
    return (ws[:c * IAST_BINS * 4].view(torch.int32).view(c, IAST_BINS), ws[o1:o1 + npix * 4].view(torch.float32).view(n, H, W),
            ws[o2:o2 + npix].view(n, H, W))


def iast_hist(probs, ws=None):
    """probs f32 (n, c, H, W) in [0, 1] -> the workspace holding the per-pixel first argmax, its value and the per-class
    fp16 histogram of the values (rgda_iast_hist; iast_views reads them)."""
    _need_cuda(probs)
    assert probs.dim() == 4 and probs.dtype == torch.float32
    probs = probs.contiguous()
    n, c, H, W = probs.shape
    ws = iast_workspace(n, c, H, W, probs.device) if ws is None else ws
    lib().call('rgda_iast_hist', probs.data_ptr(), n, c, H, W, ws.data_ptr(), ws.numel(), _stream())
    return ws


def iast_percentile(ws, prepend, q):
    """-> f32 [c]: np.percentile([prepend[k]] + class k's fp16 confidences, 100 * q[k]) per class (rgda_iast_percentile).
    prepend, q: device f64 [c]."""
    _need_cuda(ws, prepend, q)
    assert prepend.dtype == q.dtype == torch.float64 and prepend.is_contiguous() and q.is_contiguous()
    c = prepend.numel()
    assert q.numel() == c
    out = torch.empty(c, dtype=torch.float32, device=ws.device)
    lib().call('rgda_iast_percentile', prepend.data_ptr(), q.data_ptr(), out.data_ptr(), c, ws.data_ptr(), ws.numel(),
               _stream())
    return out


def iast_label(ws, cls_thresh, n, H, W, out=None):
    """-> uint8 (n, H, W): argmax + 1, 0 where the confidence is below its class's threshold (rgda_iast_label).
    cls_thresh: device f64 [c]."""
    _need_cuda(ws, cls_thresh)
    assert cls_thresh.dtype == torch.float64 and cls_thresh.is_contiguous()
    out = torch.empty((n, H, W), dtype=torch.uint8, device=ws.device) if out is None else out
    lib().call('rgda_iast_label', cls_thresh.data_ptr(), out.data_ptr(), n, cls_thresh.numel(), H, W, ws.data_ptr(),
               ws.numel(), _stream())
    return out


ANALYSIS_MAX_BINS = 256     # RGDA_ANALYSIS_MAX_BINS


def analysis_views(tables, b, c, R):
    """The pieces of a rgda_pseudo_analysis buffer -> (used int64 [b, R + 1, c], hit [b, R + 1, c], inbin [b, R + 1],
    diff24 [b, R + 1], flag int32 [1]).  Row R holds the pixels whose entropy is NaN."""
    rows = R + 1
    T = rows * (2 * c + 2)
    t = tables[:b * T * 8].view(torch.int64).view(b, T)
    return (t[:, :rows * c].view(b, rows, c), t[:, rows * c:2 * rows * c].view(b, rows, c),
            t[:, 2 * rows * c:2 * rows * c + rows], t[:, 2 * rows * c + rows:], tables[b * T * 8:b * T * 8 + 4].view(torch.int32))


def pseudo_analysis(soft, gt, lo, hi, cutoff_top, cutoff_low, ignore_label, tables=None):
    """soft f32 (b, c, H, W), gt int64 (b, H, W), lo / hi f32 [R] (the bin edges) -> the buffer holding the batch's
    per-image entropy-binned tables (rgda_pseudo_analysis; analysis_views reads them).  soft may be a contiguous view
    that starts anywhere in its buffer."""
    _need_cuda(soft, gt, lo, hi)
    assert soft.dim() == 4 and soft.dtype == torch.float32 and gt.dtype == torch.int64
    assert lo.dtype == hi.dtype == torch.float32 and lo.shape == hi.shape and lo.dim() == 1
    soft, gt, lo, hi = soft.contiguous(), gt.contiguous(), lo.contiguous(), hi.contiguous()
    b, c, H, W = soft.shape
    assert gt.shape == (b, H, W), 'gt must be (b, H, W) for soft (b, c, H, W)'
    check_class_count(c, 'pseudo_analysis')
    L = lib()
    need = L.size('rgda_pseudo_analysis_workspace', b, c, lo.numel())
    if tables is None or tables.numel() < need:
        tables = _ws(need, soft.device)
    L.call('rgda_pseudo_analysis', soft.data_ptr(), gt.data_ptr(), lo.data_ptr(), hi.data_ptr(), b, c, H, W, lo.numel(),
           cutoff_top, cutoff_low, ignore_label, tables.data_ptr(), tables.numel(), _stream())
    return tables


def pseudo_analysis_state(c, R, device):
    """A zeroed running state for pseudo_analysis_fold (rgda_pseudo_analysis_fold_workspace bytes)."""
    check_class_count(c, 'pseudo_analysis')
    return torch.zeros(lib().size('rgda_pseudo_analysis_fold_workspace', c, R), dtype=torch.uint8, device=device)


def pseudo_analysis_fold(tables, b, c, R, state):
    """Adds the b images of a pseudo_analysis buffer to the running state, in image order (rgda_pseudo_analysis_fold)."""
    _need_cuda(tables, state)
    lib().call('rgda_pseudo_analysis_fold', tables.data_ptr(), tables.numel(), b, c, R, state.data_ptr(), state.numel(),
               _stream())
    return state


def pseudo_analysis_state_views(state, c, R):
    """The pieces of a running state (any device) -> dict of total_used / total_hit [R + 1, c], total_inbin /
    total_diff24 [R + 1], acc_sum / diffi_sum f64 [R], images, acc_cnt / diffi_cnt int32 [R], flag."""
    rows = R + 1
    T = rows * (2 * c + 2)
    o = T * 8
    tot = state[:o].view(torch.int64)
    f = state[o:o + 16 * R].view(torch.float64)
    i = state[o + 16 * R + 8:o + 16 * R + 8 + 8 * R + 4].view(torch.int32)
    return dict(total_used=tot[:rows * c].view(rows, c), total_hit=tot[rows * c:2 * rows * c].view(rows, c),
                total_inbin=tot[2 * rows * c:2 * rows * c + rows], total_diff24=tot[2 * rows * c + rows:],
                acc_sum=f[:R], diffi_sum=f[R:], images=state[o + 16 * R:o + 16 * R + 8].view(torch.int64),
                acc_cnt=i[:R], diffi_cnt=i[R:2 * R], flag=i[2 * R:])


def proto_pixel_weight(feat, protos, label, sim=None, ignore_label=-1, out=None):
    """Aligner.get_prototype_weight_4pixel (rgda_proto_pixel_weight; alignment.py:267-281) -> f32 [b*H*W]: the prototype
    agreement of every label pixel with its own label, 0 where the label is ignored.  feat (b,k,h,w), protos (c,k),
    label int64 (b,H,W).  sim: the similarity map (b,c,h,w) a label_refine call with the prototype view has already
    computed (label_refine(..., return_sim=True)): the similarity pass is skipped and feat / protos may be None."""
    _need_cuda(feat, protos, label, sim)
    label = label.contiguous()
    assert label.dtype == torch.int64 and label.dim() == 3
    b, H, W = label.shape
    L = lib()
    if sim is not None:
        assert sim.dtype == torch.float32 and sim.is_contiguous() and sim.dim() == 4 and sim.shape[0] == b
        c, (h, w), k = sim.shape[1], sim.shape[-2:], 0
        ws = None
    else:
        feat, protos = feat.contiguous().float(), protos.contiguous().float()
        k, (h, w), c = feat.shape[1], feat.shape[-2:], protos.shape[0]
        assert feat.shape[0] == b and protos.shape == (c, k)
        ws = _ws(L.size('rgda_proto_pixel_weight_workspace', b, c, k, h, w), label.device)
    if out is None:
        out = torch.empty(b * H * W, dtype=torch.float32, device=label.device)
    assert out.dtype == torch.float32 and out.is_contiguous() and out.numel() == b * H * W
    L.call('rgda_proto_pixel_weight', _p(feat if sim is None else None), _p(protos if sim is None else None), _p(sim),
           label.data_ptr(), out.data_ptr(), b, k, c, h, w, H, W, ignore_label, _p(ws), 0 if ws is None else ws.numel(),
           _stream())
    return out


def teacher_probs(p1, p2, size):
    _need_cuda(p1, p2)
    p1, p2 = p1.contiguous().float(), p2.contiguous().float()
    b, c, h, w = p1.shape
    H, W = size
    out = torch.empty((b, c, H, W), dtype=torch.float32, device=p1.device)
    lib().call('rgda_teacher_probs', p1.data_ptr(), p2.data_ptr(), out.data_ptr(), b, c, h, w, H, W, _stream())
    return out


def class_count(label, class_num):
    _need_cuda(label)
    label = label.contiguous()
    cnt = torch.zeros(class_num, dtype=torch.int32, device=label.device)
    lib().call('rgda_class_count', label.data_ptr(), cnt.data_ptr(), label.numel(), class_num, _stream())
    return cnt


# --------------------------------------------------------------------------- conv stack
# Activations are torch.bfloat16 2-D tensors [N*H*W, ld] ("PxC"); a view with a column offset is
# expressed by passing a slice of the buffer (data_ptr of the slice) and its row stride.

def _ld(t):
    assert t.dim() == 2 and t.stride(1) == 1
    return t.stride(0)


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


def sumsq(g, out, ws):
    lib().call('rgda_sumsq', g.data_ptr(), g.numel(), out.data_ptr(), ws.data_ptr(), _stream())


def sgd_step(p, g, v, shadow, p_bf16, gnorm_sq, lr_dev, momentum, weight_decay, max_norm, gscale, ema_decay,
             first_step, shadow_bf16=None):
    lib().call('rgda_sgd_step', p.data_ptr(), g.data_ptr(), v.data_ptr(), _p(shadow), _p(p_bf16), _p(shadow_bf16),
               gnorm_sq.data_ptr(),
               lr_dev.data_ptr(), p.numel(), momentum, weight_decay, max_norm, gscale, ema_decay, int(first_step),
               _stream())


def weight_transpose_bf16(w, wt, Co, T, Ci):
    lib().call('rgda_weight_transpose_bf16', w.data_ptr(), wt.data_ptr(), Co, T, Ci, _stream())


def weight_transpose_batched(table, n, total_blocks):
    lib().call('rgda_weight_transpose_batched', table.data_ptr(), n, total_blocks, _stream())


def cast_bf16(src, dst):
    lib().call('rgda_cast_bf16', src.data_ptr(), dst.data_ptr(), src.numel(), _stream())


def cast_f32(src, dst):
    lib().call('rgda_cast_f32', src.data_ptr(), dst.data_ptr(), dst.numel(), _stream())


def ddp_accumulate_bf16(recv, world, out):
    lib().call('rgda_ddp_accumulate_bf16', recv.data_ptr(), world, out.data_ptr(), out.numel(), _stream())


def pad_cast_bf16(src, dst, R, K, Kp):
    lib().call('rgda_pad_cast_bf16', src.data_ptr(), dst.data_ptr(), R, K, Kp, _stream())


def unpad_acc_f32(src, dst, R, K, Kp):
    lib().call('rgda_unpad_acc_f32', src.data_ptr(), dst.data_ptr(), R, K, Kp, _stream())


def add_bf16(a, b, out, M, C):
    lib().call('rgda_add_bf16', a.data_ptr(), _ld(a), b.data_ptr(), _ld(b), out.data_ptr(), _ld(out), M, C, _stream())


# ----------------------------------------------------------------------------- teacher / pseudo-label harness
def dihedral(src, hflip, k, flip_first, dst=None, scale=1.0, accumulate=False):
    """One TTA view (rgda_dihedral_nchw): fp32 NCHW; returns dst (allocated when None)."""
    _need_cuda(src)
    n, c, h, w = src.shape
    k = k % 4
    ho, wo = (w, h) if (k & 1) else (h, w)
    if dst is None:
        assert not accumulate
        dst = torch.empty(n, c, ho, wo, device=src.device)
    assert src.is_contiguous() and dst.is_contiguous() and src.dtype == dst.dtype == torch.float32
    assert tuple(dst.shape) == (n, c, ho, wo)
    lib().call('rgda_dihedral_nchw', src.data_ptr(), dst.data_ptr(), n, c, h, w, int(bool(hflip)), k, int(bool(flip_first)),
               float(scale), int(bool(accumulate)), _stream())
    return dst


def window_crop(full, y1, x1, h, w, Th, Tw):
    n, c, Hf, Wf = full.shape
    tile = torch.empty(n, c, Th, Tw, device=full.device)
    lib().call('rgda_window_crop', full.data_ptr(), tile.data_ptr(), n, c, Hf, Wf, y1, x1, h, w, Th, Tw, _stream())
    return tile


def window_accumulate(tile, full, count, y1, x1, h, w):
    n, c, Hf, Wf = full.shape
    lib().call('rgda_window_accumulate', tile.data_ptr(), full.data_ptr(), count.data_ptr(), n, c, Hf, Wf, y1, x1, h, w,
               tile.shape[2], tile.shape[3], _stream())


def window_normalise(full, count):
    n, c, Hf, Wf = full.shape
    lib().call('rgda_window_normalise', full.data_ptr(), count.data_ptr(), n, c, Hf, Wf, _stream())


def window_gather(src, windows, tile, views=1, lut=None, out=None, flag=None):
    """rgda_window_gather: the network input of K windows, [K*views][C][Th][Tw] f32.  src: f32 [n][C][H][W], or uint8
    [n][H][W][3] with `lut` (f32 [3][256] device table); windows: device int32 [K][3] rows (image, y1, x1); tile =
    (Th, Tw); views 1 or 8 (tta_predict's order)."""
    _need_cuda(src, windows, lut, out, flag)
    th, tw = tile
    if src.dtype == torch.uint8:
        n, H, W, c = src.shape
        if c != 3 or lut is None:
            raise ValueError('window_gather: a uint8 source is [n][H][W][3] and needs lut')
        f32, u8 = None, src.contiguous()
    else:
        if src.dtype != torch.float32 or src.dim() != 4:
            raise ValueError('window_gather: the source is f32 [n][C][H][W] or uint8 [n][H][W][3]')
        n, c, H, W = src.shape
        f32, u8 = src.contiguous(), None
    if windows.dtype != torch.int32 or windows.dim() != 2 or windows.shape[1] != 3 or not windows.is_contiguous():
        raise ValueError('window_gather: windows must be a contiguous int32 [K][3] table')
    k = windows.shape[0]
    if out is None:
        out = torch.empty(k * views, c, th, tw, device=src.device)
    assert tuple(out.shape) == (k * views, c, th, tw) and out.dtype == torch.float32 and out.is_contiguous()
    lib().call('rgda_window_gather', _p(f32), _p(u8), _p(lut), windows.data_ptr(), k, views, n, c, H, W, th, tw,
               out.data_ptr(), _p(flag), _stream())
    return out


def window_gather_scaled(src, windows, tile, scaled_size, views=1, lut=None, out=None, flag=None):
    """rgda_window_gather_scaled: window_gather on the (Hs, Ws) = `scaled_size` image resize_bilinear_ac would make of the
    normalised source, without storing it; windows index the scaled image.  Arguments as window_gather."""
    _need_cuda(src, windows, lut, out, flag)
    th, tw = tile
    hs, ws = (int(v) for v in scaled_size)
    if src.dtype == torch.uint8:
        if src.dim() != 4 or src.shape[3] != 3 or lut is None:
            raise ValueError('window_gather_scaled: a uint8 source is [n][H][W][3] and needs lut')
        n, H, W, c = src.shape
        f32, u8 = None, src.contiguous()
    else:
        if src.dtype != torch.float32 or src.dim() != 4:
            raise ValueError('window_gather_scaled: the source is f32 [n][C][H][W] or uint8 [n][H][W][3]')
        n, c, H, W = src.shape
        f32, u8 = src.contiguous(), None
    if windows.dtype != torch.int32 or windows.dim() != 2 or windows.shape[1] != 3 or not windows.is_contiguous():
        raise ValueError('window_gather_scaled: windows must be a contiguous int32 [K][3] table')
    k = windows.shape[0]
    if out is None:
        out = torch.empty(k * views, c, th, tw, device=src.device)
    assert tuple(out.shape) == (k * views, c, th, tw) and out.dtype == torch.float32 and out.is_contiguous()
    lib().call('rgda_window_gather_scaled', _p(f32), _p(u8), _p(lut), windows.data_ptr(), k, views, n, c, H, W, hs, ws, th,
               tw, out.data_ptr(), _p(flag), _stream())
    return out


def scale_merge(full_s, count_s, acc, cnt):
    """rgda_scale_merge: acc [n][C][H][W] += resize_bilinear_ac(full_s / count_s, (H, W)), cnt [n][1][H][W] += 1; full_s
    [n][C][Hs][Ws] and count_s [n][1][Hs][Ws] are one scale's window sums and visit counts, left as they are."""
    _need_cuda(full_s, count_s, acc, cnt)
    n, c, hs, ws = full_s.shape
    H, W = acc.shape[-2:]
    if tuple(count_s.shape) != (n, 1, hs, ws) or tuple(acc.shape) != (n, c, H, W) or tuple(cnt.shape) != (n, 1, H, W):
        raise ValueError('scale_merge: full_s %s, count_s %s, acc %s, cnt %s' %
                         (tuple(full_s.shape), tuple(count_s.shape), tuple(acc.shape), tuple(cnt.shape)))
    assert full_s.dtype == count_s.dtype == acc.dtype == cnt.dtype == torch.float32
    assert full_s.is_contiguous() and count_s.is_contiguous() and acc.is_contiguous() and cnt.is_contiguous()
    lib().call('rgda_scale_merge', full_s.data_ptr(), count_s.data_ptr(), n, c, hs, ws, H, W, acc.data_ptr(), cnt.data_ptr(),
               _stream())


def window_scatter(pred, windows, full, count, rows, views=1, flag=None):
    """rgda_window_scatter: full [n][C][H][W] / count [n][1][H][W] += the K windows of pred [K*views][C][Th][Tw], in table
    order.  rows = (row0, nrows): the span of the flattened n*H image rows the windows cover."""
    _need_cuda(pred, windows, full, count, flag)
    n, c, H, W = full.shape
    kv, cp, th, tw = pred.shape
    k = windows.shape[0]
    if kv != k * views or cp != c or tuple(count.shape) != (n, 1, H, W):
        raise ValueError('window_scatter: pred %s, %d windows x %d views, full %s, count %s' %
                         (tuple(pred.shape), k, views, tuple(full.shape), tuple(count.shape)))
    assert pred.dtype == full.dtype == count.dtype == torch.float32 and windows.dtype == torch.int32
    assert full.is_contiguous() and count.is_contiguous() and windows.is_contiguous()
    lib().call('rgda_window_scatter', pred.contiguous().data_ptr(), windows.data_ptr(), k, views, n, c, H, W, th, tw,
               int(rows[0]), int(rows[1]), full.data_ptr(), count.data_ptr(), _p(flag), _stream())


def window_finish(full, count, labels=None, y_true=None, cm=None, flag=None):
    """rgda_window_finish: full /= count in place, then (optionally) the argmax into `labels` (uint8 or int64 [n][H][W],
    written in place) and the confusion matrix cm int64 [C][C] of the pixels with y_true >= 0 (int64 [n][H][W])."""
    _need_cuda(full, count, labels, y_true, cm, flag)
    n, c, H, W = full.shape
    assert full.is_contiguous() and count.is_contiguous() and tuple(count.shape) == (n, 1, H, W)
    u8 = i64 = None
    if labels is not None:
        assert tuple(labels.shape) == (n, H, W) and labels.is_contiguous()
        if labels.dtype == torch.uint8:
            u8 = labels
        elif labels.dtype == torch.int64:
            i64 = labels
        else:
            raise ValueError('window_finish: labels are uint8 or int64')
    yt = None
    if y_true is not None:
        yt = y_true.to(full.device, torch.int64).contiguous()
        assert yt.numel() == n * H * W and cm is not None and cm.dtype == torch.int64 and tuple(cm.shape) == (c, c)
    lib().call('rgda_window_finish', full.data_ptr(), count.data_ptr(), n, c, H, W, _p(u8), _p(i64), _p(yt), _p(cm),
               _p(flag), _stream())
    return labels


def resize_bilinear_ac(src, size):
    n, c, h, w = src.shape
    dst = torch.empty(n, c, size[0], size[1], device=src.device)
    lib().call('rgda_resize_bilinear_ac', src.contiguous().data_ptr(), dst.data_ptr(), n, c, h, w, size[0], size[1], _stream())
    return dst


def pad_rows(src, top, bottom):
    n, c, h, w = src.shape
    dst = torch.empty(n, c, h + top + bottom, w, device=src.device)
    lib().call('rgda_pad_rows_nchw', src.contiguous().data_ptr(), dst.data_ptr(), n, c, h, w, top, bottom, _stream())
    return dst


# ----------------------------------------------------------------------------- training augmentation of raw tiles
def check_augment_params(params, hi, wi, ho, wo):
    """Host-side check of a CPU int32 [N][4] (y0, x0, d, 0) table: the crop lies inside the hi x wi input, d in 0..7,
    and a transposing (odd) d only for a square output.  Raises ValueError."""
    p = params.numpy()
    if p.ndim != 2 or p.shape[1] != 4:
        raise ValueError('augment params must be [N][4], got %s' % (tuple(p.shape),))
    y0, x0, d = p[:, 0], p[:, 1], p[:, 2]
    if (y0 < 0).any() or (x0 < 0).any() or (y0 > hi - ho).any() or (x0 > wi - wo).any():
        raise ValueError('augment crop outside the %d x %d input' % (hi, wi))
    if (d < 0).any() or (d > 7).any() or ((d & 1).astype(bool) & (ho != wo)).any():
        raise ValueError('augment element d outside 0..7, or odd d with a non-square %d x %d output' % (ho, wo))


def augment_tiles(img, params, lut, size, label=None, label_lut=None, soft=None, regs=None, out=None, flag=None):
    """rgda_augment_tiles: crop + dihedral element + normalisation / label tables of N raw tiles, one launch.
    img uint8 [N][Hi][Wi][3]; label uint8 [N][Hi][Wi]; soft f32 [N][C][Hi][Wi]; regs int32 [N][Hi][Wi] (each optional but
    img, on the GPU); params int32 [N][4] (y0, x0, d, 0): a CPU tensor is checked (check_augment_params) and copied on
    the current stream, a device tensor is used as it is; lut f32 [3][256], label_lut int32 [256] device tables;
    size = (Ho, Wo).  out: {'image', 'label', 'soft', 'regs'} device tensors to write into (allocated where missing).
    flag: optional device int32 tensor, set to 1 by a sample whose device-side params are invalid.
    -> {'image': f32 [N][3][Ho][Wo], 'label': int64 [N][Ho][Wo], 'soft': f32 [N][C][Ho][Wo], 'regs': int64 [N][1][Ho][Wo]}
    (None where the input is None)."""
    _need_cuda(img, label, soft, regs, lut, label_lut)
    n, hi, wi, three = img.shape
    ho, wo = size
    if three != 3 or img.dtype != torch.uint8:
        raise ValueError('augment_tiles: img must be uint8 [N][H][W][3]')
    want = dict(label=(label, torch.uint8, (n, hi, wi)), regs=(regs, torch.int32, (n, hi, wi)),
                soft=(soft, torch.float32, (n, soft.shape[1] if soft is not None else 0, hi, wi)))
    for k, (t, dt, shape) in want.items():
        if t is not None and (t.dtype != dt or tuple(t.shape) != shape):
            raise ValueError('augment_tiles: %s must be %s %s, got %s %s' % (k, dt, shape, t.dtype, tuple(t.shape)))
    if label is not None and label_lut is None:
        raise ValueError('augment_tiles: a label needs label_lut')
    if not params.is_cuda:
        check_augment_params(params, hi, wi, ho, wo)
        params = params.to(img.device, torch.int32, non_blocking=True)
    assert params.dtype == torch.int32 and tuple(params.shape) == (n, 4)
    c = soft.shape[1] if soft is not None else 0
    shapes = dict(image=((n, 3, ho, wo), torch.float32, img), label=((n, ho, wo), torch.int64, label),
                  soft=((n, c, ho, wo), torch.float32, soft), regs=((n, 1, ho, wo), torch.int64, regs))
    res = {}
    for k, (shape, dt, src) in shapes.items():
        t = None if out is None else out.get(k)
        if src is None:
            res[k] = None
            continue
        if t is None:
            t = torch.empty(shape, dtype=dt, device=img.device)
        assert tuple(t.shape) == shape and t.dtype == dt and t.is_contiguous(), k
        res[k] = t
    ptr = lambda t: None if t is None else t.contiguous().data_ptr()
    lib().call('rgda_augment_tiles', ptr(img), ptr(label), ptr(soft), ptr(regs), ptr(params), n, hi, wi, c, ho, wo,
               ptr(lut), ptr(label_lut), ptr(res['image']), ptr(res['label']), ptr(res['soft']), ptr(res['regs']),
               ptr(flag), _stream())
    return res


AFFINE_A_MAX = 131072           # |a_kl| <= 4 * 32768: rgda_augment_affine takes scales inside [1/4, 4]


def check_affine_params(params, hi, wi):
    """Host-side check of a CPU int32 [N][8] (cy, cx, a00, a01, a10, a11, fill, 0) table, the device-side row check of
    rgda_augment_affine: |a_kl| <= 131072, the centre inside [0, hi * 65536] x [0, wi * 65536], fill below 2^24 and
    column 7 zero.  Raises ValueError."""
    p = params.numpy()
    if p.ndim != 2 or p.shape[1] != 8:
        raise ValueError('affine params must be [N][8], got %s' % (tuple(p.shape),))
    if (abs(p[:, 2:6].astype('int64')) > AFFINE_A_MAX).any():
        raise ValueError('affine matrix entry outside +-%d (a scale outside [1/4, 4])' % AFFINE_A_MAX)
    if (p[:, 0] < 0).any() or (p[:, 0] > hi * 65536).any() or (p[:, 1] < 0).any() or (p[:, 1] > wi * 65536).any():
        raise ValueError('affine crop centre outside the %d x %d input' % (hi, wi))
    if (p[:, 6] < 0).any() or (p[:, 6] >> 24).any() or (p[:, 7] != 0).any():
        raise ValueError('affine fill must be r | g << 8 | b << 16 and column 7 zero')


def augment_affine(img, params, lut, size, label=None, label_lut=None, ignore_label=-1, soft=None, regs=None, out=None,
                   flag=None):
    """rgda_augment_affine: one affine warp per sample (random scale / rotation) + normalisation / label tables of N raw
    tiles, one launch.  Arguments as augment_tiles, except params int32 [N][8] (cy, cx, a00, a01, a10, a11, fill, 0) (a
    CPU tensor is checked by check_affine_params), up to 16 soft planes, a size that may exceed the input, and
    ignore_label: the label of a pixel whose source lies outside the input (its regions are 0, its soft label all 0,
    its image the fill colour).
    -> {'image': f32 [N][3][Ho][Wo], 'label': int64 [N][Ho][Wo], 'soft': f32 [N][C][Ho][Wo], 'regs': int64 [N][1][Ho][Wo]}
    (None where the input is None)."""
    _need_cuda(img, label, soft, regs, lut, label_lut)
    n, hi, wi, three = img.shape
    ho, wo = size
    if three != 3 or img.dtype != torch.uint8:
        raise ValueError('augment_affine: img must be uint8 [N][H][W][3]')
    want = dict(label=(label, torch.uint8, (n, hi, wi)), regs=(regs, torch.int32, (n, hi, wi)),
                soft=(soft, torch.float32, (n, soft.shape[1] if soft is not None else 0, hi, wi)))
    for k, (t, dt, shape) in want.items():
        if t is not None and (t.dtype != dt or tuple(t.shape) != shape):
            raise ValueError('augment_affine: %s must be %s %s, got %s %s' % (k, dt, shape, t.dtype, tuple(t.shape)))
    if label is not None and label_lut is None:
        raise ValueError('augment_affine: a label needs label_lut')
    if not params.is_cuda:
        check_affine_params(params, hi, wi)
        params = params.to(img.device, torch.int32, non_blocking=True)
    assert params.dtype == torch.int32 and tuple(params.shape) == (n, 8)
    c = soft.shape[1] if soft is not None else 0
    shapes = dict(image=((n, 3, ho, wo), torch.float32, img), label=((n, ho, wo), torch.int64, label),
                  soft=((n, c, ho, wo), torch.float32, soft), regs=((n, 1, ho, wo), torch.int64, regs))
    res = {}
    for k, (shape, dt, src) in shapes.items():
        t = None if out is None else out.get(k)
        if src is None:
            res[k] = None
            continue
        if t is None:
            t = torch.empty(shape, dtype=dt, device=img.device)
        assert tuple(t.shape) == shape and t.dtype == dt and t.is_contiguous(), k
        res[k] = t
    ptr = lambda t: None if t is None else t.contiguous().data_ptr()
    lib().call('rgda_augment_affine', ptr(img), ptr(label), ptr(soft), ptr(regs), ptr(params), n, hi, wi, c, ho, wo,
               ptr(lut), ptr(label_lut), int(ignore_label), ptr(res['image']), ptr(res['label']), ptr(res['soft']),
               ptr(res['regs']), ptr(flag), _stream())
    return res


# ----------------------------------------------------------------------------- cross-domain mixing
MIX_CLASS, MIX_BOX = 0, 1       # rgda_mix_mode (include/rgda_hip.h)
MIX_MAX_CLASSES = 32            # one bit of class_bits per class


def mix_class_bits(classes, class_num):
    """The class set of rgda_domain_mix as its bit mask; ValueError for an id outside [0, class_num)."""
    bits = 0
    for c in classes:
        c = int(c)
        if not 0 <= c < class_num:
            raise ValueError('domain_mix: class id %d outside [0, %d)' % (c, class_num))
        bits |= 1 << c
    return bits


def domain_mix(images_s, label_s, images_t, label_t=None, soft_t=None, regs_t=None, classes=None, box=None,
               ignore_label=-1, check=False, class_num=None, flag=None):
    """rgda_domain_mix: paste the source pixels a predicate selects over the target tensors IN PLACE, one launch.
    images_s, images_t f32 (N,3,H,W); label_s int64 (N,H,W) or (N,1,H,W); optional targets label_t int64 (N,H,W) or
    (N,1,H,W), soft_t f32 (N,C,H,W), regs_t int64 (N,H,W) or (N,1,H,W).  Exactly one of
      classes: an iterable of class ids -- the pixels whose source label is one of them (ClassMix), or
      box = (y0, y1, x0, x1) -- the pixels of rows [y0, y1) and columns [x0, x1) (CutMix).
    A pasted pixel takes the source image and label, a one-hot soft label and region id 0.  class_num: the class count
    the labels are checked against (default: soft_t's C, else 32, the most the kernel serves).  flag: optional device
    int32 tensor, set to 1 by a source label that is neither a class nor ignore_label; check=True reads it back (one
    host synchronisation, as pseudo_select does) and raises ValueError.  The target tensors must be contiguous (they
    are written in place); anything but f32 images and int64 labels is a ValueError.
    -> (images_t, label_t, soft_t, regs_t)."""
    _need_cuda(images_s, label_s, images_t, label_t, soft_t, regs_t, flag)
    if (classes is None) == (box is None):
        raise ValueError('domain_mix: give exactly one of classes= and box=')
    if images_t.dim() != 4 or images_t.shape[1] != 3 or tuple(images_s.shape) != tuple(images_t.shape):
        raise ValueError('domain_mix: images must both be (N,3,H,W), got %s and %s'
                         % (tuple(images_s.shape), tuple(images_t.shape)))
    n, _, h, w = images_t.shape
    maps = ((n, h, w), (n, 1, h, w))
    c = int(class_num) if class_num is not None else (soft_t.shape[1] if soft_t is not None else MIX_MAX_CLASSES)
    want = (('images_s', images_s, torch.float32, None), ('images_t', images_t, torch.float32, None),
            ('label_s', label_s, torch.int64, maps), ('label_t', label_t, torch.int64, maps),
            ('soft_t', soft_t, torch.float32, ((n, c, h, w),)), ('regs_t', regs_t, torch.int64, maps))
    for name, t, dt, shapes in want:
        if t is None:
            continue
        if t.dtype != dt or (shapes is not None and tuple(t.shape) not in shapes):
            raise ValueError('domain_mix: %s must be %s %s, got %s %s' % (name, dt, shapes, t.dtype, tuple(t.shape)))
        if not name.endswith('_s') and not t.is_contiguous():
            raise ValueError('domain_mix: %s is written in place and must be contiguous' % name)
    if not 1 <= c <= MIX_MAX_CLASSES:
        raise ValueError('domain_mix: %d classes; the kernel serves 1..%d' % (c, MIX_MAX_CLASSES))
    if classes is not None:
        mode, bits, (y0, y1, x0, x1) = MIX_CLASS, mix_class_bits(classes, c), (0, 0, 0, 0)
    else:
        mode, bits, (y0, y1, x0, x1) = MIX_BOX, 0, (int(v) for v in box)
    if n * h * w == 0:
        return images_t, label_t, soft_t, regs_t
    if check and flag is None:
        flag = torch.zeros(1, dtype=torch.int32, device=images_t.device)
    lib().call('rgda_domain_mix', images_s.contiguous().data_ptr(), label_s.contiguous().data_ptr(), images_t.data_ptr(),
               _p(label_t) or None, _p(soft_t) or None, _p(regs_t) or None, n, c, h, w, mode, bits, y0, y1, x0, x1,
               int(ignore_label), _p(flag) or None, _stream())
    if check and int(flag.item()) != 0:
        raise ValueError('domain_mix: a source label is neither in [0, %d) nor ignore_label %d' % (c, ignore_label))
    return images_t, label_t, soft_t, regs_t


MIX_TABLE_COLS = 8              # RGDA_MIX_TABLE_COLS: {class_bits, y0, y1, x0, x1, 0, 0, 0} per image
MIX_WRITE_MAX_IMAGES = 16       # RGDA_MIX_WRITE_MAX_IMAGES


def _mix_table_check(who, table, n):
    if table.dtype != torch.int32 or tuple(table.shape) != (n, MIX_TABLE_COLS) or not table.is_contiguous():
        raise ValueError('%s: table must be contiguous torch.int32 (%d, %d), got %s %s'
                         % (who, n, MIX_TABLE_COLS, table.dtype, tuple(table.shape)))


def domain_mix_table(images_s, label_s, table, mode, images_in=None, images_out=None, label_t=None, soft_t=None,
                     ignore_label=-1, class_num=None, flag=None):
    """rgda_domain_mix_table: rgda_domain_mix with image n's predicate from row n of `table` (int32 (N, 8) on the
    device: class_bits, y0, y1, x0, x1, 0, 0, 0; mode MIX_CLASS / MIX_BOX says which columns count) and the image out of
    place: images_out[n] = cond ? images_s[n] : images_in[n], every pixel written, images_in never.  Both None: no image
    work (the call that pastes labels).  label_t int64 (N,H,W) or (N,1,H,W) and soft_t f32 (N,C,H,W) are pasted in place
    as ops.domain_mix does.  Same dtype, shape and contiguity checks as ops.domain_mix; flag: optional device int32.
    -> (images_out, label_t, soft_t)."""
    _need_cuda(images_s, label_s, table, images_in, images_out, label_t, soft_t, flag)
    if (images_in is None) != (images_out is None):
        raise ValueError('domain_mix_table: give images_in and images_out together, or neither')
    if images_s.dim() != 4 or images_s.shape[1] != 3:
        raise ValueError('domain_mix_table: images_s must be (N,3,H,W), got %s' % (tuple(images_s.shape),))
    n, _, h, w = images_s.shape
    maps = ((n, h, w), (n, 1, h, w))
    c = int(class_num) if class_num is not None else (soft_t.shape[1] if soft_t is not None else MIX_MAX_CLASSES)
    img = (tuple(images_s.shape),)
    want = (('images_s', images_s, torch.float32, img), ('images_in', images_in, torch.float32, img),
            ('images_out', images_out, torch.float32, img), ('label_s', label_s, torch.int64, maps),
            ('label_t', label_t, torch.int64, maps), ('soft_t', soft_t, torch.float32, ((n, c, h, w),)))
    for name, t, dt, shapes in want:
        if t is None:
            continue
        if t.dtype != dt or tuple(t.shape) not in shapes:
            raise ValueError('domain_mix_table: %s must be %s %s, got %s %s' % (name, dt, shapes, t.dtype, tuple(t.shape)))
        if name in ('images_out', 'label_t', 'soft_t') and not t.is_contiguous():
            raise ValueError('domain_mix_table: %s is written and must be contiguous' % name)
    if not 1 <= c <= MIX_MAX_CLASSES:
        raise ValueError('domain_mix_table: %d classes; the kernel serves 1..%d' % (c, MIX_MAX_CLASSES))
    if mode not in (MIX_CLASS, MIX_BOX):
        raise ValueError('domain_mix_table: mode must be MIX_CLASS or MIX_BOX, got %r' % (mode,))
    _mix_table_check('domain_mix_table', table, n)
    if n * h * w == 0:
        return images_out, label_t, soft_t
    lib().call('rgda_domain_mix_table', images_s.contiguous().data_ptr(), label_s.contiguous().data_ptr(),
               images_in.contiguous().data_ptr() if images_in is not None else None, _p(images_out) or None,
               _p(label_t) or None, _p(soft_t) or None, table.data_ptr(), n, c, h, w, int(mode), int(ignore_label),
               _p(flag) or None, _stream())
    return images_out, label_t, soft_t


def mix_select_classes(label_s, ranks, table, ws=None, ignore_label=-1, flag=None):
    """rgda_mix_select_classes, the DACS draw on the device: table[n][0] <- the bit set of the (P + 1) // 2 classes of
    smallest ranks[n][c] among the P classes of [0, C) that occur in label_s[n].  label_s int64 (N,H,W) or (N,1,H,W);
    ranks uint8 (N, C), every row a permutation of 0..C-1; table int32 (N, 8), its other columns are left alone.
    ws: N int32 words of workspace (allocated unless given; the call clears it).  No host readback.  -> (table, ws)."""
    _need_cuda(label_s, ranks, table, ws, flag)
    if label_s.dtype != torch.int64 or label_s.dim() not in (3, 4) or (label_s.dim() == 4 and label_s.shape[1] != 1):
        raise ValueError('mix_select_classes: label_s must be torch.int64 (N,H,W) or (N,1,H,W), got %s %s'
                         % (label_s.dtype, tuple(label_s.shape)))
    n, h, w = label_s.shape[0], label_s.shape[-2], label_s.shape[-1]
    if ranks.dtype != torch.uint8 or ranks.dim() != 2 or ranks.shape[0] != n or not ranks.is_contiguous():
        raise ValueError('mix_select_classes: ranks must be contiguous torch.uint8 (%d, C), got %s %s'
                         % (n, ranks.dtype, tuple(ranks.shape)))
    c = ranks.shape[1]
    if not 1 <= c <= MIX_MAX_CLASSES:
        raise ValueError('mix_select_classes: %d classes; the kernel serves 1..%d' % (c, MIX_MAX_CLASSES))
    _mix_table_check('mix_select_classes', table, n)
    if ws is None:
        ws = torch.empty(max(n, 4), dtype=torch.int32, device=label_s.device)
    if ws.dtype != torch.int32 or ws.numel() < n or not ws.is_contiguous():
        raise ValueError('mix_select_classes: ws must be contiguous torch.int32 with at least %d words' % n)
    if n * h * w == 0:
        return table, ws
    lib().call('rgda_mix_select_classes', label_s.contiguous().data_ptr(), ranks.data_ptr(), table.data_ptr(),
               ws.data_ptr(), n, c, h, w, int(ignore_label), _p(flag) or None, _stream())
    return table, ws


def mix_write_table(table, class_num, class_bits=0, box=(0, 0, 0, 0), ranks=None, ranks_host=None):
    """rgda_mix_write_table: every row of table (int32 (N, 8), N <= 16) <- {class_bits, *box, 0, 0, 0}, and ranks (uint8
    (N, C) on the device) <- ranks_host (a uint8 numpy array of that shape), both carried in the launch's arguments: the
    host buffer is read before this returns.  All defaults: the empty table."""
    _need_cuda(table, ranks)
    n = table.shape[0]
    _mix_table_check('mix_write_table', table, n)
    host = None
    if (ranks is None) != (ranks_host is None):
        raise ValueError('mix_write_table: give ranks and ranks_host together, or neither')
    if ranks is not None:
        import numpy as np
        host = np.ascontiguousarray(ranks_host, dtype=np.uint8)
        if ranks.dtype != torch.uint8 or tuple(ranks.shape) != (n, class_num) or not ranks.is_contiguous() \
                or host.shape != (n, class_num):
            raise ValueError('mix_write_table: ranks and ranks_host must be contiguous uint8 (%d, %d)' % (n, class_num))
    y0, y1, x0, x1 = (int(v) for v in box)
    lib().call('rgda_mix_write_table', table.data_ptr(), _p(ranks) or None, host.ctypes.data if host is not None else None,
               n, int(class_num), int(class_bits), y0, y1, x0, x1, _stream())
    return table


# ----------------------------------------------------------------------------- strong augmentation of the student's tile
STRONG_TABLE_COLS = 8           # RGDA_STRONG_TABLE_COLS: {fb, fc, fs, theta, sigma, flags, 0, 0} per image
STRONG_MAX_RADIUS = 12          # RGDA_STRONG_MAX_RADIUS: sigma <= 4


def _strong_table_check(who, table, n):
    if table.dtype != torch.float32 or tuple(table.shape) != (n, STRONG_TABLE_COLS) or not table.is_contiguous():
        raise ValueError('%s: table must be contiguous torch.float32 (%d, %d), got %s %s'
                         % (who, n, STRONG_TABLE_COLS, table.dtype, tuple(table.shape)))


def strong_write_table(table, host, size):
    """rgda_strong_write_table: table (f32 (N, 8) on the device, N <= 16) <- host (a float32 numpy array of that shape:
    fb, fc, fs, theta, sigma, flags, 0, 0 per image -- StrongAugment.draw), carried in the launch's arguments: the host
    buffer is read before this returns.  size = (H, W) of the tiles the table is for.  A row the transform does not serve
    (sigma outside (0, 4] with the blur bit, a radius that does not fit the tile, values that are not finite) is a
    ValueError before any launch."""
    import numpy as np
    _need_cuda(table)
    n = table.shape[0]
    _strong_table_check('strong_write_table', table, n)
    host = np.ascontiguousarray(host, dtype=np.float32)
    if host.shape != (n, STRONG_TABLE_COLS):
        raise ValueError('strong_write_table: host must be float32 (%d, %d), got %s' % (n, STRONG_TABLE_COLS, host.shape))
    h, w = (int(v) for v in size)
    lib().call('rgda_strong_write_table', table.data_ptr(), host.ctypes.data, n, h, w, _stream())
    return table


def strong_augment(images, table, mean, std, out=None, ws=None, flag=None):
    """rgda_strong_augment: colour jitter and Gaussian blur of normalised tiles, image n as row n of `table` (f32 (N, 8)
    on the device) says; include/rgda_hip.h carries the semantics.  images f32 (N,3,H,W), never written; out: the
    result (allocated unless given), a different buffer -- the blur reads neighbours, so in place is refused.  mean, std:
    three values each, the normalisation the tiles carry.  ws: workspace of rgda_strong_augment_workspace(N) bytes, a
    uint8 tensor (allocated unless given; the call rewrites it: each image's constants and its grey sum).  flag: optional device int32, set to 1 by a row whose blur is outside the served range (that image
    is copied).  -> out."""
    _need_cuda(images, table, out, ws, flag)
    if images.dim() != 4 or images.shape[1] != 3 or images.dtype != torch.float32:
        raise ValueError('strong_augment: images must be torch.float32 (N,3,H,W), got %s %s'
                         % (images.dtype, tuple(images.shape)))
    n, _, h, w = images.shape
    _strong_table_check('strong_augment', table, n)
    mean, std = tuple(float(v) for v in mean), tuple(float(v) for v in std)
    if len(mean) != 3 or len(std) != 3 or not all(v > 0 for v in std):
        raise ValueError('strong_augment: mean and std are three values each, std positive')
    if out is None:
        out = torch.empty(images.shape, dtype=torch.float32, device=images.device)
    if out.dtype != torch.float32 or tuple(out.shape) != tuple(images.shape) or not out.is_contiguous():
        raise ValueError('strong_augment: out is written and must be contiguous torch.float32 %s' % (tuple(images.shape),))
    need = lib().size('rgda_strong_augment_workspace', n)
    if ws is None:
        ws = _ws(need, images.device)
    if ws.dtype != torch.uint8 or ws.numel() < need or not ws.is_contiguous():
        raise ValueError('strong_augment: ws must be contiguous torch.uint8 with at least %d bytes' % need)
    if n * h * w == 0:
        return out
    src = images.contiguous()
    if src.data_ptr() == out.data_ptr():
        raise ValueError('strong_augment: out must not be the input (the blur reads neighbouring pixels)')
    lib().call('rgda_strong_augment', src.data_ptr(), out.data_ptr(), table.data_ptr(), ws.data_ptr(), n, h, w, *mean, *std,
               _p(flag) or None, _stream())
    return out


# ----------------------------------------------------------------------------- Fourier style transfer of the source tile
STYLE_TABLE_COLS = 4            # RGDA_STYLE_TABLE_COLS: {partner, b, on, 0} per source image
STYLE_MAX_B = 64                # RGDA_STYLE_MAX_B
STYLE_MAX_IMAGES = 16           # RGDA_STYLE_MAX_IMAGES


def _style_table_check(who, table, n):
    if table.dtype != torch.int32 or tuple(table.shape) != (n, STYLE_TABLE_COLS) or not table.is_contiguous():
        raise ValueError('%s: table must be contiguous torch.int32 (%d, %d), got %s %s'
                         % (who, n, STYLE_TABLE_COLS, table.dtype, tuple(table.shape)))


def fourier_style_write_table(table, host, n_targets, size):
    """rgda_fourier_style_write_table: table (int32 (N, 4) on the device, N <= 16) <- host (an int32 numpy array of that
    shape: partner, b, on, 0 per source image -- FourierStyle.draw), carried in the launch's arguments: the host buffer is
    read before this returns.  n_targets: the target images the partners index; size = (H, W) of the tiles.  A row the
    transform does not serve (a partner outside [0, n_targets), b above 64 or 2 b + 1 above min(H, W), on not 0 or 1) is a
    ValueError before any launch."""
    import numpy as np
    _need_cuda(table)
    n = table.shape[0]
    _style_table_check('fourier_style_write_table', table, n)
    host = np.ascontiguousarray(host, dtype=np.int32)
    if host.shape != (n, STYLE_TABLE_COLS):
        raise ValueError('fourier_style_write_table: host must be int32 (%d, %d), got %s' % (n, STYLE_TABLE_COLS, host.shape))
    h, w = (int(v) for v in size)
    lib().call('rgda_fourier_style_write_table', table.data_ptr(), host.ctypes.data, n, int(n_targets), h, w, _stream())
    return table


def fourier_style_workspace(n, m, h, w, device):
    """A workspace for ops.fourier_style(ws=) at n source and m target tiles of h x w: a uint8 tensor of
    rgda_fourier_style_workspace(n, m, h, w) bytes; ValueError for a shape that is not served."""
    need = lib().size('rgda_fourier_style_workspace', int(n), int(m), int(h), int(w))
    if need == 0:
        raise ValueError('fourier_style: %d + %d tiles of %d x %d are not served (1..%d images of each, H, W <= 4096)'
                         % (n, m, h, w, STYLE_MAX_IMAGES))
    return _ws(need, device)


def fourier_style(images_s, images_t, table, mean_s, std_s, mean_t, std_t, out=None, ws=None, flag=None):
    """rgda_fourier_style: Fourier Domain Adaptation of normalised source tiles -- the amplitudes of the (2 b + 1)^2 lowest
    frequencies of source image n are replaced with those of its partner target image, as row n of `table` (int32 (N, 4)
    on the device: partner, b, on, 0) says; include/rgda_hip.h carries the semantics.  images_s f32 (N,3,H,W) and
    images_t f32 (M,3,H,W), N, M <= 16, never written; out: the result (allocated unless given), a different buffer.
    mean_*, std_*: three values each, the normalisation the source and the target tiles carry.  ws: workspace of
    rgda_fourier_style_workspace(N, M, H, W) bytes, a uint8 tensor (allocated unless given; the call rewrites it).  flag:
    optional device int32, set to 1 by a row that is not served (that image is copied).  -> out."""
    _need_cuda(images_s, images_t, table, out, ws, flag)
    for name, x in (('images_s', images_s), ('images_t', images_t)):
        if x.dim() != 4 or x.shape[1] != 3 or x.dtype != torch.float32:
            raise ValueError('fourier_style: %s must be torch.float32 (N,3,H,W), got %s %s' % (name, x.dtype, tuple(x.shape)))
    n, _, h, w = images_s.shape
    m = images_t.shape[0]
    if tuple(images_t.shape[-2:]) != (h, w):
        raise ValueError('fourier_style: source and target tiles must have one size, got %s and %s'
                         % (tuple(images_s.shape[-2:]), tuple(images_t.shape[-2:])))
    if not 1 <= n <= STYLE_MAX_IMAGES or not 1 <= m <= STYLE_MAX_IMAGES:
        raise ValueError('fourier_style: %d source and %d target images; the kernels serve 1..%d of each'
                         % (n, m, STYLE_MAX_IMAGES))
    _style_table_check('fourier_style', table, n)
    norms = [tuple(float(v) for v in t) for t in (mean_s, std_s, mean_t, std_t)]
    if any(len(t) != 3 for t in norms) or not all(v > 0 for v in norms[1] + norms[3]):
        raise ValueError('fourier_style: mean and std are three values each, std positive')
    if out is None:
        out = torch.empty(images_s.shape, dtype=torch.float32, device=images_s.device)
    if out.dtype != torch.float32 or tuple(out.shape) != tuple(images_s.shape) or not out.is_contiguous():
        raise ValueError('fourier_style: out is written and must be contiguous torch.float32 %s' % (tuple(images_s.shape),))
    if h * w == 0:
        return out
    need = lib().size('rgda_fourier_style_workspace', n, m, h, w)
    if need == 0:
        raise ValueError('fourier_style: %d x %d tiles are not served (H, W <= 4096)' % (h, w))
    if ws is None:
        ws = _ws(need, images_s.device)
    if ws.dtype != torch.uint8 or ws.numel() < need or not ws.is_contiguous():
        raise ValueError('fourier_style: ws must be contiguous torch.uint8 with at least %d bytes' % need)
    src, tgt = images_s.contiguous(), images_t.contiguous()
    if out.data_ptr() in (src.data_ptr(), tgt.data_ptr()):
        raise ValueError('fourier_style: out must not be an input (the transform is out of place)')
    lib().call('rgda_fourier_style', src.data_ptr(), tgt.data_ptr(), out.data_ptr(), table.data_ptr(), ws.data_ptr(), n, m, h, w,
               *norms[0], *norms[1], *norms[2], *norms[3], _p(flag) or None, _stream())
    return out


# ----------------------------------------------------------------------------- region maps without SAM
def superpixels_max_regions(h, w, min_area):
    """The exclusive bound on the region ids rgda_superpixels writes for an h x w image: R <= h * w // min_area, so
    ids lie in [0, that + 1) -- the `max_regions` a Homogenizer / SSLStep is given."""
    return int(h) * int(w) // int(min_area) + 1


def superpixels(img, region_size=16, compactness=10, iters=10, min_area=None, out=None, ws=None):
    """rgda_superpixels: img uint8 [N][H][W][3] on the GPU -> (regs int32 [N][H][W], count int32 [N]).  The integer SLIC
    of include/rgda_hip.h (this library's own specification: it stands in for the reference's third-party LSC / SLIC
    generators and reproduces neither), 4-connected components, components below `min_area` (default S * S // 4)
    dropped to region 0, the others numbered 1..count.  out: (regs, count) tensors to write into; ws: a workspace of
    at least rgda_superpixels_workspace bytes to reuse.  No host synchronisation."""
    _need_cuda(img)
    if img.dim() != 4 or img.shape[3] != 3 or img.dtype != torch.uint8:
        raise ValueError('superpixels: img must be uint8 [N][H][W][3], got %s %s' % (img.dtype, tuple(img.shape)))
    n, h, w, _ = img.shape
    s = int(region_size)
    min_area = s * s // 4 if min_area is None else int(min_area)
    img = img.contiguous()
    if img.data_ptr() % 4:
        img = img.clone()
    L = lib()
    need = L.size('rgda_superpixels_workspace', n, h, w, s)
    if need == 0:
        raise ValueError(f'superpixels: {n} x {h} x {w} tiles at region_size {s} are not served: 4 <= region_size <= 64, '
                         f'H and W multiples of it and at most 16384, N <= 65535')
    if ws is None or ws.numel() < need or ws.data_ptr() % 16:
        ws = _ws(need, img.device)
    regs, count = out if out is not None else (None, None)
    if regs is None:
        regs = torch.empty((n, h, w), dtype=torch.int32, device=img.device)
    if count is None:
        count = torch.empty((n,), dtype=torch.int32, device=img.device)
    assert tuple(regs.shape) == (n, h, w) and regs.dtype == torch.int32 and regs.is_contiguous()
    assert tuple(count.shape) == (n,) and count.dtype == torch.int32 and count.is_contiguous()
    L.call('rgda_superpixels', img.data_ptr(), n, h, w, s, int(compactness), int(iters), min_area, regs.data_ptr(),
           count.data_ptr(), ws.data_ptr(), ws.numel(), _stream())
    return regs, count


def region_shrink(regs, win=3, fill=0):
    """rgda_region_shrink (the reference's edge_shrinking, superpixels.py:129-152, bit-exact): regs int32 [N][H][W] or
    [H][W] -> a new map that keeps an id where the (2 * win + 1)^2 window inside the image holds only that id and is
    `fill` elsewhere."""
    _need_cuda(regs)
    if regs.dtype != torch.int32 or regs.dim() not in (2, 3):
        raise ValueError('region_shrink: regs must be int32 [N][H][W] or [H][W], got %s %s' % (regs.dtype, tuple(regs.shape)))
    src = regs.contiguous()
    out = torch.empty_like(src)
    n, h, w = (1,) + tuple(src.shape) if src.dim() == 2 else tuple(src.shape)
    lib().call('rgda_region_shrink', src.data_ptr(), n, h, w, int(win), int(fill), out.data_ptr(), _stream())
    return out


# ----------------------------------------------------------------------------- evaluation path
def argmax_nchw(probs):
    n, c, h, w = probs.shape
    out = torch.empty(n, h, w, dtype=torch.int64, device=probs.device)
    lib().call('rgda_argmax_nchw', probs.contiguous().float().data_ptr(), out.data_ptr(), n, c, h * w, _stream())
    return out


def confusion_accumulate(y_true, y_pred, cm, flag):
    """cm int64 [C, C] += counts over the pixels with y_true >= 0 (row = true class)."""
    assert cm.dtype == torch.int64 and cm.is_contiguous() and cm.shape[0] == cm.shape[1]
    yt, yp = y_true.contiguous().view(-1), y_pred.contiguous().view(-1)
    assert yt.dtype == yp.dtype == torch.int64 and yt.numel() == yp.numel()
    lib().call('rgda_confusion_accumulate', yt.data_ptr(), yp.data_ptr(), cm.data_ptr(), flag.data_ptr(), yt.numel(),
               cm.shape[0], _stream())


# ----------------------------------------------------------------------------- stage 2 ("align")
def pcl_flag(ws, class_num, k):
    """The int32 flag word of a workspace that rgda_pcl_loss has used (one host sync): bit 2 (value 4) a label outside
    [0, class_num) that is not ignore_label, bit 3 (value 8) a kept pixel whose loss is not finite (the loss reads NaN)."""
    off = (int(class_num) * int(k) * 4 + 255) // 256 * 256 + 4
    return int(ws[off:off + 4].view(torch.int32).item())


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
    if ws is None:
        ws = _ws(L.size('rgda_pcl_loss_workspace', C, K), feat.device)
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


MMD_KERNEL_TYPES = {'rbf': 0, 'linear': 1}      # RGDA_MMD_RBF, RGDA_MMD_LINEAR


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


DCA_PRED_KINDS = {'prob': 0, 'logits': 1, 'logits2': 2}      # pred_kind of rgda_dca_context / rgda_dca_loss
DCA_KINDS = {'cov': 0, 'mse': 1}


def _dca_side(feat, preds, pred_kind, who):
    """one side of the DCA entry points -> (f32 feature tensor, b, hw, ldc, ldb, c, C, the prediction planes kept alive)"""
    assert feat.dim() == 4, f'{who}: NCHW (b, c, h, w) features'
    feat, b, hw, ldc, ldb, c = _feat_rows(feat, who)
    preds = tuple(preds) if isinstance(preds, (tuple, list)) else (preds,)
    if len(preds) != (2 if pred_kind == 'logits2' else 1):
        raise ValueError(f'{who}: pred_kind {pred_kind!r} takes {2 if pred_kind == "logits2" else 1} prediction map(s)')
    preds = tuple(p.detach().float().contiguous() for p in preds)
    C = preds[0].shape[1]
    for p in preds:
        assert p.dim() == 4 and p.shape[0] == b and p.shape[1] == C and p.shape[2] * p.shape[3] == hw, (p.shape, feat.shape)
    _need_cuda(feat, *preds)
    return feat, b, hw, ldc, ldb, c, C, preds


def _dca_kind(pred_kind, who):
    if pred_kind not in DCA_PRED_KINDS:
        raise ValueError(f'{who}: pred_kind {pred_kind!r}; served are {sorted(DCA_PRED_KINDS)}')
    return DCA_PRED_KINDS[pred_kind]


def dca_context(feat, preds, pred_kind='prob', ignore_bg=False, return_all=False):
    """CategoryAlign_Module.get_context (regda/dca_modules.py:20-34) on rgda_dca_context: feat f32 (b, c, h, w), read in
    place through its channel and image strides; preds f32 (b, C, h, w): probabilities ('prob'), logits whose softmax is
    taken ('logits') or a pair of logit maps whose softmaxes are averaged ('logits2').  -> u f32 (b, n, c), the class
    contexts normalised over the CLASS axis (n = C - 1 with ignore_bg); with return_all (u, v, Z): the contexts before
    the normalisation (b, n, c) and the class masses (b, C)."""
    pk = _dca_kind(pred_kind, 'dca_context')
    feat, b, hw, ldc, ldb, c, C, preds = _dca_side(feat, preds, pred_kind, 'dca_context')
    n = C - 1 if ignore_bg else C
    u = torch.empty(b, n, c, device=feat.device)
    v = torch.empty(b, n, c, device=feat.device) if return_all else None
    Z = torch.empty(b, C, device=feat.device) if return_all else None
    L = lib()
    ws = _ws(L.size('rgda_dca_context_workspace', b, c), feat.device)
    L.call('rgda_dca_context', feat.data_ptr(), b, hw, ldc, ldb, preds[0].data_ptr(), _p(preds[1] if pk == 2 else None), pk,
           c, C, int(bool(ignore_bg)), u.data_ptr(), _p(v), _p(Z), ws.data_ptr(), ws.numel(), _stream())
    return (u, v, Z) if return_all else u


def dca_loss(feat_a, preds_a, feat_b, preds_b, pred_kind='logits2', kind='cov', ignore_bg=True, weight=1.0, loss=None,
             dfeat_a=None, dfeat_b=None, accumulate=False, return_ws=False):
    """The category alignment losses of regda/dca_modules.py on rgda_dca_loss: kind 'cov' is
    regularize(get_cross_corcoef_mat(side a, side b)) (CCR: a = source, b = target; ICR: the two halves of one batch),
    kind 'mse' is F.mse_loss(get_context(a), get_context(b)) (MSE_cross / MSE_intra; equal image counts).  feat_* f32
    (b, c, h, w), read in place (batch and channel slices included); preds_* as in dca_context, always constants.
    loss (f32[1]) += weight * L; dfeat_a / dfeat_b (optional) bf16 [b*h*w, >= c] pixel-major rows: (+)= weight * dL / dfeat
    of that side; a side without rows gets no gradient launch.  Returns the (accumulating) fp32 loss tensor (and the
    workspace with return_ws: the layout of include/rgda_hip.h)."""
    pk = _dca_kind(pred_kind, 'dca_loss')
    if kind not in DCA_KINDS:
        raise ValueError(f"dca_loss: kind {kind!r}; served are 'cov' and 'mse'")
    fa, ba, hw, lca, lba, c, C, pa = _dca_side(feat_a, preds_a, pred_kind, 'dca_loss')
    fb, bb, hwb, lcb, lbb, cb, Cb, pb = _dca_side(feat_b, preds_b, pred_kind, 'dca_loss')
    if (hw, c, C) != (hwb, cb, Cb):
        raise ValueError(f'dca_loss: the sides differ in (pixels, channels, classes): {(hw, c, C)} vs {(hwb, cb, Cb)}')
    _need_cuda(dfeat_a, dfeat_b)
    (ga, lda), (gb, ldb_) = _grad_rows(dfeat_a, ba * hw), _grad_rows(dfeat_b, bb * hw)
    if ga and gb and lda != ldb_:
        raise ValueError('dca_loss: the two gradient buffers share one leading dimension')
    loss = _loss_out(loss, fa.device)
    L = lib()
    ws = _ws(L.size('rgda_dca_loss_workspace', ba, bb, c, C, int(bool(ignore_bg))), fa.device)
    L.call('rgda_dca_loss', fa.data_ptr(), ba, lca, lba, pa[0].data_ptr(), _p(pa[1] if pk == 2 else None), ga,
           fb.data_ptr(), bb, lcb, lbb, pb[0].data_ptr(), _p(pb[1] if pk == 2 else None), gb, hw, c, C, pk,
           int(bool(ignore_bg)), DCA_KINDS[kind], loss.data_ptr(), lda or ldb_, int(bool(accumulate)), float(weight),
           ws.data_ptr(), ws.numel(), _stream())
    return (loss, ws) if return_ws else loss


SAW_CLASS_COUNTS = (2, 4, 6, 8, 16)      # len(selected_classes) rgda_saw_loss serves (the reference asserts the same set)
SAW_MAX_CHANNELS = 4096


def saw_margin(C, relax_denom):
    """SAW.__init__'s margin (regda/gast/SAW.py:33-37): 0 for relax_denom == 0, else nod // relax_denom (floor division)"""
    nod = float(C * (C - 1) // 2)
    return 0.0 if relax_denom == 0 else float(nod // relax_denom)


def saw_loss(feat, cls_w, selected_classes, relax_denom=2.0, weight=1.0, loss=None, dfeat=None, accumulate=False,
             check=False, return_ws=False):
    """SAW(classifier, selected_classes, relax_denom)(feat) (regda/gast/SAW.py) on rgda_saw_loss: feat f32 (b, k, h, w),
    read in place through its channel and image strides when the pixels of an image are contiguous, copied otherwise;
    cls_w f32 (n_cls, k) on the device, the classifier weight (a constant: it receives no gradient; its channels are
    ranked on the device, so a weight that changes every step costs no host sync); selected_classes: 2, 4, 6, 8 or 16
    distinct rows of cls_w.  Equal |w| rank by the lower channel index.  loss (f32[1]) += weight * L; dfeat (optional)
    bf16 [b*h*w, >= k] pixel-major rows: (+)= weight * dL / dfeat (accumulate=False writes every row; channels that take
    no part as zeros).  check=True reads the flag word back (one host sync) and raises ValueError on a non-finite weight.
    Returns the (accumulating) fp32 loss tensor (and the workspace with return_ws; saw_tables reads it)."""
    import ctypes
    _need_cuda(feat, cls_w, dfeat)
    assert feat.dim() == 4, 'saw_loss: NCHW (b, k, h, w) features'
    feat, b, hw, ldc, ldb, k = _feat_rows(feat, 'saw_loss')
    sel = [int(c) for c in selected_classes]
    C = len(sel)
    if C not in SAW_CLASS_COUNTS:
        raise ValueError(f'saw_loss: {C} selected classes; served are {SAW_CLASS_COUNTS}')
    cls_w = cls_w.detach()
    assert cls_w.dim() == 2 and cls_w.shape[1] == k, (cls_w.shape, k)
    if cls_w.dtype != torch.float32 or cls_w.stride(1) != 1:
        cls_w = cls_w.float().contiguous()
    sel_host = (ctypes.c_int32 * C)(*sel)
    loss = _loss_out(loss, feat.device)
    L = lib()
    ws = _ws(L.size('rgda_saw_loss_workspace', b, hw, k, C), feat.device)
    L.call('rgda_saw_loss', feat.data_ptr(), b, hw, ldc, ldb, k, cls_w.data_ptr(), cls_w.shape[0], cls_w.stride(0),
           sel_host, C, saw_margin(C, relax_denom), loss.data_ptr(), *_grad_rows(dfeat, b * hw), int(bool(accumulate)),
           float(weight), ws.data_ptr(), ws.numel(), _stream())
    if check and int(ws[:4].view(torch.int32).item()) & 1:
        raise ValueError('saw_loss: a classifier weight is not finite')
    return (loss, ws) if return_ws else loss


def saw_tables(ws, b, k, C):
    """What rgda_saw_loss left in its workspace (the layout of include/rgda_hip.h), for diagnostics and tests -> dict:
    flag (int), ch int32 [G, C] and wgh f32 [G, C] (the slot tables), inv int32 [k, C] (the rank of the slot a channel
    fills for a class, -1: none), active bool [b, G], signs int8 [b, G, nod] (pairs (j, j'), j < j', row-major),
    s f32 [b, G]."""
    a = lambda x: (x + 255) // 256 * 256      # noqa: E731
    G, nod = k // C, C * (C - 1) // 2
    TS = (nod + 1 + 3) // 4 * 4
    o = 256
    tab = ws[o:o + b * G * TS].view(torch.int8).view(b, G, TS)
    o += a(b * G * TS)
    s = ws[o:o + 4 * b * G].view(torch.float32).view(b, G)
    o += 2 * a(4 * b * G)
    ch = ws[o:o + 4 * G * C].view(torch.int32).view(G, C)
    o += a(4 * G * C)
    wgh = ws[o:o + 4 * G * C].view(torch.float32).view(G, C)
    o += a(4 * G * C)
    inv = ws[o:o + 4 * k * C].view(torch.int32).view(k, C)
    return dict(flag=int(ws[:4].view(torch.int32).item()), ch=ch, wgh=wgh, inv=inv, active=tab[:, :, 0] != 0,
                signs=tab[:, :, 1:1 + nod], s=s)


# ---------------------------------------------------------------- TransNorm (regda/trans_norm.py)
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


# ---------------------------------------------------------------- ASPP head (Classifier_Module)
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


# ---------------------------------------------------------------- output-space adversarial alignment (adv_kernels.hip)
ADV_CP = 16         # channels of a probability row: the classes zero-padded to one K slice of the bf16 MFMA
DISC_SLOPE = 0.2    # nn.LeakyReLU(negative_slope=0.2), regda/models/Discriminator.py:15


def _rows_bf16(t, cols, who):
    assert t.dtype == torch.bfloat16 and t.dim() == 2 and t.shape[1] == cols and t.is_contiguous(), (who, t.shape, t.dtype)
    return t


def adv_probs(x, size=None, softmax=True, out=None):
    """x f32 (b, C, h, w) on the GPU -> P bf16 [b*H*W, 16]: softmax over the classes of the bilinear (align_corners=True)
    upsample to size = (H, W), or with softmax=False the given probabilities packed as they are (size is x's own)."""
    _need_cuda(x, out)
    assert x.dim() == 4 and x.dtype == torch.float32 and x.is_contiguous(), 'adv_probs: contiguous f32 (b, C, h, w)'
    b, C, h, w = x.shape
    check_class_count(C, 'adv_probs')
    H, W = (h, w) if size is None else (int(size[0]), int(size[1]))
    if not softmax and (H, W) != (h, w):
        raise ValueError('adv_probs: given probabilities are packed at their own size')
    P = out if out is not None else torch.empty((b * H * W, ADV_CP), dtype=torch.bfloat16, device=x.device)
    _rows_bf16(P, ADV_CP, 'adv_probs')
    assert P.shape[0] == b * H * W
    lib().call('rgda_adv_probs_fwd', x.data_ptr(), P.data_ptr(), b, C, h, w, H, W, ADV_CP, 0 if softmax else 1, _stream())
    return P


def adv_probs_backward(dP, x, dx, size=None, softmax=True, scale=1.0):
    """dx f32 (b, C, h, w) += scale * (adv_probs' gradient of dP bf16 [b*H*W, 16]); x: the forward's input."""
    _need_cuda(dP, x, dx)
    assert dx.dim() == 4 and dx.dtype == torch.float32 and dx.is_contiguous() and x.shape == dx.shape
    assert x.dtype == torch.float32 and x.is_contiguous()
    b, C, h, w = dx.shape
    check_class_count(C, 'adv_probs_backward')
    H, W = (h, w) if size is None else (int(size[0]), int(size[1]))
    _rows_bf16(dP, ADV_CP, 'adv_probs_backward')
    assert dP.shape[0] == b * H * W
    lib().call('rgda_adv_probs_bwd', dP.data_ptr(), x.data_ptr(), dx.data_ptr(), b, C, h, w, H, W, ADV_CP,
               0 if softmax else 1, float(scale), _stream())
    return dx


def disc_conv(x, w, bias, N, H, W, slope=DISC_SLOPE, out=None):
    """One discriminator layer: x bf16 [N*H*W, Cin], w bf16 [Cout, 16, Cin], bias f32 [Cout] or None ->
    lrelu(conv 4x4 / stride 2 / pad 1 + bias) as bf16 [N*(H/2)*(W/2), Cout]."""
    _need_cuda(x, w, bias, out)
    Cout, taps, Cin = w.shape
    assert taps == 16 and w.dtype == torch.bfloat16 and w.is_contiguous()
    _rows_bf16(x, Cin, 'disc_conv')
    assert x.shape[0] == N * H * W and (bias is None or (bias.dtype == torch.float32 and bias.numel() == Cout and bias.is_contiguous()))
    y = out if out is not None else torch.empty((N * (H // 2) * (W // 2), Cout), dtype=torch.bfloat16, device=x.device)
    _rows_bf16(y, Cout, 'disc_conv')
    lib().call('rgda_disc_conv_fwd', x.data_ptr(), w.data_ptr(), _p(bias), y.data_ptr(), N, H, W, Cin, Cout, float(slope), _stream())
    return y


def disc_bias_lrelu(y, bias, slope=DISC_SLOPE):
    """y bf16 [M, C] = lrelu(y + bias) in place (the epilogue pass behind the generic convolution)."""
    _need_cuda(y, bias)
    M, C = y.shape
    _rows_bf16(y, C, 'disc_bias_lrelu')
    assert bias.dtype == torch.float32 and bias.numel() == C and bias.is_contiguous()
    lib().call('rgda_disc_bias_lrelu', y.data_ptr(), bias.data_ptr(), M, C, float(slope), _stream())
    return y


def disc_bias_grad(g):
    """g bf16 [M, C] -> f32 [C] column sums in a fixed order."""
    _need_cuda(g)
    M, C = g.shape
    _rows_bf16(g, C, 'disc_bias_grad')
    db = torch.empty(C, dtype=torch.float32, device=g.device)
    L = lib()
    ws = _ws(L.size('rgda_disc_bias_grad_workspace', M, C), g.device)
    L.call('rgda_disc_bias_grad', g.data_ptr(), M, C, db.data_ptr(), ws.data_ptr(), ws.numel(), _stream())
    return db


def disc_conv_backward(g, x, wt, N, H, W, below=True, need_dx=True, need_dparams=True, slope=DISC_SLOPE):
    """The gradients of disc_conv from g bf16 [N*(H/2)*(W/2), Cout], the gradient of the layer's PRE-activation.
    x bf16 [N*H*W, Cin]: the layer's input; wt bf16 [Cin, 16, Cout]: the transposed operand copy.
    -> (dx, dw, db): dx bf16 [N*H*W, Cin] masked by x's sign where `below` (x is a stored LeakyReLU output) -- the
    pre-activation gradient of the layer underneath; dw f32 [Cout, 16, Cin] (rgda_conv2d_wgrad_grouped) and db f32 [Cout]."""
    _need_cuda(g, x, wt)
    Cin, taps, Cout = wt.shape
    assert taps == 16 and wt.dtype == torch.bfloat16 and wt.is_contiguous()
    _rows_bf16(x, Cin, 'disc_conv_backward')
    _rows_bf16(g, Cout, 'disc_conv_backward')
    assert x.shape[0] == N * H * W and g.shape[0] == N * (H // 2) * (W // 2)
    dx = dw = db = None
    if need_dparams:
        dw = torch.zeros((Cout, 16, Cin), dtype=torch.float32, device=g.device)
        conv2d_wgrad_grouped([(x, g, dw, N, H, W, H // 2, W // 2, 4, 4, 2, 1, 1)])
        db = disc_bias_grad(g)
    if need_dx:
        dx = torch.empty_like(x)
        lib().call('rgda_disc_conv_bwd_data', g.data_ptr(), wt.data_ptr(), x.data_ptr() if below else 0, dx.data_ptr(), N, H, W,
                   Cin, Cout, float(slope), _stream())
    return dx, dw, db


def disc_head(a4, w, bias, N, H, W):
    """The classifier: a4 bf16 [N*H*W, C], w f32 [16, C], bias f32 [1] -> z f32 [N, (H/2)*(W/2)]."""
    _need_cuda(a4, w, bias)
    C = w.shape[1]
    assert w.shape == (16, C) and w.dtype == torch.float32 and w.is_contiguous()
    _rows_bf16(a4, C, 'disc_head')
    assert a4.shape[0] == N * H * W
    z = torch.empty((N, (H // 2) * (W // 2)), dtype=torch.float32, device=a4.device)
    lib().call('rgda_disc_head_fwd', a4.data_ptr(), w.data_ptr(), _p(bias), z.data_ptr(), N, H, W, C, _stream())
    return z


def disc_head_backward(dz, a4, w, N, H, W, need_da=True, need_dparams=True, slope=DISC_SLOPE):
    """-> (da4 bf16 [N*H*W, C] masked by a4's sign, dw f32 [16, C], db f32 [1]) from dz f32 [N, (H/2)*(W/2)]."""
    _need_cuda(dz, a4, w)
    C = w.shape[1]
    _rows_bf16(a4, C, 'disc_head_backward')
    assert dz.dtype == torch.float32 and dz.is_contiguous() and dz.numel() == N * (H // 2) * (W // 2)
    da = torch.empty_like(a4) if need_da else None
    dw = torch.empty((16, C), dtype=torch.float32, device=a4.device) if need_dparams else None
    db = torch.empty(1, dtype=torch.float32, device=a4.device) if need_dparams else None
    lib().call('rgda_disc_head_bwd', dz.data_ptr(), a4.data_ptr(), w.data_ptr(), _p(da), _p(dw), _p(db), N, H, W, C,
               float(slope), _stream())
    return da, dw, db


def bce_logits(z, label, scale=1.0, loss=None, accumulate=False, want_grad=True):
    """scale * F.binary_cross_entropy_with_logits(z, full_like(z, label)) for label 0 or 1 -> (loss f32 [1] on the
    device, dz f32 of z's shape or None).  accumulate: added onto `loss`."""
    _need_cuda(z, loss)
    assert z.dtype == torch.float32 and z.is_contiguous()
    if float(label) not in (0.0, 1.0):
        raise ValueError('bce_logits: the label is 0 or 1, got %r' % (label,))
    if loss is None:
        assert not accumulate
        loss = torch.empty(1, dtype=torch.float32, device=z.device)
    dz = torch.empty_like(z) if want_grad else None
    lib().call('rgda_bce_logits', z.data_ptr(), z.numel(), float(label), float(scale), loss.data_ptr(), int(bool(accumulate)),
               _p(dz), _stream())
    return loss, dz


# ---------------------------------------------------------------- category-level adversarial alignment (clan_kernels.hip)
def _pair_logits(x1, x2, who):
    _need_cuda(x1, x2)
    assert x1.dim() == 4 and x1.dtype == torch.float32 and x1.is_contiguous(), who + ': contiguous f32 (b, C, h, w)'
    assert x2.shape == x1.shape and x2.dtype == torch.float32 and x2.is_contiguous(), who + ': x2 as x1'
    check_class_count(x1.shape[1], who)
    return x1.shape


def clan_probs(x1, x2, size=None):
    """The two heads' logits x1, x2 f32 (b, C, h, w) -> (P bf16 [b*H*W, 16] = softmax(up x1 + up x2), what the
    discriminator reads, and wmap f32 (b, H, W) = 1 - cos(softmax(up x1), softmax(up x2))); `up`: bilinear,
    align_corners=True, to size = (H, W)."""
    b, C, h, w = _pair_logits(x1, x2, 'clan_probs')
    H, W = (h, w) if size is None else (int(size[0]), int(size[1]))
    P = torch.empty((b * H * W, ADV_CP), dtype=torch.bfloat16, device=x1.device)
    wmap = torch.empty((b, H, W), dtype=torch.float32, device=x1.device)
    lib().call('rgda_clan_probs_fwd', x1.data_ptr(), x2.data_ptr(), P.data_ptr(), wmap.data_ptr(), b, C, h, w, H, W, ADV_CP,
               _stream())
    return P, wmap


def clan_probs_backward(dP, gw, x1, x2, dx1, dx2, size=None, scale=1.0):
    """dx1, dx2 f32 (b, C, h, w) += scale * (clan_probs' gradient of dP bf16 [b*H*W, 16] and of gw f32 (b, H, W), the
    gradient with respect to wmap; gw None: the weight map is a constant); x1, x2: the forward's inputs."""
    b, C, h, w = _pair_logits(x1, x2, 'clan_probs_backward')
    _need_cuda(dP, gw, dx1, dx2)
    for dx in (dx1, dx2):
        assert dx.shape == x1.shape and dx.dtype == torch.float32 and dx.is_contiguous()
    H, W = (h, w) if size is None else (int(size[0]), int(size[1]))
    _rows_bf16(dP, ADV_CP, 'clan_probs_backward')
    assert dP.shape[0] == b * H * W
    assert gw is None or (gw.dtype == torch.float32 and gw.is_contiguous() and gw.numel() == b * H * W)
    lib().call('rgda_clan_probs_bwd', dP.data_ptr(), _p(gw), x1.data_ptr(), x2.data_ptr(), dx1.data_ptr(), dx2.data_ptr(), b, C,
               h, w, H, W, ADV_CP, float(scale), _stream())
    return dx1, dx2


def wbce_logits(z, size, target, wmap=None, alpha=1.0, beta=0.0, scale=1.0, mean=True, loss=None, accumulate=False,
                want_dz=True, want_gw=False):
    """WeightedBCEWithLogitsLoss (regda/loss.py:60-85) on z f32 (b, hz, wz) upsampled (bilinear, align_corners=True) to
    size = (H, W): scale * mean-or-sum over the pixels of (alpha + beta * wmap) * BCE(up z, target); wmap f32 (b, H, W) or
    None for the plain loss; target a tensor f32 (b, H, W) or the constant label 0 / 1.
    -> (loss f32 [1] on the device, dz f32 of z's shape or None, gw f32 (b, H, W), the gradient for wmap, or None)."""
    _need_cuda(z, wmap, loss)
    assert z.dim() == 3 and z.dtype == torch.float32 and z.is_contiguous(), 'wbce_logits: contiguous f32 (b, hz, wz)'
    b, hz, wz = z.shape
    H, W = int(size[0]), int(size[1])
    label = 0.0
    if isinstance(target, torch.Tensor):
        _need_cuda(target)
        assert target.dtype == torch.float32 and target.is_contiguous() and target.numel() == b * H * W
    else:
        if float(target) not in (0.0, 1.0):
            raise ValueError('wbce_logits: a constant label is 0 or 1, got %r' % (target,))
        label, target = float(target), None
    assert wmap is None or (wmap.dtype == torch.float32 and wmap.is_contiguous() and wmap.numel() == b * H * W)
    if want_gw and wmap is None:
        raise ValueError('wbce_logits: no weight map, no gradient with respect to it')
    if loss is None:
        assert not accumulate
        loss = torch.empty(1, dtype=torch.float32, device=z.device)
    dz = torch.empty_like(z) if want_dz else None
    gw = torch.empty((b, H, W), dtype=torch.float32, device=z.device) if want_gw else None
    L = lib()
    nbytes = L.size('rgda_wbce_logits_workspace', b, H, W)
    if not nbytes:
        raise ValueError(f'wbce_logits: {b} x {H} x {W} pixels are not served')
    ws = _ws(nbytes, z.device)
    L.call('rgda_wbce_logits', z.data_ptr(), b, hz, wz, H, W, _p(target), label, _p(wmap), float(alpha), float(beta),
           float(scale), int(bool(mean)), loss.data_ptr(), int(bool(accumulate)), _p(dz), _p(gw), ws.data_ptr(), ws.numel(),
           _stream())
    return loss, dz, gw


# ---------------------------------------------------------------- feature-space adversarial alignment (fada_kernels.hip)
FADA_CP = 32            # columns of a head row of PixelDiscriminator: 2 * num_classes <= 32
FADA_MAX_CLASSES = 16


def check_fada_classes(nc, who='num_classes'):
    """ValueError unless 1 <= nc <= FADA_MAX_CLASSES (the two heads share one 32-column tile)."""
    if not 1 <= int(nc) <= FADA_MAX_CLASSES:
        raise ValueError(f'{who}: {nc} classes; the head kernel serves 1 <= num_classes <= {FADA_MAX_CLASSES}')


def feat_pack_rows(x, out=None):
    """x f32 (b, k, h, w) on the GPU (read in place through its channel and image strides where the pixels of an image
    are contiguous) -> bf16 rows [b*h*w, ld] with columns 0 .. k-1 written; `out` gives a wider, caller-filled buffer."""
    if x.dim() != 4 or x.dtype != torch.float32:
        raise ValueError(f'feat_pack_rows: f32 (b, k, h, w) features, got {x.dtype} {tuple(x.shape)}')
    _need_cuda(x, out)
    x, b, hw, ldc, ldb, k = _feat_rows(x, 'feat_pack_rows')
    if out is None:
        if k % 8:
            raise ValueError(f'feat_pack_rows: {k} channels; dense rows need k % 8 == 0 (or a wider `out`)')
        out = torch.empty((b * hw, k), dtype=torch.bfloat16, device=x.device)
    _rows_bf16(out, out.shape[1], 'feat_pack_rows')
    assert out.shape[0] == b * hw and out.shape[1] >= k
    lib().call('rgda_feat_pack_rows', x.data_ptr(), b, hw, ldc, ldb, k, out.data_ptr(), out.shape[1], _stream())
    return out


def feat_unpack_rows(rows, dx, scale=1.0, accumulate=False):
    """dx f32 (b, k, h, w) (a strided view as in feat_pack_rows) = (accumulate ? dx : 0) + scale * rows[:, :k]"""
    _need_cuda(rows, dx)
    assert dx.dim() == 4 and dx.dtype == torch.float32
    b, k, h, w = dx.shape
    ldb, ldc = dx.stride(0), dx.stride(1)
    assert (w == 1 or dx.stride(3) == 1) and (h == 1 or dx.stride(2) == w) and ldc >= h * w and (b == 1 or ldb >= ldc * k), \
        'feat_unpack_rows: the pixels of one image must be contiguous'
    _rows_bf16(rows, rows.shape[1], 'feat_unpack_rows')
    assert rows.shape[0] == b * h * w and rows.shape[1] >= k
    lib().call('rgda_feat_unpack_rows', rows.data_ptr(), rows.shape[1], dx.data_ptr(), b, h * w, ldc, ldb, k, float(scale),
               int(bool(accumulate)), _stream())
    return dx


def _fada_head_operands(a2, wh, bias, N, H, W, who):
    _need_cuda(a2, wh, bias)
    rows, taps, Ch = wh.shape
    assert rows == FADA_CP and taps == 9 and wh.dtype == torch.bfloat16 and wh.is_contiguous(), who
    assert bias.dtype == torch.float32 and bias.numel() == FADA_CP and bias.is_contiguous(), who
    _rows_bf16(a2, Ch, who)
    assert a2.shape[0] == N * H * W
    return Ch


def fada_head(a2, wh, bias, N, H, W, nc):
    """The two heads of PixelDiscriminator: a2 bf16 [N*H*W, Ch], wh bf16 [32, 9, Ch], bias f32 [32] -> z f32 [N*H*W, 32]
    (columns 0 .. 2 nc - 1 live)."""
    check_fada_classes(nc, 'fada_head')
    Ch = _fada_head_operands(a2, wh, bias, N, H, W, 'fada_head')
    z = torch.empty((N * H * W, FADA_CP), dtype=torch.float32, device=a2.device)
    lib().call('rgda_fada_head', a2.data_ptr(), wh.data_ptr(), bias.data_ptr(), N, H, W, Ch, int(nc), z.data_ptr(), 0, 0, 1.0,
               1.0, 0.0, 0, 0, 0, 0, _stream())
    return z


def fada_loss(a2, wh, bias, x2, side, temperature=1.8, clip=0.9, scale=1.0, loss=None, want_z=False):
    """The fused head + loss: with z = head(a2), a = min(softmax(x2 / temperature), clip) (x2 f32 (N, nc, H, W) logits, no
    gradient) and M = N*H*W, loss (f32 [1], accumulating) += scale * l(z, a, side) and dz bf16 [M, 32] = scale * dl/dz.
    -> (loss, dz, z or None)."""
    if x2.dim() != 4 or x2.dtype != torch.float32:
        raise ValueError(f'fada_loss: f32 (N, nc, H, W) logits, got {x2.dtype} {tuple(x2.shape)}')
    N, nc, H, W = x2.shape
    check_fada_classes(nc, 'fada_loss')
    if side not in (0, 1):
        raise ValueError(f'fada_loss: side is 0 (source) or 1 (target), got {side!r}')
    if not temperature > 0 or not clip > 0:
        raise ValueError(f'fada_loss: temperature and clip must be positive, got {temperature!r} and {clip!r}')
    _need_cuda(x2, loss)
    Ch = _fada_head_operands(a2, wh, bias, N, H, W, 'fada_loss')
    x2 = x2.contiguous()
    loss = _loss_out(loss, a2.device)
    M = N * H * W
    dz = torch.empty((M, FADA_CP), dtype=torch.bfloat16, device=a2.device)
    z = torch.empty((M, FADA_CP), dtype=torch.float32, device=a2.device) if want_z else None
    L = lib()
    ws = _ws(L.size('rgda_fada_head_workspace', M), a2.device)
    L.call('rgda_fada_head', a2.data_ptr(), wh.data_ptr(), bias.data_ptr(), N, H, W, Ch, nc, _p(z), x2.data_ptr(), int(side),
           float(temperature), float(clip), float(scale), loss.data_ptr(), dz.data_ptr(), ws.data_ptr(), ws.numel(), _stream())
    return loss, dz, z


def fada_head_backward_data(dz, wt, below, N, H, W, slope=DISC_SLOPE):
    """da bf16 [N*H*W, Ch] from dz bf16 [N*H*W, 32] and wt bf16 [Ch, 9, 32], masked by the sign of `below` bf16 [N*H*W, Ch],
    the stored activation."""
    _need_cuda(dz, wt, below)
    Ch, taps, cp = wt.shape
    assert taps == 9 and cp == FADA_CP and wt.dtype == torch.bfloat16 and wt.is_contiguous()
    _rows_bf16(dz, FADA_CP, 'fada_head_backward_data')
    assert dz.shape[0] == N * H * W
    _rows_bf16(below, Ch, 'fada_head_backward_data')
    assert below.shape[0] == N * H * W
    da = torch.empty((N * H * W, Ch), dtype=torch.bfloat16, device=dz.device)
    lib().call('rgda_fada_head_bwd_data', dz.data_ptr(), wt.data_ptr(), below.data_ptr(), da.data_ptr(), N, H, W, Ch, float(slope),
               _stream())
    return da


def lrelu_mask_rows(g, a, slope=DISC_SLOPE):
    """g bf16 [M, C] *= (a > 0 ? 1 : slope) in place (a: the stored activation, same shape)"""
    _need_cuda(g, a)
    M, C = g.shape
    _rows_bf16(g, C, 'lrelu_mask_rows')
    _rows_bf16(a, C, 'lrelu_mask_rows')
    assert a.shape[0] == M
    lib().call('rgda_lrelu_mask_rows', g.data_ptr(), a.data_ptr(), M, C, float(slope), _stream())
    return g
