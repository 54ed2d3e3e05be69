"""The label path: pseudo-label selection, LRH, label refinement, prototypes (csrc/label_kernels.hip), and the region
maps LRH reads where there is no SAM: integer SLIC and region shrinking (the small csrc/superpixel_kernels.hip)."""
import torch

from .._lib import lib
from .base import _need_cuda, _p, _stream, _ws


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
