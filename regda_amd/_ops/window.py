"""The teacher / pseudo-label harness and the evaluation path: TTA views, sliding windows, resizes, argmax and
the confusion matrix (csrc/teacher_kernels.hip), and the batched window gather / scatter / merge
(csrc/window_kernels.hip)."""
import torch

from .._lib import lib
from .base import _need_cuda, _p, _stream


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
    return _window_gather('window_gather', src, windows, tile, views, lut, out, flag)


def _window_gather(who, src, windows, tile, views, lut, out, flag, *scaled_size):
    """The body of window_gather and window_gather_scaled (rgda_<who>); scaled_size: the scaled call's (Hs, Ws), passed
    behind the source's H and W."""
    _need_cuda(src, windows, lut, out, flag)
    th, tw = tile
    if src.dtype == torch.uint8:
        if src.dim() != 4 or src.shape[3] != 3 or lut is None:
            raise ValueError('%s: a uint8 source is [n][H][W][3] and needs lut' % who)
        n, H, W, c = src.shape
        f32, u8 = None, src.contiguous()
    else:
        if src.dtype != torch.float32 or src.dim() != 4:
            raise ValueError('%s: the source is f32 [n][C][H][W] or uint8 [n][H][W][3]' % who)
        n, c, H, W = src.shape
        f32, u8 = src.contiguous(), None
    if windows.dtype != torch.int32 or windows.dim() != 2 or windows.shape[1] != 3 or not windows.is_contiguous():
        raise ValueError('%s: windows must be a contiguous int32 [K][3] table' % who)
    k = windows.shape[0]
    if out is None:
        out = torch.empty(k * views, c, th, tw, device=src.device)
    assert tuple(out.shape) == (k * views, c, th, tw) and out.dtype == torch.float32 and out.is_contiguous()
    lib().call('rgda_' + who, _p(f32), _p(u8), _p(lut), windows.data_ptr(), k, views, n, c, H, W, *scaled_size, th, tw,
               out.data_ptr(), _p(flag), _stream())
    return out


def window_gather_scaled(src, windows, tile, scaled_size, views=1, lut=None, out=None, flag=None):
    """rgda_window_gather_scaled: window_gather on the (Hs, Ws) = `scaled_size` image resize_bilinear_ac would make of the
    normalised source, without storing it; windows index the scaled image.  Arguments as window_gather."""
    hs, ws = (int(v) for v in scaled_size)
    return _window_gather('window_gather_scaled', src, windows, tile, views, lut, out, flag, hs, ws)


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
