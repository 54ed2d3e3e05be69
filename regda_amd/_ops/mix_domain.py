"""Cross-domain mixing: ClassMix / CutMix pastes and their tables (csrc/mix_domain_kernels.hip)."""
import torch

from .._lib import lib
from .base import _H, _check_operands, _need_cuda, _p, _stream, _table_check


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
    wr = 'written in place'
    _check_operands('domain_mix', (
        ('images_s', images_s, torch.float32, None, ''), ('images_t', images_t, torch.float32, None, wr),
        ('label_s', label_s, torch.int64, maps, ''), ('label_t', label_t, torch.int64, maps, wr),
        ('soft_t', soft_t, torch.float32, ((n, c, h, w),), wr), ('regs_t', regs_t, torch.int64, maps, wr)))
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


MIX_TABLE_COLS = _H['RGDA_MIX_TABLE_COLS']                  # {class_bits, y0, y1, x0, x1, 0, 0, 0} per image
MIX_WRITE_MAX_IMAGES = _H['RGDA_MIX_WRITE_MAX_IMAGES']      # rows mix_write_table carries in one launch


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
    _check_operands('domain_mix_table', (
        ('images_s', images_s, torch.float32, img, ''), ('images_in', images_in, torch.float32, img, ''),
        ('images_out', images_out, torch.float32, img, 'written'), ('label_s', label_s, torch.int64, maps, ''),
        ('label_t', label_t, torch.int64, maps, 'written'), ('soft_t', soft_t, torch.float32, ((n, c, h, w),), 'written')))
    if not 1 <= c <= MIX_MAX_CLASSES:
        raise ValueError('domain_mix_table: %d classes; the kernel serves 1..%d' % (c, MIX_MAX_CLASSES))
    if mode not in (MIX_CLASS, MIX_BOX):
        raise ValueError('domain_mix_table: mode must be MIX_CLASS or MIX_BOX, got %r' % (mode,))
    _table_check('domain_mix_table', table, n, MIX_TABLE_COLS, torch.int32)
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
    _table_check('mix_select_classes', table, n, MIX_TABLE_COLS, torch.int32)
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
    _table_check('mix_write_table', table, n, MIX_TABLE_COLS, torch.int32)
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
