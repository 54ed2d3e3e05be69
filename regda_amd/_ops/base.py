"""What every family module uses: the class-count and step-shape checks, the cached stream, pointer and device
checks, the BatchNorm statistics format, workspaces, and the operand helpers the once-per-step wrappers share.
The checks read rgda_class_lds (csrc/abi.hip)."""
import torch

from .. import _header
from .._lib import lib

_H = _header.constants()        # the integer #defines of include/rgda_hip.h, by their C names


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


STAT_FRAC_FWD, STAT_FRAC_BWD = _H['RGDA_STAT_FRAC_FWD'], _H['RGDA_STAT_FRAC_BWD']      # fraction bits of rgda_stat_t


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


def _ld(t):
    assert t.dim() == 2 and t.stride(1) == 1
    return t.stride(0)


# Operand helpers of the once-per-step wrappers.  One that raises ValueError serves only sites that raise ValueError for
# that condition; a site that asserts keeps its assert.

def _grad_pair(p1, p2, g1, g2, want_grad, accumulate=False):
    """The gradient outputs of an upsample loss: allocated like p1 / p2 unless given; (None, None) without gradients."""
    if not want_grad:
        return None, None
    assert not accumulate or (g1 is not None and g2 is not None), 'accumulate adds onto given gradients'
    g1 = torch.empty_like(p1) if g1 is None else g1
    g2 = torch.empty_like(p2) if g2 is None else g2
    assert g1.is_contiguous() and g2.is_contiguous() and g1.shape == p1.shape and g2.shape == p2.shape
    return g1, g2


def _ws_unless(ws, device, query, *args):
    """`ws` when given (the entry point checks its length), else a new workspace of the size query's bytes."""
    return _ws(lib().size(query, *args), device) if ws is None else ws


def _ws_or(who, ws, need, device):
    """A workspace of `need` bytes, allocated unless given; ValueError for a given one that is not that."""
    if ws is None:
        ws = _ws(need, device)
    if ws.dtype != torch.uint8 or ws.numel() < need or not ws.is_contiguous():
        raise ValueError('%s: ws must be contiguous %s with at least %d bytes' % (who, torch.uint8, need))
    return ws


def _out_like(who, out, like):
    """A contiguous output of the dtype and shape of `like`, allocated unless given; ValueError for another."""
    if out is None:
        out = torch.empty(like.shape, dtype=like.dtype, device=like.device)
    if out.dtype != like.dtype or tuple(out.shape) != tuple(like.shape) or not out.is_contiguous():
        raise ValueError('%s: out is written and must be contiguous %s %s' % (who, like.dtype, tuple(like.shape)))
    return out


def _table_check(who, table, n, cols, dtype):
    if table.dtype != dtype or tuple(table.shape) != (n, cols) or not table.is_contiguous():
        raise ValueError('%s: table must be contiguous %s (%d, %d), got %s %s'
                         % (who, dtype, n, cols, table.dtype, tuple(table.shape)))


def _write_host_table(who, table, host, cols, dtype, size, *extra):
    """rgda_<who>: the device table (N, cols) <- the host array of that shape, carried in the launch's arguments.  dtype:
    the name numpy and torch share; size = (H, W) of the tiles; extra: the entry point's arguments between n and h."""
    import numpy as np
    _need_cuda(table)
    n = table.shape[0]
    _table_check(who, table, n, cols, getattr(torch, dtype))
    host = np.ascontiguousarray(host, dtype=dtype)
    if host.shape != (n, cols):
        raise ValueError('%s: host must be %s (%d, %d), got %s' % (who, dtype, n, cols, host.shape))
    h, w = (int(v) for v in size)
    lib().call('rgda_' + who, table.data_ptr(), host.ctypes.data, n, *extra, h, w, _stream())
    return table


def _check_operands(who, want):
    """want: rows (name, tensor or None, dtype, admitted shapes or None, '' or how it is written: then contiguous)."""
    for name, t, dt, shapes, written in want:
        if t is None:
            continue
        if t.dtype != dt or (shapes is not None and tuple(t.shape) not in shapes):
            raise ValueError('%s: %s must be %s %s, got %s %s' % (who, name, dt, shapes, t.dtype, tuple(t.shape)))
        if written and not t.is_contiguous():
            raise ValueError('%s: %s is %s and must be contiguous' % (who, name, written))
