"""Histogram matching of the source tile (csrc/hist_kernels.hip; include/rgda_hip.h: rgda_hist_style carries the
contract).  Not part of the flat regda_amd.ops namespace yet: regda_amd.aug.histogram re-exports these."""
import torch

from .._lib import lib
from .base import _H, _check_operands, _need_cuda, _out_like, _p, _stream, _table_check, _write_host_table, _ws, _ws_or

HIST_BLEND_ONE = _H['RGDA_HIST_BLEND_ONE']          # blend_q of a full match: beta = blend_q / 65536
_COLS, _MAX_IMAGES = _H['RGDA_STYLE_TABLE_COLS'], _H['RGDA_STYLE_MAX_IMAGES']


def hist_style_write_table(table, host, n_targets, size):
    """rgda_hist_style_write_table: table (int32 (N, 4) on the device, N <= 16) <- host (an int32 numpy array of that
    shape: partner, blend_q, on, 0 per source image -- HistogramStyle.draw), carried in the launch's arguments: the host
    buffer is read before this returns.  n_targets: the target images the partners index; size = (H, W) of the tiles.  A
    row that is not served (a partner outside [0, n_targets), blend_q outside [0, 65536], on not 0 or 1) is a ValueError
    before any launch."""
    return _write_host_table('hist_style_write_table', table, host, _COLS, 'int32', size, int(n_targets))


def hist_style_workspace(n, m, h, w, device):
    """A workspace for hist_style(ws=) at n source and m target tiles of h x w: a uint8 tensor of
    rgda_hist_style_workspace(n, m, h, w) bytes; ValueError for a shape that is not served."""
    need = lib().size('rgda_hist_style_workspace', int(n), int(m), int(h), int(w))
    if need == 0:
        raise ValueError('hist_style: %d + %d tiles of %d x %d are not served (1..%d images of each, H, W <= 4096)'
                         % (n, m, h, w, _MAX_IMAGES))
    return _ws(need, device)


def hist_style(images_s, images_t, table, mean_s, std_s, mean_t, std_t, out=None, ws=None, flag=None, hist=None, lut=None):
    """rgda_hist_style: per-channel histogram matching of normalised source tiles -- the grey levels of source image n
    are mapped onto the distribution of its partner target image and blended with weight blend_q / 65536, as row n of
    `table` (int32 (N, 4) on the device: partner, blend_q, on, 0) says; include/rgda_hip.h carries the semantics.
    images_s f32 (N,3,H,W) and images_t f32 (M,3,H,W), N, M <= 16, never written; out: the result (allocated unless
    given), a different buffer.  mean_*, std_*: three values each, the normalisation the source and the target tiles
    carry.  ws: workspace of rgda_hist_style_workspace(N, M, H, W) bytes, a uint8 tensor (allocated unless given; the
    call rewrites it).  flag: optional device int32, set to 1 by a row that is not served (that image is copied).
    hist: optional int32 (N + M, 3, 256), written with the histograms, the source images first; lut: optional float64
    (N, 3, 256), written with the matched levels L.  -> out."""
    _need_cuda(images_s, images_t, table, out, ws, flag, hist, lut)
    for name, x in (('images_s', images_s), ('images_t', images_t)):
        if x.dim() != 4 or x.shape[1] != 3 or x.dtype != torch.float32:
            raise ValueError('hist_style: %s must be torch.float32 (N,3,H,W), got %s %s' % (name, x.dtype, tuple(x.shape)))
    n, _, h, w = images_s.shape
    m = images_t.shape[0]
    if tuple(images_t.shape[-2:]) != (h, w):
        raise ValueError('hist_style: source and target tiles must have one size, got %s and %s'
                         % (tuple(images_s.shape[-2:]), tuple(images_t.shape[-2:])))
    if not 1 <= n <= _MAX_IMAGES or not 1 <= m <= _MAX_IMAGES:
        raise ValueError('hist_style: %d source and %d target images; the kernels serve 1..%d of each' % (n, m, _MAX_IMAGES))
    _table_check('hist_style', table, n, _COLS, torch.int32)
    _check_operands('hist_style', [('hist', hist, torch.int32, ((n + m, 3, 256),), 'written'),
                                   ('lut', lut, torch.float64, ((n, 3, 256),), 'written')])
    norms = [tuple(float(v) for v in t) for t in (mean_s, std_s, mean_t, std_t)]
    if any(len(t) != 3 for t in norms) or not all(v > 0 for v in norms[1] + norms[3]):
        raise ValueError('hist_style: mean and std are three values each, std positive')
    out = _out_like('hist_style', out, images_s)
    if h * w == 0:
        return out
    need = lib().size('rgda_hist_style_workspace', n, m, h, w)
    if need == 0:
        raise ValueError('hist_style: %d x %d tiles are not served (H, W <= 4096)' % (h, w))
    ws = _ws_or('hist_style', ws, need, images_s.device)
    src, tgt = images_s.contiguous(), images_t.contiguous()
    if out.data_ptr() in (src.data_ptr(), tgt.data_ptr()):
        raise ValueError('hist_style: out must not be an input (the transform is out of place)')
    lib().call('rgda_hist_style', src.data_ptr(), tgt.data_ptr(), out.data_ptr(), table.data_ptr(), ws.data_ptr(), n, m, h, w,
               *norms[0], *norms[1], *norms[2], *norms[3], _p(hist) or None, _p(lut) or None, _p(flag) or None, _stream())
    return out
