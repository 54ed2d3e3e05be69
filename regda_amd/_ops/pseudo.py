"""Pseudo-label statistics: IAST's adaptive thresholds -- fp16 histograms, percentiles, labels
(csrc/iast_kernels.hip) -- and the entropy-binned accuracy tables (csrc/analysis_kernels.hip); two small files,
grouped."""
import torch

from .._lib import lib
from .base import _H, _need_cuda, _stream, _ws, check_class_count


IAST_BINS = _H['RGDA_IAST_BINS']        # the non-negative fp16 bit patterns 0 .. 0x7C00


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


ANALYSIS_MAX_BINS = _H['RGDA_ANALYSIS_MAX_BINS']        # entropy bins of one rgda_pseudo_analysis call


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
