"""Category-wise feature losses: DCA class contexts with ICR / CCR / MSE (csrc/dca_kernels.hip) and
semantic-aware whitening (csrc/saw_kernels.hip); two small files, grouped."""
import torch

from .._lib import lib
from .base import _need_cuda, _p, _stream, _ws
from .feature import _feat_rows, _grad_rows, _loss_out


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
