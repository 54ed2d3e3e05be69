"""The fused upsample + loss family on the two heads' logits (csrc/loss_kernels.hip)."""
import ctypes
import math

import torch

from .._lib import lib
from .base import _grad_pair, _need_cuda, _p, _stream, _ws, _ws_unless


def _upsample_operands(p1, p2, label, class_weight, want_grad, g1, g2):
    """The operands of a fused upsample + loss call: f32 contiguous logits, the int64 label, the loss and gradient
    outputs (g1 / g2 allocated unless given; None without gradients), the class weights."""
    p1, p2 = p1.contiguous().float(), p2.contiguous().float()
    label = label.contiguous()
    assert label.dtype == torch.int64
    loss = torch.empty(1, dtype=torch.float32, device=p1.device)
    g1, g2 = _grad_pair(p1, p2, g1, g2, want_grad)
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
    g1, g2 = _grad_pair(p1, p2, g1, g2, want_grad, accumulate)
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
    g1, g2 = _grad_pair(p1, p2, g1, g2, want_grad, accumulate)
    L = lib()
    arr = (ctypes.c_int * nl)(*sizes)
    ws = _ws_unless(ws, p1.device, 'rgda_upsample_pycda_workspace', b, c, h, w, H, W, arr, nl)
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
    g1, g2 = _grad_pair(p1, p2, g1, g2, want_grad, accumulate)
    L = lib()
    if ws is None:
        ws = upsample_overlap_workspace(p1, label.shape)
    if heads == 1:
        p2 = p1
    L.call('rgda_upsample_overlap', heads, p1.data_ptr(), p2.data_ptr(), label.data_ptr(), alpha, beta, gamma, smooth,
           weight, int(bool(accumulate)), loss.data_ptr(), index.data_ptr(), present.data_ptr(), _p(g1), _p(g2), _p(flag), b,
           c, h, w, H, W, int(ignore_label), ws.data_ptr(), ws.numel(), _stream())
    return loss, index, present, g1, g2
