"""CategoryAlign_Module, ICR, CCR, MSE_intra, MSE_cross -- mirror of regda/dca_modules.py (Deep Covariance Alignment, the
LoveDA authors' domain-adaptation baseline) on rgda_dca_context / rgda_dca_loss.

The reference forms the (b, C, c, hw) product feats * preds in get_context and walks the n x n Pearson coefficients in
Python.  The kernels read the feature map once per side, form the class probabilities from the logits in registers (they
are never written), and leave the gradient w.r.t. the features as pixel-major bf16 rows in the same call; backward scales
the stored rows by the incoming gradient.  The predictions are constants, as in the reference (detached).

Kept from the reference: F.normalize(dim=1) in get_context runs over the CLASS axis; a non-positive diagonal entry of
the correlation matrix gives a NaN loss (regularize takes its logarithm unclamped).  `get_intra_corcoef_mat` is commented
out at its only call site in the reference and is left out."""
import torch
import torch.nn as nn

from . import ops
from .gast._rowsgrad import rows_loss


class CategoryAlign_Module(nn.Module):
    def __init__(self, num_classes=7, ignore_bg=False):
        super().__init__()
        self.num_classes = num_classes
        self.ignore_bg = ignore_bg

    def get_context(self, preds, feats):
        """preds (b, C, h, w) probabilities, feats (b, c, h, w) -> (b, n, c) (dca_modules.py:20-34).  Not differentiable:
        the losses below carry the gradient."""
        return ops.dca_context(feats.detach(), preds, 'prob', self.ignore_bg)

    def get_cross_corcoef_mat(self, preds1, feats1, preds2, feats2):
        """-> (n, n): the Pearson coefficients over the channels of the batch-mean contexts (dca_modules.py:47-57)"""
        a = self.get_context(preds1, feats1).mean(0)
        b = self.get_context(preds2, feats2).mean(0)
        a = a - a.mean(1, keepdim=True)
        b = b - b.mean(1, keepdim=True)
        return (a @ b.t()) / (a.norm(dim=1)[:, None] * b.norm(dim=1)[None, :])

    def regularize(self, cor_mat):
        """dca_modules.py:59-76"""
        n = self.num_classes - 1 if self.ignore_bg else self.num_classes
        assert cor_mat.size()[0] == n
        pos = -torch.log(torch.diag(cor_mat)).mean()
        undiag = cor_mat.flatten()[:-1].view(n - 1, n + 1)[:, 1:].flatten()
        neg = -torch.log(1 - undiag.clamp(min=1e-6)).mean()
        return pos + neg


def _split(inputs, multi_layer):
    """(preds1, preds2, feats) or (preds, feats) -> (the prediction maps, feats, pred_kind)"""
    if multi_layer:
        p1, p2, feats = inputs
        return (p1, p2), feats, 'logits2'
    p, feats = inputs
    return (p,), feats, 'logits'


def _check_classes(preds, num_classes):
    if num_classes is not None and preds[0].shape[1] != num_classes:
        raise ValueError(f'num_classes = {num_classes}, the predictions have {preds[0].shape[1]} classes')


def _intra(inputs, kind, multi_layer, ignore_bg, num_classes=None):
    preds, feats, pk = _split(inputs, multi_layer)
    _check_classes(preds, num_classes)
    B = feats.shape[0]
    if B < 2:
        raise ValueError('the intra-domain terms split the batch in two: at least two images')
    h = B // 2
    pa, pb = tuple(p[:h] for p in preds), tuple(p[h:] for p in preds)

    def op(x, g):
        hw = x.shape[2] * x.shape[3]
        ga, gb = (None, None) if g is None else (g[:h * hw], g[h * hw:])
        return ops.dca_loss(x[:h], pa, x[h:], pb, pk, kind, ignore_bg, dfeat_a=ga, dfeat_b=gb)
    return rows_loss(op, feats)


def _cross(source, target, kind, multi_layer, ignore_bg, num_classes=None):
    sp, sf, pk = _split(source, multi_layer)
    tp, tf, _ = _split(target, multi_layer)
    _check_classes(sp, num_classes)
    sf = sf.detach()
    return rows_loss(lambda x, g: ops.dca_loss(sf, sp, x, tp, pk, kind, ignore_bg, dfeat_b=g), tf)


def ICR(inputs, num_classes, multi_layer=False, ignore_bg=True):
    """Intra-domain Covariance Regularization (dca_modules.py:79-105)"""
    return _intra(inputs, 'cov', multi_layer, ignore_bg, num_classes)


def CCR(source, target, num_classes, multi_layer=False, ignore_bg=True):
    """Cross-domain Covariance Regularization (dca_modules.py:108-133): the gradient reaches the target features only"""
    return _cross(source, target, 'cov', multi_layer, ignore_bg, num_classes)


def MSE_intra(inputs, multi_layer=False, ignore_bg=True):
    """MSE-Alignment for intra domain (dca_modules.py:136-159); the two halves hold equally many images"""
    return _intra(inputs, 'mse', multi_layer, ignore_bg)


def MSE_cross(source, target, multi_layer=False, ignore_bg=True):
    """MSE-Alignment for cross domain (dca_modules.py:162-188): the gradient reaches the target features only"""
    return _cross(source, target, 'mse', multi_layer, ignore_bg)
