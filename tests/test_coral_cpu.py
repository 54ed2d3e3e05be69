"""CPU: the CORAL arithmetic contract of rgda_coral_loss (include/rgda_hip.h), restated here from the formulas,
against the reference's own CoralLoss / Aligner.align_domain (tests/golden/coral.npz); argument validation of the new
entry points (no GPU needed: every check comes before a launch)."""
import ctypes

import numpy as np
import pytest
import torch


def coral_restated(xs, xt):
    """rows (ns, d), (nt, d) -> (loss, dL/dxs, dL/dxt), float64:
        mu = column means, Xc = X - mu, C = Xc^T Xc / (n - 1), D = Cs - Ct, L = sum(D^2) / (4 d^2)
        dL/dXs = Xcs D / (d^2 (ns - 1)),  dL/dXt = -Xct D / (d^2 (nt - 1))"""
    xs, xt = xs.double(), xt.double()
    d, ns, nt = xs.shape[1], xs.shape[0], xt.shape[0]
    cs, ct = xs - xs.mean(0), xt - xt.mean(0)
    D = cs.T @ cs / (ns - 1) - ct.T @ ct / (nt - 1)
    return (D * D).sum() / (4 * d * d), cs @ D / (d * d * (ns - 1)), -(ct @ D) / (d * d * (nt - 1))


def _rows(x):
    return x.permute(0, 2, 3, 1).reshape(-1, x.shape[1]) if x.dim() == 4 else x


def coral_cases(g):
    """the three fixture cases as (xs, xt) tensors in their stored shapes"""
    for i in range(3):
        a, s, o = (float(v) for v in g['scales'][i])
        xs = torch.from_numpy(g[f'qs{i}'].astype(np.float32) / 32.0) * a
        xt = torch.from_numpy(g[f'qt{i}'].astype(np.float32) / 32.0) * s + o
        yield i, xs, xt


def test_restated_coral_matches_the_reference_goldens(gold):
    g = gold('coral.npz')
    for i, xs, xt in coral_cases(g):
        loss, gs, gt = coral_restated(_rows(xs), _rows(xt))
        np.testing.assert_allclose(float(loss), float(g[f'loss{i}']), rtol=2e-5)
        ref_s, ref_t = (torch.from_numpy(g[k + str(i)]) for k in ('gs', 'gt'))
        # the autograd gradient includes the mean term, which vanishes (D symmetric, centred rows sum to zero)
        for got, ref in ((gs, ref_s), (gt, ref_t)):
            ref = _rows(ref).double()
            assert (got - ref).abs().max().item() <= 1e-4 * ref.abs().max().item() + 1e-12, i


def test_coral_entry_points_reject_bad_arguments():
    from regda_amd import _lib
    L = _lib.lib()
    assert L.size('rgda_coral_loss_workspace', 64, 80, 64) > 0
    for ns, nt, d in ((1, 64, 64), (64, 1, 64), (64, 64, 100), (64, 64, 0)):
        assert L.size('rgda_coral_loss_workspace', ns, nt, d) == 0
    fake = ctypes.c_void_p(256)       # never dereferenced: the arguments are rejected first

    def call(feat_s=fake, bs=2, hws=16, feat_t=fake, bt=2, hwt=16, d=64, loss=fake, dfs=None, ldds=0, ws=fake):
        L.call('rgda_coral_loss', feat_s, bs, hws, hws, d * hws, feat_t, bt, hwt, hwt, d * hwt, d, loss, dfs, ldds,
               None, 0, 0, 1.0, ws, 1 << 30, None)
    for kw in (dict(feat_s=None), dict(feat_t=None), dict(loss=None), dict(ws=None),
               dict(bs=1, hws=1), dict(bt=1, hwt=1), dict(d=100), dict(d=0), dict(dfs=fake, ldds=60)):
        with pytest.raises(ValueError):
            call(**kw)
    with pytest.raises(_lib.RgdaError):          # workspace too small
        L.call('rgda_coral_loss', fake, 2, 16, 16, 1024, fake, 2, 16, 16, 1024, 64, fake, None, 0, None, 0, 0, 1.0,
               fake, 16, None)
