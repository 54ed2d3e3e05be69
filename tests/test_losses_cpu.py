"""CPU: the restated --ls / --lt losses (tests/loss_ref.py) against the reference's own classes (tests/golden/losses.npz),
argument validation of rgda_upsample_loss, and the flag -> loss mapping of tools/train_ssl_reg.py:134-158."""
import ctypes

import numpy as np
import pytest
import torch

import loss_ref
from oracle import labelpath as olp

F0 = torch.tensor([0.4, 0.25, 0.1, 0.1, 0.1, 0.05])
CASES = ['ohem', 'ohem_topk', 'ohem_bal', 'ohem_ignored', 'focal', 'ghm', 'ups', 'ups_bal', 'uvem', 'uvem_bal',
         'uvem_zeros', 'ups_zeros', 'uvem_onehot']


def case(g, name):
    return {k.split('/', 1)[1]: g[k] for k in g.files if k.startswith(name + '/')}


def restated(name, c, calls=None):
    """-> [(loss, g1, g2) per call], the balancer / GHM state after the calls"""
    kind = name.split('_')[0]
    bal = None
    if name.endswith('_bal'):
        bal = olp.ClassBalanceState(6, -1, 0.9, 2.0)
        bal.freq = F0.clone()
    st = loss_ref.GhmState(0.99) if kind == 'ghm' else None
    fn = loss_ref.make_loss(kind, balancer=bal, ghm_state=st)
    lab = torch.from_numpy(c['lab'].astype(np.int64))
    soft = torch.from_numpy(c['soft']) if 'soft' in c else None
    out = []
    for _ in range(calls or (2 if kind == 'ghm' else 1)):
        p1, p2 = torch.from_numpy(c['p1']).requires_grad_(True), torch.from_numpy(c['p2']).requires_grad_(True)
        loss = loss_ref.loss_calc([p1, p2], lab, fn, soft)
        loss.backward()
        out.append((loss.detach(), p1.grad, p2.grad, None if st is None else st.acc_sum.clone()))
    return out, bal, st


@pytest.mark.parametrize('name', CASES)
def test_restated_losses_match_the_reference_goldens(gold, name):
    c = case(gold('losses.npz'), name)
    out, bal, st = restated(name, c)
    for k, (loss, g1, g2, acc) in enumerate(out):
        sfx = '' if k == 0 else str(k)
        ref = float(c['loss' + sfx])
        if np.isnan(ref):
            assert torch.isnan(loss)
        else:
            assert float(loss) == pytest.approx(ref, rel=2e-6)
        for got, key in ((g1, 'g1'), (g2, 'g2')):
            np.testing.assert_allclose(got.numpy(), c[key + sfx], rtol=1e-4, atol=1e-9)
        if acc is not None:
            np.testing.assert_allclose(acc.numpy(), c['acc' + sfx], rtol=1e-6)
    if bal is not None:
        np.testing.assert_allclose(bal.freq.numpy(), c['freq'], rtol=1e-6)


def test_the_fixture_covers_the_branches_and_quirks(gold):
    g = gold('losses.npz')
    # OHEM: the threshold branch and the top-k branch (fewer than n_min above -log 0.7), in both heads
    for name, topk in (('ohem', False), ('ohem_topk', True)):
        c = case(g, name)
        lab = torch.from_numpy(c['lab'].astype(np.int64))
        n_min = int((lab != -1).sum()) // 5
        for p in (c['p1'], c['p2']):
            v = loss_ref._ce(loss_ref.up(torch.from_numpy(p), (32, 32)), lab, -1)
            assert (int((v > loss_ref.OHEM_THRESH).sum()) < n_min) == topk
    # all labels ignored: NaN loss, zero gradient
    c = case(g, 'ohem_ignored')
    assert np.isnan(c['loss']) and not c['g1'].any() and not c['g2'].any()
    # GHM: saturated pixels (g == 0) are counted in bin 0 of the state
    c = case(g, 'ghm')
    g0 = loss_ref.ghm_g(loss_ref.up(torch.from_numpy(c['p1']), (32, 32)), torch.from_numpy(c['lab'].astype(np.int64)))
    assert int((g0 == 0).sum()) >= 50 and c['acc'][0] > 0 and c['acc1'][0] > c['acc'][0] * 0.99
    # exact zeros in the soft label: NaN entropy; a one-hot soft label: nothing counted, a loss of order 1e10
    for name in ('uvem_zeros', 'ups_zeros'):
        assert torch.isnan(loss_ref.entropy(torch.from_numpy(case(g, name)['soft']))).any()
    assert float(case(g, 'uvem_onehot')['loss']) > 1e8


def test_upsample_loss_rejects_bad_arguments():
    from regda_amd import _lib
    L = _lib.lib()
    assert L.size('rgda_upsample_loss_workspace', 1, 2, 6, 8, 8, 32, 32) > L.size('rgda_upsample_loss_workspace', 2, 2, 6, 8, 8, 32, 32)
    assert L.size('rgda_upsample_loss_workspace', 0, 2, 6, 8, 8, 32, 32) == 0
    assert L.size('rgda_upsample_loss_workspace', 6, 2, 6, 8, 8, 32, 32) == 0
    fake = ctypes.c_void_p(256)      # never dereferenced: the arguments are rejected first

    def call(kind=1, heads=2, p1=fake, p2=fake, label=fake, soft=None, cw=None, acc=None, m=0.2, t=0.7, gamma=4.0,
             thresh=0.36, mom=0.99, loss=fake, g1=fake, g2=fake, b=2, c=6, H=32, ws=fake, ws_bytes=1 << 30):
        L.call('rgda_upsample_loss', kind, heads, p1, p2, label, soft, cw, acc, m, t, gamma, thresh, mom, loss, g1, g2,
               b, c, 8, 8, H, 32, -1, ws, ws_bytes, None)
    for kw in (dict(kind=0), dict(kind=6), dict(heads=3), dict(heads=1, p2=ctypes.c_void_p(512)), dict(p1=None), dict(label=None),
               dict(loss=None), dict(g1=None), dict(ws=None), dict(b=0), dict(H=0),
               dict(kind=4), dict(kind=5), dict(kind=5, soft=fake, gamma=0.0), dict(kind=3),
               dict(kind=3, acc=fake, mom=1.0), dict(kind=2, cw=fake), dict(kind=3, acc=fake, cw=fake),
               dict(thresh=-1.0)):
        with pytest.raises(ValueError):
            call(**kw)
    with pytest.raises(ValueError):      # class count other than 6: unsupported
        call(c=5)
    with pytest.raises(_lib.RgdaError):  # workspace too small
        call(ws_bytes=16)


class _Balancer:
    pass


def test_flag_mapping_follows_train_ssl_reg():
    from regda_amd.gast import balance as B
    bs, bt = _Balancer(), _Balancer()
    s = B.source_loss('CrossEntropy', bs)
    assert type(s) is B.CrossEntropy and s.class_balancer is bs
    s = B.source_loss('OhemCrossEntropy', bs)
    assert type(s) is B.OhemCrossEntropy and s.class_balancer is bs
    assert s.thresh.dtype == torch.float32 and abs(float(s.thresh) - 0.35667494) < 5e-8    # f32 -log(0.7)
    for lt in ('ours', 'uvem'):
        f = B.target_loss(lt, bt, 0.3, 0.8, 2.0)
        assert type(f) is B.UVEMLoss and f.class_balancer is bt and (f.m, f.threshold, f.gamma) == (0.3, 0.8, 2.0)
    f = B.target_loss('ups', bt, 0.3, 0.8, 2.0)
    assert type(f) is B.UPSLoss and f.class_balancer is bt and f.threshold == 0.7
    # --bct is ignored by ohem, focal and ghm (train_ssl_reg.py:144-152)
    f = B.target_loss('ohem', bt)
    assert type(f) is B.OhemCrossEntropy and f.class_balancer is None
    f = B.target_loss('focal', bt)
    assert type(f) is B.FocalLoss and f.class_balancer is None and f.gamma == 2.0
    f = B.target_loss('ghm', bt, device='cpu')
    assert type(f) is B.GHMLoss and f.class_balancer is None and f.momentum == 0.99 and f.acc_sum.shape == (30,)
    f = B.target_loss('none', bt)
    assert type(f) is B.CrossEntropy and f.class_balancer is bt
    for bad in (lambda: B.source_loss('Focal'), lambda: B.target_loss('dice')):
        with pytest.raises(ValueError):
            bad()
    with pytest.raises(NotImplementedError):
        B.FocalLoss(alpha=torch.ones(6))
    np.testing.assert_allclose(B.UVEMLoss(m=0.2, threshold=0.7, gamma=4.0).get_weight(torch.tensor([0.0, 0.2, 0.45, 0.7])).numpy(),
                               loss_ref.uvem_weight(torch.tensor([0.0, 0.2, 0.45, 0.7]), 0.2, 0.7, 4.0).numpy())


def test_loss_modules_move_and_cast_like_any_module():
    """.to() / .cpu() / .float() go through nn.Module._apply, also from a parent module."""
    from regda_amd.gast import balance as B
    mods = [B.OhemCrossEntropy(), B.FocalLoss(), B.GHMLoss(device='cpu'), B.UPSLoss(), B.UVEMLoss(), B.CrossEntropy()]
    for m in mods:
        assert m.to('cpu') is m and m.cpu() is m and m.float() is m and m.double() is m
    parent = torch.nn.ModuleList(mods)
    assert parent.to('cpu') is parent and parent.float() is parent
