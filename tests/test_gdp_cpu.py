"""CPU: the restated GDPLoss and prototype pixel weight (tests/gdp_ref.py) against the reference's own classes
(tests/golden/gdp.npz), the Python surface of GDPLoss / target_loss('gdp'), and the ABI of rgda_upsample_gdp /
rgda_proto_pixel_weight (exports, plan table, argument errors)."""
import ctypes

import numpy as np
import pytest
import torch

import gdp_ref

# name -> (class count, class_balance, prototype_refine, momentum, calls, single prediction)
CASES = {
    'plain6': (6, False, False, 0.99, 1, False), 'plain7': (7, False, False, 0.99, 1, False),
    'cb6': (6, True, False, 0.99, 1, False), 'cb7': (7, True, False, 0.99, 1, False),
    'pr6': (6, False, True, 0.99, 1, False), 'pr7': (7, False, True, 0.99, 1, False),
    'both6': (6, True, True, 0.99, 1, False), 'both7': (7, True, True, 0.99, 1, False),
    'mom0': (6, False, False, 0.0, 1, False), 'state': (7, True, True, 0.99, 2, False),
    'ignored': (6, False, False, 0.99, 1, False), 'oneclass': (7, False, False, 0.99, 1, False),
    'saturated': (6, False, False, 0.99, 1, False), 'single': (7, True, False, 0.99, 1, True),
}


def case(g, name):
    """The case's inputs (its own over the base inputs of its class count) and the reference's outputs."""
    C = CASES[name][0]
    c = {k.split('/', 1)[1]: g[k] for k in g.files if k.startswith(f'c{C}/')}
    c.update({k.split('/', 1)[1]: g[k] for k in g.files if k.startswith(name + '/')})
    return c


def restated(name, c, dtype=torch.float32):
    """-> [(loss, g1, g2, acc_sum, bins_weight, freq) per call]"""
    C, cb, pr, mom, calls, single = CASES[name]
    st = gdp_ref.GdpState(mom, dtype)
    bal = gdp_ref.BalanceState(C, -1, 0.99, 0.5) if cb else None
    if bal is not None:
        bal.freq = bal.freq.to(dtype)
    lab = torch.from_numpy(c['lab'].astype(np.int64))
    pw = torch.from_numpy(c['pw']).to(dtype) if pr else None
    out = []
    for _ in range(calls):
        p1 = torch.from_numpy(c['p1']).to(dtype).requires_grad_(True)
        p2 = torch.from_numpy(c['p2']).to(dtype).requires_grad_(True)
        loss = gdp_ref.loss_calc(p1 if single else [p1, p2], lab, st, -1, pw, bal)
        if loss.requires_grad:
            loss.backward()
        z = torch.zeros_like(p1)
        out.append((loss.detach(), p1.grad if p1.grad is not None else z, p2.grad if p2.grad is not None else z,
                    st.acc_sum.clone(), st.bins_weight.clone(), None if bal is None else bal.freq.clone()))
    return out


@pytest.mark.parametrize('name', sorted(CASES))
def test_restated_gdp_matches_the_reference_goldens(gold, name):
    c = case(gold('gdp.npz'), name)
    single = CASES[name][5]
    for k, (loss, g1, g2, acc, bw, freq) in enumerate(restated(name, c)):
        sfx = '' if k == 0 else str(k)
        assert float(loss) == pytest.approx(float(c['loss' + sfx]), rel=2e-6, abs=0 if float(c['loss' + sfx]) else 1e-12)
        np.testing.assert_allclose(g1.numpy(), c['g1' + sfx], rtol=1e-4, atol=1e-9)
        if not single:
            np.testing.assert_allclose(g2.numpy(), c['g2' + sfx], rtol=1e-4, atol=1e-9)
        np.testing.assert_allclose(acc.numpy(), c['acc' + sfx], rtol=1e-6)
        np.testing.assert_allclose(bw.numpy(), c['bw' + sfx], rtol=1e-6)
        if freq is not None:
            np.testing.assert_allclose(freq.numpy(), c['freq' + sfx], rtol=1e-6)


@pytest.mark.parametrize('C', [6, 7])
def test_restated_prototype_weight_matches_the_reference_golden(gold, C):
    g = gold('gdp.npz')
    lab = torch.from_numpy(g[f'c{C}/lab'].astype(np.int64))
    got = gdp_ref.proto_weight(torch.from_numpy(g[f'c{C}/feat']), torch.from_numpy(g[f'c{C}/protos']), lab)
    ref = g[f'c{C}/pw']
    assert got.shape == ref.shape == (lab.numel(),)
    np.testing.assert_allclose(got.numpy(), ref, rtol=0, atol=1e-4)       # the project's bound for the refine goldens
    assert not ref[(lab == -1).reshape(-1).numpy()].any() and ref.max() > 0.999


def test_the_fixture_covers_the_branches_and_quirks(gold):
    g = gold('gdp.npz')
    # every label ignored: loss 0 / 1e-7 = 0, zero gradients, an empty histogram
    c = case(g, 'ignored')
    assert float(c['loss']) == 0.0 and not c['g1'].any() and not c['g2'].any() and not c['acc'].any() and not c['bw'].any()
    # the saturated block: g == 0 exactly; counted in bin 0 (and, symmetrised, in bin 29), bucket 0, weight 0
    c = case(g, 'saturated')
    lab = torch.from_numpy(c['lab'].astype(np.int64))
    g0 = gdp_ref.ghm_g(gdp_ref.up(torch.from_numpy(c['p1']), lab.shape[-2:]), lab)
    assert int((g0 == 0).sum()) >= 50
    # a one-class label map leaves most bins empty: their weight is the `where(acc_sum != 0, ., 0)` branch
    c = case(g, 'oneclass')
    assert int((c['acc'] == 0).sum()) >= 4 and not c['bw'][c['acc'] == 0].any()
    # symmetry of the histogram, momentum 0: acc_sum is the symmetrised histogram itself
    c = case(g, 'mom0')
    np.testing.assert_array_equal(c['acc'], c['acc'][::-1])
    assert c['acc'].sum() == pytest.approx(float((c['lab'] != -1).sum()))
    # state: the second call moves acc_sum and the balancer on (the bin weights are scale-free: the same inputs again
    # leave them where they were)
    c = case(g, 'state')
    assert (c['acc1'] > c['acc'] * 1.9).all() and not np.array_equal(c['freq1'], c['freq'])
    np.testing.assert_allclose(c['bw1'], c['bw'], rtol=1e-5)
    assert c['bw'].max() == pytest.approx(1.0, abs=1e-6)


class _Balancer:
    pass


def test_gdp_python_surface():
    from regda_amd.gast import balance as B
    assert 'gdp' in B.TARGET_LOSSES
    f = B.target_loss('gdp', None, class_num=7, device='cpu')
    assert type(f) is B.GDPLoss and f.kind == 'gdp' and f.class_balancer is None and f.momentum == 0.99
    assert f.acc_sum.shape == (30,) and f.bins_weight.shape == (30,) and f.bins_num == 30 and f.edges.shape == (31,)
    assert not f.class_balance and not f.prototype_refine
    # a balancer handed over is used only with class balancing on, and then replaces the internal one
    bt = _Balancer()
    assert B.target_loss('gdp', bt, device='cpu').class_balancer is None
    assert B.target_loss('gdp', bt, device='cpu', gdp_class_balance=True).class_balancer is bt
    assert B.GDPLoss(class_balance=True, class_balancer=bt, device='cpu').class_balancer is bt
    f = B.target_loss('gdp', None, device='cpu', gdp_prototype=True)
    assert f.prototype_refine
    with pytest.raises(RuntimeError, match='set_prototype_weight_4pixel'):
        f.launch(None, None, torch.zeros(1, 4, 4, dtype=torch.int64))
    f.set_prototype_weight_4pixel(torch.zeros(3))
    with pytest.raises(ValueError):
        f.launch(None, None, torch.zeros(1, 4, 4, dtype=torch.int64))
    with pytest.raises(NotImplementedError):
        B.GDPLoss(bins=31, device='cpu')
    # new keyword arguments sit at the end of target_loss's signature
    import inspect
    names = list(inspect.signature(B.target_loss).parameters)
    assert names[:8] == ['lt', 'class_balancer', 'uvem_m', 'uvem_t', 'uvem_g', 'class_num', 'ignore_label', 'device']
    assert names[8:10] == ['gdp_prototype', 'gdp_class_balance']
    m = B.GDPLoss(device='cpu')
    assert m.to('cpu') is m and m.float() is m
    from regda_amd import ops
    assert ops.LOSS_KINDS['gdp'] == 6
    from regda_amd.gast.alignment import Aligner
    assert callable(Aligner.get_prototype_weight_4pixel)


def test_gdp_abi_exports_plan_table_and_argument_errors():
    from regda_amd import _lib
    L = _lib.lib()
    for name in ('rgda_upsample_gdp', 'rgda_upsample_gdp_workspace', 'rgda_proto_pixel_weight',
                 'rgda_proto_pixel_weight_workspace'):
        assert name in L.protos and name not in L.missing
    assert L.raw('rgda_plan_fn_id')(b'rgda_upsample_gdp') >= 0 and L.raw('rgda_plan_fn_id')(b'rgda_proto_pixel_weight') >= 0
    assert L.raw('rgda_plan_fn_id')(b'rgda_upsample_gdp_workspace') == -1
    assert L.raw('rgda_abi_version')() == 10
    fake = ctypes.c_void_p(256)      # never dereferenced: the arguments are rejected first
    # the kind exists, and rgda_upsample_loss refuses it: it needs the other entry point
    assert L.size('rgda_upsample_loss_workspace', 6, 2, 6, 8, 8, 32, 32) == 0
    with pytest.raises(ValueError):
        L.call('rgda_upsample_loss', 6, 2, fake, fake, fake, None, None, fake, 0.2, 0.7, 4.0, 0.36, 0.99, fake, fake, fake,
               2, 6, 8, 8, 32, 32, -1, fake, 1 << 30, None)
    # GDP's workspace is GHM's layout: header, row partials, T, 2 bytes per pixel
    assert L.size('rgda_upsample_gdp_workspace', 2, 6, 8, 8, 32, 32) == L.size('rgda_upsample_loss_workspace', 3, 2, 6, 8, 8, 32, 32)
    assert L.size('rgda_upsample_gdp_workspace', 0, 6, 8, 8, 32, 32) == 0

    def gdp(heads=2, p1=fake, p2=fake, label=fake, pw=None, cw=None, acc=fake, bw=fake, mom=0.99, loss=fake, g1=fake,
            g2=fake, b=2, c=6, H=32, ws=fake, ws_bytes=1 << 30):
        L.call('rgda_upsample_gdp', heads, p1, p2, label, pw, cw, acc, bw, mom, loss, g1, g2, b, c, 8, 8, H, 32, -1, ws,
               ws_bytes, None)
    for kw in (dict(heads=0), dict(heads=3), dict(heads=1, p2=ctypes.c_void_p(512)), dict(p1=None), dict(p2=None),
               dict(label=None), dict(acc=None), dict(bw=None), dict(loss=None), dict(g1=None), dict(g2=None), dict(ws=None),
               dict(mom=1.0), dict(mom=-0.1), dict(b=0), dict(H=0)):
        with pytest.raises(ValueError):
            gdp(**kw)
    with pytest.raises(ValueError):      # class counts outside 6..16: unsupported
        gdp(c=5)
    with pytest.raises(ValueError):
        gdp(c=17)
    with pytest.raises(_lib.RgdaError):  # workspace too small
        gdp(ws_bytes=16)

    def ppw(feat=fake, protos=fake, sim=None, label=fake, out=fake, b=2, k=64, c=6, h=8, w=8, H=32, ws=fake,
            ws_bytes=1 << 30):
        L.call('rgda_proto_pixel_weight', feat, protos, sim, label, out, b, k, c, h, w, H, 32, -1, ws, ws_bytes, None)
    for kw in (dict(feat=None), dict(protos=None), dict(label=None), dict(out=None), dict(ws=None), dict(b=0), dict(H=0),
               dict(k=1), dict(k=66), dict(k=8192), dict(sim=fake, label=None), dict(sim=fake, out=None)):
        with pytest.raises(ValueError):
            ppw(**kw)
    for kw in (dict(c=5), dict(c=17), dict(c=16, k=4096),        # the prototypes do not fit in LDS (label_refine's limit)
               dict(c=16, w=513, sim=fake)):                     # the staged sim rows pass 64 KB
        with pytest.raises(ValueError):
            ppw(**kw)
    with pytest.raises(_lib.RgdaError):
        ppw(ws_bytes=16)
    assert L.size('rgda_proto_pixel_weight_workspace', 2, 6, 64, 8, 8) >= (2 * 6 * 64 + 6 + 6 * 64) * 4
