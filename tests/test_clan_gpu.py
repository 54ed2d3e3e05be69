"""GPU: the kernels of csrc/clan_kernels.hip alone, through regda_amd.ops, per element against the float64 restatement
(tests/clan_ref.py) at the smallest shapes where they can go wrong, and WeightedBCEWithLogitsLoss against the goldens
minted from the reference's own module.  Every bound comes from tests/golden/clan_tolerances.json
(derive_clan_tolerances.py); none is set by hand.  Every op is run twice and must repeat its bits.  Each test prints its
figures before it asserts."""
import json
import os

import pytest
import torch

import clan_ref as C

R = C.R
pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
BF = torch.bfloat16


@pytest.fixture(scope='module')
def tol():
    return json.load(open(os.path.join(HERE, 'golden', 'clan_tolerances.json')))


@pytest.fixture(scope='module')
def ops():
    from regda_amd import ops
    return ops


def check(name, got, ref, bound):
    e = R.err(got.detach().cpu(), ref)
    print('[clan %s] err %.3e bound %.3e' % (name, e, bound))
    assert torch.isfinite(got).all(), name
    assert e < bound, (name, e, bound)


@pytest.mark.parametrize('name', list(C.PAIR_CASES))
def test_pair_probabilities_forward_and_backward(ops, tol, name):
    c, t = C.pair_case(name), tol['pair'][name]
    ref = C.pair_reference(c)
    b, Cn, H, W = c['b'], c['C'], c['H'], c['W']
    x1, x2 = c['x1'].cuda(), c['x2'].cuda()
    P, wmap = ops.clan_probs(x1, x2, c['size'])
    assert P.shape == (b * H * W, 16) and P.dtype == BF and (P[:, Cn:] == 0).all(), 'the padding channels are zero'
    assert wmap.shape == (b, H, W) and wmap.dtype == torch.float32
    check('pair %s P' % name, R.nchw(P[:, :Cn].double(), b, H, W), ref['P'], t['P'])
    e = float((wmap.double().cpu() - ref['wmap']).abs().max())
    print('[clan pair %s wmap] abs err %.3e bound %.3e (max %.3e)' % (name, e, t['wmap'], float(ref['wmap'].max())))
    assert torch.isfinite(wmap).all() and e < t['wmap']
    if name.startswith('same'):
        assert float(ref['wmap'].abs().max()) < 1e-15 and float(wmap.abs().max()) < t['wmap']
    P2, wmap2 = ops.clan_probs(x1, x2, c['size'])
    assert torch.equal(P, P2) and torch.equal(wmap, wmap2), 'two runs are bit-identical'
    dP = R.rows(R.pad_classes(c['dP'])).to(BF).cuda()
    for key, gw in (('', c['gw'].cuda()), ('_nogw', None)):
        dx1, dx2 = torch.zeros_like(x1), torch.zeros_like(x2)
        ops.clan_probs_backward(dP, gw, x1, x2, dx1, dx2, c['size'])
        check('pair %s dx1%s' % (name, key), dx1.double(), ref['dx1' + key], t['dx1' + key])
        check('pair %s dx2%s' % (name, key), dx2.double(), ref['dx2' + key], t['dx2' + key])
        # the gradient is ADDED, times the scale: one product by a power of two and one f32 addition per element
        base1, base2 = torch.randn_like(x1), torch.randn_like(x2)
        for _ in range(2):
            a1, a2 = base1.clone(), base2.clone()
            ops.clan_probs_backward(dP, gw, x1, x2, a1, a2, c['size'], scale=0.5)
            for a, base, dx in ((a1, base1, dx1), (a2, base2, dx2)):
                want = base.double() + 0.5 * dx.double()
                assert ((a.double() - want).abs() <= R.U32 * want.abs() + 1e-45).all()
            if _:
                assert torch.equal(a1, keep[0]) and torch.equal(a2, keep[1]), 'two runs are bit-identical'
            keep = (a1, a2)
    if name.startswith('same'):         # x1 == x2: both heads receive the same gradient
        assert torch.equal(dx1, dx2)


_WBCE = {}


def wbce_run(shape, v):
    if shape not in _WBCE:
        _WBCE[shape] = (C.wbce_case(shape), {})
    c, refs = _WBCE[shape]
    if v not in refs:
        refs[v] = C.wbce_reference(c, v)
    return c, refs[v]


@pytest.mark.parametrize('shape,v', [(s, v) for s in C.WBCE_SHAPES for v in C.wbce_variants(s)],
                         ids=lambda p: p if isinstance(p, str) else C.variant_name(p))
def test_weighted_bce_on_an_upsampled_map(ops, tol, shape, v):
    target, use_w, mean, acc, want_dz, want_gw = v
    c, ref = wbce_run(shape, v)
    t = tol['wbce'][C.bounds_key(shape, v)]
    assert float(c['z'].abs().max()) == 80.0, 'the ends of the stable form are part of every case'
    z = c['z'].cuda()
    tgt = c['target'].cuda() if target == 'tensor' else target
    wmap = c['wmap'].cuda() if use_w else None
    START = 2.0
    outs = []
    for _ in range(2):
        loss = torch.full((1,), START, device='cuda') if acc else None
        loss, dz, gw = ops.wbce_logits(z, c['size'], tgt, wmap, C.ALPHA, C.BETA, C.SCALE, mean, loss=loss, accumulate=acc,
                                       want_dz=want_dz, want_gw=want_gw)
        outs.append((loss.clone(), dz, gw))
    (loss, dz, gw), again = outs
    assert all((a is None and b is None) or torch.equal(a, b) for a, b in zip(outs[0], again)), 'two runs are bit-identical'
    want = float(ref['loss'])
    got = loss.item() - (START if acc else 0.0)
    # onto a loss of 2.0 the sum is rounded once more, to an f32 of the size of the total
    bound = t['loss'] * abs(want) + (2 * R.U32 * (START + abs(want)) if acc else 0.0)
    print('[clan wbce %s %s] loss %.9g ref %.9g (+- %.2e)' % (shape, C.variant_name(v), got, want, bound))
    assert torch.isfinite(loss).all() and abs(got - want) < bound
    assert (dz is None) == (not want_dz) and (gw is None) == (not want_gw)
    if want_dz:
        assert dz.shape == z.shape
        check('wbce %s %s dz' % (shape, C.variant_name(v)), dz.double(), ref['dz'], t['dz'])
    if want_gw:
        assert gw.shape == (c['b'], c['H'], c['W'])
        check('wbce %s %s gw' % (shape, C.variant_name(v)), gw.double(), ref['gw'], t['gw'])


def test_weighted_bce_refuses_what_it_does_not_serve(ops):
    z = torch.zeros(2, 1, 1, device='cuda')
    with pytest.raises(ValueError, match='0 or 1'):
        ops.wbce_logits(z, (32, 32), 0.5)
    with pytest.raises(ValueError, match='no weight map'):
        ops.wbce_logits(z, (32, 32), 0, None, want_gw=True)


@pytest.mark.parametrize('name', list(C.GOLDEN_CASES))
def test_module_matches_the_references_own_loss(gold, tol, name):
    from regda_amd.loss import WeightedBCEWithLogitsLoss
    c, t = C.golden_case(gold, name), tol['golden'][name]
    crit = WeightedBCEWithLogitsLoss(size_average=c['size_average'])
    runs = []
    for _ in range(2):
        x = c['input'].cuda().requires_grad_(True)
        w = None if c['weight'] is None else c['weight'].cuda().requires_grad_(True)
        loss = crit(x, c['target'].cuda(), w, c['alpha'], c['beta'])
        assert loss.shape == () and loss.dtype == torch.float32
        (3.0 * loss).backward()
        runs.append((loss.detach().clone(), x.grad, None if w is None else w.grad))
    (loss, dx, dw), again = runs
    assert all((a is None and b is None) or torch.equal(a, b) for a, b in zip(runs[0], again)), 'two runs are bit-identical'
    want = float(c['loss'])
    print('[clan golden %s] loss %.9g ref %.9g (rel bound %.2e)' % (name, loss.item(), want, t['loss']))
    assert torch.isfinite(loss) and abs(loss.item() - want) < t['loss'] * abs(want)
    # backward scales the stored gradients by the upstream gradient: one more rounding
    check('golden %s dinput' % name, dx.double() / 3.0, c['dinput'], t['dz'] + R.U32)
    assert dx.shape == c['input'].shape
    if w is not None:
        check('golden %s dweight' % name, dw.double() / 3.0, c['dweight'], t['gw'] + R.U32)
    # a weight that needs no gradient gets none; an input that needs none neither
    x = c['input'].cuda().requires_grad_(True)
    w = None if c['weight'] is None else c['weight'].cuda()
    loss2 = crit(x, c['target'].cuda(), w, c['alpha'], c['beta'])
    loss2.backward()
    assert torch.equal(loss2.detach(), loss) and (w is None or w.grad is None)


def test_refusals_return_their_status_and_launch_nothing(ops):
    """every refusal leaves the output buffers as they were: the status is returned before the first launch"""
    from regda_amd import _lib
    L = _lib.lib()
    ARG, UNSUP = -1, -4
    b, Cn, h, w, H, W = 2, 6, 2, 2, 32, 32
    x = torch.randn(b, 17, h, w, device='cuda')
    P = torch.full((b * H * W + 1, 16), 7.0, dtype=BF, device='cuda')
    wm, gwb = torch.full((b * H * W,), 7.0, device='cuda'), torch.full((b * H * W,), 7.0, device='cuda')
    dx = torch.full((2, b, 17, h, w), 7.0, device='cuda')
    s = torch.cuda.current_stream().cuda_stream

    def fwd(x1=x.data_ptr(), P_=P.data_ptr(), wmap=wm.data_ptr(), C_=Cn, Cp=16):
        return L.raw('rgda_clan_probs_fwd')(x1, x.data_ptr(), P_, wmap, b, C_, h, w, H, W, Cp, s)

    def bwd(dP=P.data_ptr(), x1=x.data_ptr(), dx1=dx[0].data_ptr(), C_=Cn, Cp=16):
        return L.raw('rgda_clan_probs_bwd')(dP, wm.data_ptr(), x1, x.data_ptr(), dx1, dx[1].data_ptr(), b, C_, h, w, H, W, Cp,
                                            1.0, s)

    for f in (fwd, bwd):
        assert f(C_=5) == UNSUP and f(C_=17) == UNSUP and f(Cp=8) == UNSUP and f(Cp=32) == UNSUP, f.__name__
        assert f(x1=None) == ARG, f.__name__
    assert fwd(P_=P.data_ptr() + 2) == ARG and fwd(P_=None) == ARG and fwd(wmap=None) == ARG
    assert bwd(dP=P.data_ptr() + 2) == ARG and bwd(dP=None) == ARG and bwd(dx1=None) == ARG
    z, loss, ws = torch.zeros(b, device='cuda'), torch.full((1,), 7.0, device='cuda'), torch.empty(4096, dtype=torch.uint8, device='cuda')

    def wb(z_=z.data_ptr(), label=0.0, wmap=wm.data_ptr(), loss_=loss.data_ptr(), gw=gwb.data_ptr(), ws_bytes=4096, H_=H):
        return L.raw('rgda_wbce_logits')(z_, b, 1, 1, H_, W, None, label, wmap, 0.4, 40.0, 1.0, 1, loss_, 0, dx.data_ptr(), gw,
                                         ws.data_ptr(), ws_bytes, s)

    assert wb(z_=None) == ARG and wb(loss_=None) == ARG and wb(label=0.5) == ARG and wb(wmap=None) == ARG and wb(H_=0) == ARG
    assert wb(ws_bytes=16) == -2
    for name in ('clan_probs', 'clan_probs_backward'):
        with pytest.raises(ValueError, match='classes'):
            args = (x, x) if name == 'clan_probs' else (P[:b * H * W], None, x, x, dx[0], dx[1])
            getattr(ops, name)(*args, size=(H, W))
    torch.cuda.synchronize()
    assert (P == 7.0).all() and (wm == 7.0).all() and (gwb == 7.0).all() and (dx == 7.0).all() and loss.item() == 7.0
