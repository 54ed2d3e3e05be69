"""GPU: the kernels of csrc/adv_kernels.hip per element against the float64 restatement (tests/adv_ref.py) on shared,
bf16-representable inputs -- so both sides read the same LeakyReLU signs -- and FCDiscriminator as a whole.  The generic
weight gradient (rgda_conv2d_wgrad_grouped) runs a 4 x 4 / stride 2 filter here for the first time and is checked per
element too.  Every bound comes from tests/golden/adv_tolerances.json (derive_adv_tolerances.py): three times the bf16
storage model's deviation from float64 plus the f32 accumulation floor; none is set by hand.  Each test prints its
figures before it asserts."""
import json
import os

import pytest
import torch

import adv_ref as R

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
BF = torch.bfloat16


@pytest.fixture(scope='module')
def tol():
    return json.load(open(os.path.join(HERE, 'golden', 'adv_tolerances.json')))


@pytest.fixture(scope='module')
def ops():
    from regda_amd import ops
    return ops


def dev_rows(x):
    """float64 (N, C, H, W) with bf16-representable values -> bf16 rows on the device"""
    return R.rows(x).to(BF).cuda()


def operand_copies(ops, w):
    """OIHW float64 (bf16-representable) -> wf bf16 [Co, 16, Ci], wt bf16 [Ci, 16, Co] through rgda_weight_transpose_bf16"""
    Co, Ci = w.shape[:2]
    w32 = w.permute(0, 2, 3, 1).reshape(Co, 16, Ci).float().contiguous().cuda()
    wt = torch.empty((Ci, 16, Co), dtype=BF, device='cuda')
    ops.weight_transpose_bf16(w32, wt, Co, 16, Ci)
    return w32.to(BF), wt


def check(name, got, ref, bound):
    e = R.err(got.detach().cpu(), ref)
    print('[adv %s] err %.3e bound %.3e' % (name, e, bound))
    assert torch.isfinite(got).all(), name
    assert e < bound, (name, e, bound)


_CONV = {}


def conv_run(ops, name):
    """the case, its float64 reference (computed once) and the device operands"""
    if name not in _CONV:
        c = R.conv_case(name)
        _CONV[name] = (c, R.conv_reference(c))
    c, ref = _CONV[name]
    wf, wt = operand_copies(ops, c['w'])
    return c, ref, dev_rows(c['x']), wf, wt, dev_rows(c['g'])


@pytest.mark.parametrize('name', list(R.CONV_CASES))
def test_conv_forward(ops, tol, name):
    c, ref, x, wf, wt, g = conv_run(ops, name)
    y = ops.disc_conv(x, wf, c['b'].float().cuda(), c['N'], c['H'], c['W'])
    check('conv %s y' % name, R.nchw(y.double(), c['N'], c['H'] // 2, c['W'] // 2), ref['y'], tol['conv'][name]['y'])
    # without a bias pointer: the same minus the bias, before the activation
    y0 = ops.disc_conv(x, wf, None, c['N'], c['H'], c['W'])
    ref0 = R.layer(c['x'], c['w'], None)
    check('conv %s y (no bias)' % name, R.nchw(y0.double(), c['N'], c['H'] // 2, c['W'] // 2), ref0,
          3 * R.err(R.bf(ref0), ref0) + 16 * c['Ci'] * R.U32)


@pytest.mark.parametrize('name', [n for n, c in R.CONV_CASES.items() if c[3] % 64 == 0])
def test_conv_forward_generic_route(ops, tol, name):
    """layers 2-4 of the module: rgda_conv2d on the 4 x 4 / stride 2 geometry, then rgda_disc_bias_lrelu in place"""
    c, ref, x, wf, wt, g = conv_run(ops, name)
    y = torch.empty((c['N'] * (c['H'] // 2) * (c['W'] // 2), c['Co']), dtype=BF, device='cuda')
    ops.conv2d(x, wf, y, c['N'], c['H'], c['W'], c['H'] // 2, c['W'] // 2, 4, 4, 2, 1, 1)
    raw = y.clone()
    assert ops.disc_bias_lrelu(y, c['b'].float().cuda()) is y
    check('conv %s y (generic route)' % name, R.nchw(y.double(), c['N'], c['H'] // 2, c['W'] // 2), ref['y'], tol['conv'][name]['y_generic'])
    # the epilogue pass alone, per element on its own input: one bf16 rounding of an f32 add and multiply
    want = torch.nn.functional.leaky_relu(raw.double().cpu() + c['b'], R.SLOPE)
    check('conv %s epilogue pass' % name, y.double(), want, 3 * R.err(R.bf(want), want) + 2 * R.U32)


@pytest.mark.parametrize('name', list(R.CONV_CASES))
def test_conv_data_gradient(ops, tol, name):
    """x holds exact zeros, negative zeros and negatives: all three take the slope"""
    c, ref, x, wf, wt, g = conv_run(ops, name)
    assert (c['x'] == 0).any() and (c['x'] < 0).any() and torch.signbit(c['x'][c['x'] == 0]).any()
    dx, dw, db = ops.disc_conv_backward(g, x, wt, c['N'], c['H'], c['W'], below=True, need_dparams=False)
    assert dw is None and db is None
    check('conv %s dx' % name, R.nchw(dx.double(), c['N'], c['H'], c['W']), ref['dx'], tol['conv'][name]['dx'])
    dx, _, _ = ops.disc_conv_backward(g, x, wt, c['N'], c['H'], c['W'], below=False, need_dparams=False)
    check('conv %s dx (no mask)' % name, R.nchw(dx.double(), c['N'], c['H'], c['W']), ref['dx_plain'], tol['conv'][name]['dx_plain'])


@pytest.mark.parametrize('name', list(R.CONV_CASES))
def test_conv_weight_and_bias_gradient(ops, tol, name):
    c, ref, x, wf, wt, g = conv_run(ops, name)
    _, dw, db = ops.disc_conv_backward(g, x, wt, c['N'], c['H'], c['W'], need_dx=False)
    dw = dw.view(c['Co'], 4, 4, c['Ci']).permute(0, 3, 1, 2)
    check('conv %s dw' % name, dw.double(), ref['dw'], tol['conv'][name]['dw'])
    check('conv %s db' % name, db.double(), ref['db'], tol['conv'][name]['db'])
    _, dw2, db2 = ops.disc_conv_backward(g, x, wt, c['N'], c['H'], c['W'], need_dx=False)
    assert torch.equal(dw2.view(-1), dw.permute(0, 2, 3, 1).reshape(-1)) and torch.equal(db2, db), 'two runs are bit-identical'


@pytest.mark.parametrize('name', list(R.PROBS_CASES))
def test_probabilities(ops, tol, name):
    c = R.probs_case(name)
    ref = R.probs_reference(c)
    x = c['x'].cuda()
    P = ops.adv_probs(x, c['size'], softmax=c['softmax'])
    assert P.shape == (c['b'] * c['H'] * c['W'], 16) and (P[:, c['C']:] == 0).all(), 'the padding channels are zero'
    check('probs %s P' % name, R.nchw(P[:, :c['C']].double(), c['b'], c['H'], c['W']), ref['P'], tol['probs'][name]['P'])
    dP = dev_rows(R.pad_classes(c['dP']))
    base = torch.randn(x.shape, device='cuda')
    dx = base.clone()
    ops.adv_probs_backward(dP, x, dx, c['size'], softmax=c['softmax'], scale=0.5)
    # the gradient is ADDED, times the scale; the bound is relative to the gradient itself
    check('probs %s dx' % name, (dx.double() - base.double()) * 2, ref['dx'], tol['probs'][name]['dx'] + 2 * R.U32 * float(base.abs().max() / ref['dx'].abs().max()))
    dx2 = base.clone()
    ops.adv_probs_backward(dP, x, dx2, c['size'], softmax=c['softmax'], scale=0.5)
    assert torch.equal(dx, dx2)


@pytest.mark.parametrize('name', list(R.HEAD_CASES))
def test_head(ops, tol, name):
    c = R.head_case(name)
    ref = R.head_reference(c)
    N, H, W, C = c['N'], c['H'], c['W'], c['C']
    a = dev_rows(c['a'])
    w = c['w'].permute(0, 2, 3, 1).reshape(16, C).float().contiguous().cuda()
    z = ops.disc_head(a, w, c['b'].float().cuda(), N, H, W)
    check('head %s z' % name, z.double().view(N, 1, H // 2, W // 2), ref['z'], tol['head'][name]['z'])
    dz = c['dz'].float().cuda().view(N, -1).contiguous()
    da, dw, db = ops.disc_head_backward(dz, a, w, N, H, W)
    check('head %s da' % name, R.nchw(da.double(), N, H, W), ref['da'], tol['head'][name]['da'])
    check('head %s dw' % name, dw.double().view(4, 4, C).permute(2, 0, 1).unsqueeze(0), ref['dw'], tol['head'][name]['dw'])
    check('head %s db' % name, db.double(), ref['db'], tol['head'][name]['db'])
    da2, none_w, none_b = ops.disc_head_backward(dz, a, w, N, H, W, need_dparams=False)
    assert none_w is None and none_b is None and torch.equal(da, da2)


@pytest.mark.parametrize('name', list(R.BCE_SIZES))
@pytest.mark.parametrize('label', (0, 1))
def test_bce(ops, tol, name, label):
    z = R.bce_case(name)
    assert z.abs().max() == 40.0
    loss_ref, dz_ref = R.bce(z, label)
    loss, dz = ops.bce_logits(z.cuda(), label, scale=0.5)
    t = tol['bce'][name]
    print('[adv bce %s t=%d] loss %.9g ref %.9g' % (name, label, loss.item(), 0.5 * float(loss_ref)))
    assert torch.isfinite(loss).all() and abs(loss.item() - 0.5 * float(loss_ref)) < t['loss'] * 0.5 * float(loss_ref)
    check('bce %s t=%d dz' % (name, label), dz.double(), 0.5 * dz_ref, t['dz'])
    acc = torch.full((1,), 2.0, device='cuda')
    _, none = ops.bce_logits(z.cuda(), label, scale=0.5, loss=acc, accumulate=True, want_grad=False)
    assert none is None and abs(acc.item() - 2.0 - loss.item()) < 4 * R.U32 * 2.5
    with pytest.raises(ValueError):
        ops.bce_logits(z.cuda(), 0.5)


_MODULE = {}


def module_run(name):
    from regda_amd.models.Discriminator import FCDiscriminator
    if name not in _MODULE:
        c = R.module_case(name)
        _MODULE[name] = (c, {lab: R.module_reference(c, lab) for lab in (0, 1)})
    c, refs = _MODULE[name]
    m = FCDiscriminator(c['C'], ndf=c['ndf'])
    m.load_state_dict(c['sd'])
    return c, refs, m.cuda()


@pytest.mark.parametrize('name', list(R.MODULE_CASES))
def test_module(tol, name):
    """output per element; gradients by relative L2 norm per tensor (a pre-activation within rounding of zero may take the
    other LeakyReLU branch than float64 does); Adam on the module's .grad moves the parameters as it moves the
    restatement's"""
    import torch.nn.functional as F
    c, refs, m = module_run(name)
    for lab in (0, 1):
        ref, t = refs[lab], tol['module'][name][str(lab)]
        m.zero_grad()
        x = c['x'].cuda().requires_grad_(True)
        z = m(x)
        assert z.shape == (c['b'], 1, c['H'] // 32, c['W'] // 32) and z.dtype == torch.float32
        check('module %s t=%d z' % (name, lab), z.double(), ref['z'], t['z'])
        F.binary_cross_entropy_with_logits(z, torch.full_like(z, float(lab))).backward()
        e = R.rel2(x.grad.cpu(), ref['dx'])
        print('[adv module %s t=%d] dx rel2 %.3e bound %.3e' % (name, lab, e, t['dx']))
        assert e < t['dx']
        for k in R.PARAMS:
            g = m.get_parameter(k).grad
            assert g is not None and g.shape == c['sd'][k].shape, k
            e = R.rel2(g.cpu(), ref['grads'][k])
            print('[adv module %s t=%d] %s rel2 %.3e bound %.3e' % (name, lab, k, e, t[k]))
            assert e < t[k], (k, e, t[k])
        if lab == 1:
            before = {k: m.get_parameter(k).detach().clone() for k in R.PARAMS}
            op_before = m.operands()
            torch.optim.Adam(m.parameters(), lr=1e-4, betas=(0.9, 0.99)).step()
            for k in R.PARAMS:
                q = m.get_parameter(k)
                # every element moved by Adam's step for the module's own .grad ...
                assert R.adam_first_step_check(before[k], q, q.grad), k
                # ... and in the restatement's direction, but for the derived number of elements whose gradient the
                # rounding points may push across zero (adv_ref.opposite_bound)
                moved, want = (q.detach() - before[k]).cpu(), -ref['grads'][k]
                n = R.opposite(moved, want)
                print('[adv module %s] adam %s: %d of %d elements move against the restatement, bound %d' % (
                    name, k, n, want.numel(), t['opposite.' + k]))
                assert n <= t['opposite.' + k], (k, n, t['opposite.' + k])
            # the operand copies follow the parameters
            assert m.operands() is not op_before
            with torch.no_grad():
                z2 = m(c['x'].cuda())
            assert not torch.equal(z2, z.detach()) and m.operands() is m.operands()


def test_module_is_deterministic_and_input_only_backward():
    c, refs, m = module_run('ndf32_c6_32x32')
    outs = []
    for _ in range(2):
        m.zero_grad()
        x = c['x'].cuda().requires_grad_(True)
        m(x).sum().backward()
        outs.append([x.grad.clone()] + [p.grad.clone() for p in m.parameters()])
    assert all(torch.equal(a, b) for a, b in zip(*outs))
    for p in m.parameters():
        p.requires_grad_(False)
    x = c['x'].cuda().requires_grad_(True)
    m(x).sum().backward()
    assert torch.equal(x.grad, outs[0][0])
