"""GPU: the kernels of the feature-space adversarial path per element against the float64 restatement (tests/fada_ref.py)
at the smallest shapes at which they can go wrong -- one pixel, 35 rows (no multiple of the 32-pixel tile), 128 rows whose
tiles cross an image boundary, a border-dominated 3 x 33 map in three workgroups -- the generic 3 x 3 routes the
discriminator relies on at the same shapes, and the module.  Bounds: tests/golden/fada_tolerances.json
(derive_fada_tolerances.py); pack / unpack and the mask pass are bit-exact."""
import functools
import json
import os

import pytest
import torch

import fada_ref as R

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
BF = torch.bfloat16


@pytest.fixture(scope='module')
def tol():
    return json.load(open(os.path.join(HERE, 'golden', 'fada_tolerances.json')))


def dev_rows(x, cols=None):
    """float64 (b, C, H, W) -> bf16 rows on the GPU, zero-padded to `cols` columns"""
    r = R.rows(x).to(BF)
    if cols is not None and cols > r.shape[1]:
        r = torch.cat((r, torch.zeros(r.shape[0], cols - r.shape[1], dtype=BF)), 1)
    return r.contiguous().cuda()


def taps_last(w, rows=None):
    """OIHW float64 -> f32 [rows, 9, I] on the GPU, zero rows beyond O"""
    t = w.permute(0, 2, 3, 1).reshape(w.shape[0], 9, w.shape[1]).float()
    if rows is not None and rows > t.shape[0]:
        t = torch.cat((t, torch.zeros(rows - t.shape[0], 9, t.shape[2])), 0)
    return t.contiguous().cuda()


def transposed(w32):
    from regda_amd import ops
    Co, T, Ci = w32.shape
    wt = torch.empty((Ci, T, Co), dtype=BF, device='cuda')
    ops.weight_transpose_bf16(w32, wt, Co, T, Ci)
    return wt


def back(rows, b, H, W, cols=None):
    """GPU rows -> float64 (b, cols, H, W) on the CPU"""
    r = rows.detach().cpu().to(R.F64)
    return R.nchw(r if cols is None else r[:, :cols], b, H, W)


@functools.lru_cache(maxsize=None)
def head(shape, Ch, nc):
    c = R.head_case(shape, Ch, nc)
    return c, R.head_reference(c)


def head_operands(c):
    w32 = taps_last(c['w'], R.CP)
    bias = torch.zeros(R.CP)
    bias[:2 * c['nc']] = c['bias'].float()
    return dev_rows(c['a']), w32.to(BF), w32, bias.cuda()


# ------------------------------------------------------------------------------------------------ pack / unpack
@pytest.mark.parametrize('name', list(R.PACK_CASES))
def test_pack_and_unpack_are_bit_exact(name):
    from regda_amd import ops
    base, idx = R.pack_case(name)
    dev = base.cuda()
    view = dev[idx]
    want = R.rows(base[idx]).to(BF)           # torch's f32 -> bf16 cast rounds to nearest even
    got = ops.feat_pack_rows(view)
    assert torch.equal(got.cpu(), want)
    wide = torch.full((want.shape[0], want.shape[1] + 8), 3.0, dtype=BF, device='cuda')
    ops.feat_pack_rows(view, out=wide)
    assert torch.equal(wide[:, :want.shape[1]].cpu(), want) and bool((wide[:, want.shape[1]:] == 3.0).all())
    b, k, h, w = view.shape
    vals = R.nchw(want.float(), b, h, w)
    for accumulate in (False, True):
        target = torch.randn(base.shape, generator=torch.Generator().manual_seed(9)).cuda()
        old = target.cpu().clone()
        ops.feat_unpack_rows(got, target[idx], scale=0.3, accumulate=accumulate)
        expect = old.clone()
        upd = torch.tensor(0.3, dtype=torch.float32) * vals
        expect[idx] = old[idx] + upd if accumulate else upd
        assert torch.equal(target.cpu(), expect), (name, accumulate)          # and nothing outside the view moved


# ------------------------------------------------------------------------------------------------ the heads
@pytest.mark.parametrize('Ch', R.HEAD_CHANNELS)
@pytest.mark.parametrize('shape', list(R.SHAPES))
def test_head_forward(tol, shape, Ch):
    from regda_amd import ops
    for nc in R.CLASS_COUNTS:
        c, ref = head(shape, Ch, nc)
        a, wh, _, bias = head_operands(c)
        z = ops.fada_head(a, wh, bias, c['b'], c['H'], c['W'], nc)
        e, bound = R.err(back(z, c['b'], c['H'], c['W'], 2 * nc), ref['z']), tol['head'][R.head_name(shape, Ch, nc)]['z']
        print('[fada head %s ch%d nc%d] z err %.3e bound %.3e' % (shape, Ch, nc, e, bound))
        assert e < bound
        assert bool((z[:, 2 * nc:] == 0).all())


@pytest.mark.parametrize('Ch', R.HEAD_CHANNELS)
@pytest.mark.parametrize('shape', list(R.SHAPES))
def test_fused_loss(tol, shape, Ch):
    from regda_amd import ops
    for nc in R.CLASS_COUNTS:
        c, ref = head(shape, Ch, nc)
        a, wh, _, bias = head_operands(c)
        t = tol['head'][R.head_name(shape, Ch, nc)]
        x2 = c['x2'].cuda()
        for s in R.LOSS_SETTINGS:
            side, T, clip = s
            loss, dz, z = ops.fada_loss(a, wh, bias, x2, side, T, clip, scale=0.5, want_z=(side == 0))
            first = loss.clone()
            ops.fada_loss(a, wh, bias, x2, side, T, clip, scale=0.5, loss=loss)        # accumulates onto the same word
            want = float(ref[('loss',) + s])
            e_l = abs(2 * first.item() - want)
            e_dz = R.err(2 * back(dz, c['b'], c['H'], c['W'], 2 * nc), ref[('dz',) + s])
            print('[fada loss %s ch%d nc%d side %d T %g clip %g] loss %.7g ref %.7g (+- %.2e)  dz err %.3e bound %.3e' % (
                shape, Ch, nc, side, T, clip, 2 * first.item(), want, t['loss_%d_%g_%g' % s], e_dz, t['dz_%d_%g_%g' % s]))
            assert e_l < t['loss_%d_%g_%g' % s] and e_dz < t['dz_%d_%g_%g' % s]
            assert loss.item() == 2 * first.item() and torch.isfinite(dz.float()).all()
            assert bool((dz[:, 2 * nc:] == 0).all())
            if z is not None:
                assert R.err(back(z, c['b'], c['H'], c['W'], 2 * nc), ref['z']) < t['z']


@pytest.mark.parametrize('Ch', R.HEAD_CHANNELS)
@pytest.mark.parametrize('shape', list(R.SHAPES))
def test_head_backward(tol, shape, Ch):
    """the data gradient with the mask fused (activations exactly zero and negative zero take the slope) and the parameter
    gradients on the generic weight-gradient and bias-sum routes with 32 columns"""
    from regda_amd import ops
    for nc in R.CLASS_COUNTS:
        c, ref = head(shape, Ch, nc)
        a, _, w32, _ = head_operands(c)
        t = tol['head'][R.head_name(shape, Ch, nc)]
        b, H, W = c['b'], c['H'], c['W']
        dz = dev_rows(c['dz'], R.CP)
        wt = transposed(w32)
        da = ops.fada_head_backward_data(dz, wt, a, b, H, W)
        e = R.err(back(da, b, H, W), ref['da'])
        dw = torch.zeros((R.CP, 9, Ch), dtype=torch.float32, device='cuda')
        ops.conv2d_wgrad_grouped([(a, dz, dw, b, H, W, H, W, 3, 3, 1, 1, 1)])
        db = ops.disc_bias_grad(dz)
        dw_ref = ref['dw'].permute(0, 2, 3, 1).reshape(2 * nc, 9, Ch)
        e_w, e_b = R.err(dw[:2 * nc].cpu(), dw_ref), R.err(db[:2 * nc].cpu(), ref['db'])
        print('[fada head bwd %s ch%d nc%d] da %.3e (%.3e) dw %.3e (%.3e) db %.3e (%.3e)' % (
            shape, Ch, nc, e, t['da'], e_w, t['dw'], e_b, t['db']))
        assert e < t['da'] and e_w < t['dw'] and e_b < t['db']
        assert bool((dw[2 * nc:] == 0).all()) and bool((db[2 * nc:] == 0).all())


@pytest.mark.parametrize('shape', list(R.SHAPES))
def test_mask_pass_is_bit_exact(shape):
    from regda_amd import ops
    c, _ = head(shape, 256, 6)
    gen = torch.Generator().manual_seed(12)
    a = dev_rows(c['a'])
    g = (torch.randn(a.shape, generator=gen)).to(BF).cuda()
    want = (g.float() * torch.where(a.float() > 0, 1.0, 0.2).float()).to(BF)         # zero and negative zero: the slope
    got = ops.lrelu_mask_rows(g.clone(), a)
    assert torch.equal(got, want)
    zero = a.float() == 0
    assert bool(zero.any()) and torch.equal(got[zero].float(), (g[zero].float() * 0.2).to(BF).float())


# ------------------------------------------------------------------------------------------------ the generic routes
@pytest.mark.parametrize('name', list(R.GENERIC_CASES))
def test_generic_routes_on_the_3x3_geometry(tol, name):
    """rgda_conv2d mode 0 + rgda_disc_bias_lrelu, mode 1 on the transposed operand (alone and added onto non-zero rows
    through res=, res and y being the same rows), rgda_conv2d_wgrad_grouped and rgda_disc_bias_grad"""
    from regda_amd import ops
    c = R.generic_case(name)
    ref, t = R.generic_reference(c), tol['generic'][name]
    b, H, W, Ci, Co = c['b'], c['H'], c['W'], c['Ci'], c['Co']
    M = b * H * W
    x, g, w32 = dev_rows(c['x']), dev_rows(c['g']), taps_last(c['w'])
    y = torch.empty((M, Co), dtype=BF, device='cuda')
    ops.conv2d(x, w32.to(BF), y, b, H, W, H, W, 3, 3, 1, 1, 1)
    ops.disc_bias_lrelu(y, c['bias'].float().cuda())
    wt = transposed(w32)
    dx = torch.empty((M, Ci), dtype=BF, device='cuda')
    ops.conv2d(g, wt, dx, b, H, W, H, W, 3, 3, 1, 1, 1, mode=1)
    onto = x.clone()
    ops.conv2d(g, wt, onto, b, H, W, H, W, 3, 3, 1, 1, 1, mode=1, res=onto)
    dw = torch.zeros((Co, 9, Ci), dtype=torch.float32, device='cuda')
    ops.conv2d_wgrad_grouped([(x, g, dw, b, H, W, H, W, 3, 3, 1, 1, 1)])
    db = ops.disc_bias_grad(g)
    errs = dict(y=R.err(back(y, b, H, W), ref['y']), dx=R.err(back(dx, b, H, W), ref['dx']),
                dx_onto=R.err(back(onto, b, H, W), ref['dx_onto']),
                dw=R.err(dw.cpu(), ref['dw'].permute(0, 2, 3, 1).reshape(Co, 9, Ci)), db=R.err(db.cpu(), ref['db']))
    print('[fada generic %s]' % name, {k: '%.3e (%.3e)' % (v, t[k]) for k, v in errs.items()})
    for k, v in errs.items():
        assert v < t[k], (name, k, v, t[k])


# ------------------------------------------------------------------------------------------------ the module
def run_module(c, side):
    from regda_amd.models.PixelDiscriminator import PixelDiscriminator
    m = PixelDiscriminator(R.MODULE_NC, R.MODULE_NDF, c['nc']).cuda()
    m.load_state_dict(c['sd'], strict=True)
    x = c['x'].cuda().requires_grad_(True)
    z = m(x)
    a = torch.softmax(c['x2'].cuda() / R.T_DEFAULT, 1).clamp(max=R.CLIP_DEFAULT)
    nc = c['nc']
    loss = -(a * torch.log_softmax(z, 1)[:, side * nc:(side + 1) * nc]).sum() / (z.shape[0] * z.shape[2] * z.shape[3])
    loss.backward()
    return m, x, z, loss


@pytest.mark.parametrize('name', list(R.MODULE_CASES))
def test_module_forward_backward_and_adam(tol, name):
    c = R.module_case(name)
    for side in (0, 1):
        t, ref = tol['module'][name][str(side)], R.module_reference(c, side)
        m, x, z, loss = run_module(c, side)
        assert z.shape == (c['b'], 2 * c['nc'], c['H'], c['W']) and z.dtype == torch.float32
        errs = dict(z=R.err(z.detach().cpu(), ref['z']), dx=R.rel2(x.grad.cpu(), ref['dx']),
                    loss=abs(loss.item() - float(ref['loss'])) / abs(float(ref['loss'])))
        errs.update({k: R.rel2(m.get_parameter(k).grad.cpu(), ref['grads'][k]) for k in R.PARAMS})
        print('[fada module %s side %d]' % (name, side), {k: '%.3e (%.3e)' % (v, t[k]) for k, v in errs.items()})
        for k, v in errs.items():
            assert v < t[k], (name, side, k, v, t[k])
        m2, x2, z2, loss2 = run_module(c, side)                   # two runs are bit-identical
        assert torch.equal(z, z2) and torch.equal(x.grad, x2.grad) and torch.equal(loss, loss2)
        for k in R.PARAMS:
            assert torch.equal(m.get_parameter(k).grad, m2.get_parameter(k).grad), k
        before = {k: m.get_parameter(k).detach().cpu().clone() for k in R.PARAMS}
        torch.optim.Adam(m.parameters(), lr=1e-4, betas=(0.9, 0.99)).step()
        op_before = m._op
        assert m.operands() is not op_before                      # the bf16 copies follow the parameters' versions
        for k in R.PARAMS:
            q = m.get_parameter(k)
            assert R.adam_first_step_check(before[k], q, q.grad), (name, side, k)
            n = R.opposite(q.detach().cpu() - before[k], -ref['grads'][k])
            assert n <= t['opposite.' + k], (name, side, k, n, t['opposite.' + k])
