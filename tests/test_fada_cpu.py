"""CPU: the feature-space adversarial path without a GPU -- the library's new symbols and the module import, the float64
restatement against the goldens minted from the reference's PixelDiscriminator, the state dict, properties of the loss,
every refusal (raised before the GPU is touched), the argument checks of the entry points (which return before any launch)
and the committed tolerance file against what its derive script observes."""
import ctypes
import json
import os
import sys

import pytest
import torch

import fada_ref as R
from regda_amd import _lib

HERE = os.path.dirname(os.path.abspath(__file__))
INT_SYMBOLS = ('rgda_feat_pack_rows', 'rgda_feat_unpack_rows', 'rgda_fada_head', 'rgda_fada_head_bwd_data',
               'rgda_lrelu_mask_rows')
ARG, WS, UNSUP = -1, -2, -4


@pytest.fixture(scope='module')
def tol():
    return json.load(open(os.path.join(HERE, 'golden', 'fada_tolerances.json')))


def test_library_exports_the_symbols_with_plan_ids():
    L = _lib.lib()
    assert L.raw('rgda_abi_version')() == 10
    for name in INT_SYMBOLS + ('rgda_fada_head_workspace',):
        assert name in L.protos and name not in L.missing, name
    for name in INT_SYMBOLS:
        assert L.raw('rgda_plan_fn_id')(name.encode()) >= 0, name
        assert len(L.protos[name][1]) <= 36, name


def test_module_imports_with_the_reference_interface():
    from regda_amd.models.PixelDiscriminator import PixelDiscriminator
    from regda_amd import ops
    m = PixelDiscriminator(2048, num_classes=7)
    assert m.D[0].weight.shape == (512, 2048, 3, 3) and m.D[2].weight.shape == (256, 512, 3, 3)
    assert m.cls1.weight.shape == (7, 256, 3, 3) and m.cls2.bias.shape == (7,)
    assert PixelDiscriminator(64).cls1.weight.shape[0] == 1             # the reference's defaults
    assert all(p.dtype == torch.float32 and isinstance(p, torch.nn.Parameter) for p in m.parameters())
    for f in ('feat_pack_rows', 'feat_unpack_rows', 'fada_head', 'fada_loss', 'fada_head_backward_data', 'lrelu_mask_rows'):
        assert callable(getattr(ops, f))
    import regda_amd.models.Discriminator as D
    assert not hasattr(D, 'PixelDiscriminator')


def test_state_dict_round_trips_with_the_reference(gold):
    from regda_amd.models.PixelDiscriminator import PixelDiscriminator
    keys = [str(k) for k in gold('fada.npz')['keys']]
    m = PixelDiscriminator(R.MODULE_NC, R.MODULE_NDF, 7)
    assert list(m.state_dict().keys()) == keys == list(R.PARAMS)
    sd = R.golden_case(gold, 'nc7_2x8x8')['sd']
    m.load_state_dict(sd, strict=True)
    for k, v in m.state_dict().items():
        assert torch.equal(v, sd[k]) and v.shape == sd[k].shape, k
    with pytest.raises(RuntimeError, match='size mismatch'):
        PixelDiscriminator(R.MODULE_NC, R.MODULE_NDF, 6).load_state_dict(sd)


@pytest.mark.parametrize('name', R.GOLDEN_CASES)
def test_restatement_matches_the_reference(gold, tol, name):
    """float64 against the reference's float32; the bound is three times the float32 formulation's own deviation from
    float64 on the same inputs (derive_fada_tolerances.py); a wrong formula is off by orders of magnitude more"""
    c = R.golden_case(gold, name)
    p = R.params64(c['sd'])
    assert R.err(c['z'], R.disc_forward(p, c['x'])[0]) < tol['golden'][name]['0']['z']
    for s in (0, 1):
        r, t = R.disc_loss_grads(p, c['x'], c['x2'], s), tol['golden'][name][str(s)]
        assert abs(float(c['loss%d' % s]) - float(r['loss'])) < t['loss'] * abs(float(r['loss']))
        assert R.err(c['dx%d' % s], r['dx']) < t['dx'], (name, s)
        for k in R.PARAMS:
            assert R.err(c['g%d' % s][k], r['grads'][k]) < t[k], (name, s, k, R.err(c['g%d' % s][k], r['grads'][k]))


def test_layerwise_backward_is_the_autograd_gradient():
    c = R.module_case('nc7_1x5x7')
    for s in (0, 1):
        a, b = R.module_reference(c, s), R.autograd_reference(c['sd'], c['x'], c['x2'], s)
        assert R.err(a['z'], b['z']) < 1e-13 and R.err(a['dx'], b['dx']) < 1e-12 and abs(float(a['loss'] - b['loss'])) < 1e-13
        for k in R.PARAMS:
            assert R.err(a['grads'][k], b['grads'][k]) < 1e-12, k


def test_properties_of_the_loss():
    gen = torch.Generator().manual_seed(3)
    z = torch.randn(2, 12, 3, 4, generator=gen, dtype=torch.float64)
    x2 = torch.randn(2, 6, 3, 4, generator=gen, dtype=torch.float64)
    for side in (0, 1):
        a = R.soft_labels(x2, 1.8, 1.0)         # no cap: S_p = 1
        assert torch.allclose(a.sum(1), torch.ones(2, 3, 4, dtype=torch.float64))
        loss, dz = R.loss_and_dz(z, a, side)
        assert dz.sum(1).abs().max() < 1e-15                             # rows of dz sum to zero where S_p = 1
        dead = dz[:, (1 - side) * 6:(2 - side) * 6]
        assert torch.allclose(dead, torch.softmax(z, 1)[:, (1 - side) * 6:(2 - side) * 6] / 24)      # the dead half: a' = 0
        zz = z.clone().requires_grad_(True)
        R.loss_and_dz(zz, a, side)[0].backward()
        assert R.err(dz, zz.grad) < 1e-13
    capped = R.soft_labels(x2 * 10, 1.8, 0.9)
    assert capped.max() == 0.9 and capped.sum(1).min() < 1.0             # after the cap S_p may be below 1
    loss, dz = R.loss_and_dz(z, capped, 0)
    assert dz.sum(1).abs().max() < 1e-15             # still zero: S * softmax sums to S, as a' does
    big = torch.full((1, 6, 1, 2), -80.0, dtype=torch.float64)
    big[0, 2] = 80.0
    a = R.soft_labels(big, 1.0, 0.9)
    loss, dz = R.loss_and_dz(torch.randn(1, 12, 1, 2, generator=gen, dtype=torch.float64) * 80, a, 1)
    assert torch.isfinite(a).all() and torch.isfinite(loss) and torch.isfinite(dz).all() and float(a.max()) == 0.9


def test_refusals_need_no_gpu():
    from regda_amd import ops
    from regda_amd.gast.fada import FeatureAdversarialAligner
    from regda_amd.models.PixelDiscriminator import PixelDiscriminator as P
    with pytest.raises(ValueError, match='input channels'):
        P(64, 64, 6)(torch.zeros(2, 128, 4, 4))
    with pytest.raises(ValueError, match='input_nc'):
        P(32, 64, 6)(torch.zeros(2, 32, 4, 4))
    with pytest.raises(ValueError, match='input_nc'):
        P(96, 64, 6)(torch.zeros(2, 96, 4, 4))
    with pytest.raises(ValueError, match='ndf'):
        P(64, 32, 6)(torch.zeros(2, 64, 4, 4))
    with pytest.raises(ValueError, match='ndf'):
        P(64, 192, 6)(torch.zeros(2, 64, 4, 4))
    with pytest.raises(ValueError, match='classes'):
        P(64, 64, 17)(torch.zeros(2, 64, 4, 4))
    with pytest.raises(ValueError, match=r'\(b, C, H, W\)'):
        P(64, 64, 6)(torch.zeros(64, 4, 4))
    with pytest.raises(ValueError, match='f32'):
        P(64, 64, 6)(torch.zeros(2, 64, 4, 4, dtype=torch.float64))
    with pytest.raises(RuntimeError, match='GPU'):                  # a served shape on the CPU: no fallback
        P(64, 64, 6)(torch.zeros(2, 64, 1, 3))
    # ops: shapes and scalars first, then the device
    rows = torch.zeros(8, 32, dtype=torch.bfloat16)
    with pytest.raises(ValueError, match='f32'):
        ops.feat_pack_rows(torch.zeros(2, 32, 2))
    with pytest.raises(RuntimeError, match='GPU'):
        ops.feat_pack_rows(torch.zeros(2, 32, 2, 2))
    with pytest.raises(RuntimeError, match='GPU'):
        ops.feat_unpack_rows(rows, torch.zeros(2, 32, 2, 2))
    with pytest.raises(RuntimeError, match='GPU'):
        ops.lrelu_mask_rows(rows, rows)
    wh, bias, x2 = torch.zeros(32, 9, 32, dtype=torch.bfloat16), torch.zeros(32), torch.zeros(2, 6, 2, 2)
    with pytest.raises(ValueError, match='classes'):
        ops.fada_head(rows, wh, bias, 2, 2, 2, 17)
    with pytest.raises(ValueError, match='classes'):
        ops.fada_loss(rows, wh, bias, torch.zeros(2, 17, 2, 2), 0)
    with pytest.raises(ValueError, match='side'):
        ops.fada_loss(rows, wh, bias, x2, 2)
    with pytest.raises(ValueError, match='temperature'):
        ops.fada_loss(rows, wh, bias, x2, 0, temperature=0.0)
    with pytest.raises(ValueError, match='logits'):
        ops.fada_loss(rows, wh, bias, x2.double(), 0)
    with pytest.raises(RuntimeError, match='GPU'):
        ops.fada_loss(rows, wh, bias, x2, 0)
    with pytest.raises(RuntimeError, match='GPU'):
        ops.fada_head(rows, wh, bias, 2, 2, 2, 6)
    with pytest.raises(RuntimeError, match='GPU'):
        ops.fada_head_backward_data(rows, torch.zeros(32, 9, 32, dtype=torch.bfloat16), rows, 2, 2, 2)
    # the aligner
    with pytest.raises(ValueError, match='no discriminator'):
        FeatureAdversarialAligner(None)
    with pytest.raises(ValueError, match='temperature'):
        FeatureAdversarialAligner(P(64, 64, 6), temperature=0.0)
    with pytest.raises(ValueError, match='clip'):
        FeatureAdversarialAligner(P(64, 64, 6), clip=1.5)
    al = FeatureAdversarialAligner(P(64, 64, 6))
    al.check_served((4, 64, 8, 8), (4, 6, 8, 8))
    with pytest.raises(ValueError, match='num_classes'):
        al.check_served((4, 64, 8, 8), (4, 7, 8, 8))
    with pytest.raises(ValueError, match='pixels'):
        al.check_served((4, 64, 8, 8), (4, 6, 8, 4))
    with pytest.raises(ValueError, match='input channels'):
        al.check_served((4, 2048, 8, 8), (4, 6, 8, 8))
    with pytest.raises(ValueError, match='discriminator'):
        al.check_state_dict({'optimizer': al.optimizer.state_dict()})


def test_source_step_refuses_a_negative_weight_before_the_model_is_touched():
    from regda_amd.source import SourceStep
    with pytest.raises(ValueError, match='fada_weight'):
        SourceStep(None, fada_weight=-1)
    with pytest.raises(ValueError, match='fada_weight'):
        SourceStep(None, fada_weight=float('nan'))


def test_argument_errors_before_any_launch():
    L = _lib.lib()
    p = ctypes.c_void_p(4096)          # non-null, aligned, never dereferenced: every call below returns before a launch
    odd = ctypes.c_void_p(4096 + 2)
    nan = float('nan')

    def pk(x=p, b=2, hw=35, ldc=35, ldb=35 * 32, k=32, rows=p, ld=32):
        return L.raw('rgda_feat_pack_rows')(x, b, hw, ldc, ldb, k, rows, ld, None)

    def up(rows=p, ld=32, dx=p, b=2, hw=35, ldc=35, ldb=35 * 32, k=32, scale=1.0, acc=0):
        return L.raw('rgda_feat_unpack_rows')(rows, ld, dx, b, hw, ldc, ldb, k, scale, acc, None)

    for f in (pk, up):
        for kw in (dict(rows=None), dict(b=0), dict(hw=0), dict(k=0), dict(ld=0), dict(ld=24), dict(ldc=34), dict(ldb=35 * 31),
                   dict(rows=odd)):
            assert f(**kw) == ARG, (f.__name__, kw)
        for kw in (dict(k=30, ld=36), dict(b=1 << 17, ldb=35 * 32), dict(b=1 << 14, hw=1 << 14, ldc=1 << 14, ldb=1 << 19)):
            assert f(**kw) == UNSUP, (f.__name__, kw)
    assert pk(x=None) == ARG and pk(x=odd) == ARG and up(dx=None) == ARG and up(scale=nan) == ARG

    def hd(a=p, wh=p, bias=p, N=2, H=3, W=3, Ch=32, nc=6, z=p, x2=p, side=0, T=1.8, clip=0.9, scale=1.0, loss=p, dz=p, ws=p,
           wsb=1 << 20):
        return L.raw('rgda_fada_head')(a, wh, bias, N, H, W, Ch, nc, z, x2, side, T, clip, scale, loss, dz, ws, wsb, None)

    for kw in (dict(a=None), dict(wh=None), dict(bias=None), dict(N=0), dict(H=0), dict(W=-1), dict(Ch=0), dict(a=odd), dict(wh=odd),
               dict(z=odd), dict(z=None, x2=None), dict(side=2), dict(T=0.0), dict(T=nan), dict(clip=0.0), dict(clip=nan),
               dict(scale=nan), dict(loss=None), dict(dz=None), dict(ws=None), dict(dz=odd)):
        assert hd(**kw) == ARG, kw
    for kw in (dict(Ch=48), dict(nc=0), dict(nc=17), dict(N=1 << 12, H=1 << 10, W=1 << 10)):
        assert hd(**kw) == UNSUP, kw
    assert hd(wsb=0) == WS and hd(x2=None, loss=None, dz=None, ws=None, wsb=0, N=1 << 12, H=1 << 10, W=1 << 10) == UNSUP
    assert L.size('rgda_fada_head_workspace', 128) == 256 and L.size('rgda_fada_head_workspace', 32 * 64 + 1) == 512
    assert L.size('rgda_fada_head_workspace', 0) == 0

    def hb(dz=p, wt=p, below=p, da=p, N=2, H=3, W=3, Ch=64, slope=0.2):
        return L.raw('rgda_fada_head_bwd_data')(dz, wt, below, da, N, H, W, Ch, slope, None)

    for kw in (dict(dz=None), dict(wt=None), dict(below=None), dict(below=odd), dict(da=None), dict(N=0), dict(H=0), dict(W=0), dict(Ch=0), dict(slope=nan), dict(da=odd),
               dict(dz=odd)):
        assert hb(**kw) == ARG, kw
    assert hb(Ch=40) == UNSUP and hb(N=1 << 12, H=1 << 10, W=1 << 10) == UNSUP

    mk = L.raw('rgda_lrelu_mask_rows')
    assert mk(None, p, 64, 64, 0.2, None) == ARG and mk(p, None, 64, 64, 0.2, None) == ARG and mk(p, p, 0, 64, 0.2, None) == ARG
    assert mk(p, p, 64, 0, 0.2, None) == ARG and mk(odd, p, 64, 64, 0.2, None) == ARG and mk(p, p, 64, 64, nan, None) == ARG
    assert mk(p, p, 64, 12, 0.2, None) == UNSUP and mk(p, p, 1 << 24, 1 << 10, 0.2, None) == UNSUP
    with pytest.raises(ValueError):
        L.call('rgda_fada_head_bwd_data', None, None, None, None, 2, 3, 3, 64, 0.2, None)


def test_committed_tolerances_are_what_the_derive_script_observes(tol):
    """every case of the GPU tests has its bounds in the file, and the file is what derive_fada_tolerances.py computes here"""
    sys.path.insert(0, os.path.join(HERE, 'golden'))
    from derive_fada_tolerances import derive
    now = derive()
    assert tol['margin'] == 3.0
    assert set(tol['head']) == {R.head_name(s, ch, nc) for s in R.SHAPES for ch in R.HEAD_CHANNELS for nc in R.CLASS_COUNTS}
    assert set(tol['generic']) == set(R.GENERIC_CASES) and set(tol['module']) == set(R.MODULE_CASES)
    assert set(tol['golden']) == set(R.GOLDEN_CASES)

    def same(a, b, path, rel=1e-3):
        if isinstance(a, dict):
            assert set(a) == set(b), path
            for k in a:
                same(a[k], b[k], path + (k,), rel)
        else:
            assert a == pytest.approx(b, rel=rel), path

    for group in ('head', 'generic'):
        same(tol[group], now[group], (group,))
    for n in R.MODULE_CASES:
        # (a whole-module deviation counts LeakyReLU branches that flip under bf16 rounding: one more or fewer on another
        # machine moves it by percents, not digits)
        same(tol['module'][n], now['module'][n], ('module', n), rel=0.25)
    for n in R.GOLDEN_CASES:           # float32 on this machine may round otherwise than where the file was written:
        for s in ('0', '1'):           # the bounds stay within a factor of three of each other
            for q, v in tol['golden'][n][s].items():
                assert v / 3 < now['golden'][n][s][q] < v * 3, (n, s, q)
