"""CPU: the adversarial path without a GPU -- the library's new symbols and the module import, the float64 restatement
against the goldens minted from the reference's FCDiscriminator, the state dict, every refusal (raised before the GPU is
touched), the argument checks of the entry points (which return before any launch) and the committed tolerance file
against what its derive script observes."""
import ctypes
import json
import os
import sys

import pytest
import torch

import adv_ref as R
from regda_amd import _lib

HERE = os.path.dirname(os.path.abspath(__file__))
INT_SYMBOLS = ('rgda_adv_probs_fwd', 'rgda_adv_probs_bwd', 'rgda_disc_conv_fwd', 'rgda_disc_conv_bwd_data',
               'rgda_disc_bias_lrelu', 'rgda_disc_bias_grad', 'rgda_disc_head_fwd', 'rgda_disc_head_bwd', 'rgda_bce_logits')
ARG, WS, UNSUP = -1, -2, -4


@pytest.fixture(scope='module')
def tol():
    return json.load(open(os.path.join(HERE, 'golden', 'adv_tolerances.json')))


def test_library_exports_the_adversarial_symbols():
    L = _lib.lib()
    assert L.raw('rgda_abi_version')() == 10
    for name in INT_SYMBOLS + ('rgda_disc_bias_grad_workspace',):
        assert name in L.protos and name not in L.missing, name
    for name in INT_SYMBOLS:
        assert L.raw('rgda_plan_fn_id')(name.encode()) >= 0, name


def test_module_imports_with_the_reference_interface():
    from regda_amd.models.Discriminator import FCDiscriminator
    from regda_amd import ops
    m = FCDiscriminator(6)
    assert m.conv1.weight.shape == (64, 6, 4, 4) and m.classifier.weight.shape == (1, 512, 4, 4)
    assert all(p.dtype == torch.float32 and isinstance(p, torch.nn.Parameter) for p in m.parameters())
    for f in ('adv_probs', 'adv_probs_backward', 'disc_conv', 'disc_conv_backward', 'disc_head', 'bce_logits'):
        assert callable(getattr(ops, f))


@pytest.mark.parametrize('name', R.GOLDEN_CASES)
def test_restatement_matches_the_reference(gold, tol, name):
    """float64 against the reference's float32; the bound is three times the float32 formulation's own deviation from
    float64 on the same inputs (derive_adv_tolerances.py); a wrong formula is off by orders of magnitude more"""
    c = R.golden_case(gold, name)
    p = R.params64(c['sd'])
    assert R.err(c['z'], R.disc_forward(p, c['x'])[0]) < tol['golden'][name]['0']['z']
    for lab in (0, 1):
        r, t = R.disc_loss_grads(p, c['x'], lab), tol['golden'][name][str(lab)]
        assert abs(float(c['loss%d' % lab]) - float(r['loss'])) < t['loss'] * abs(float(r['loss']))
        assert R.err(c['dx%d' % lab], r['dx']) < t['dx'], (name, lab)
        for k in R.PARAMS:
            assert R.err(c['g%d' % lab][k], r['grads'][k]) < t[k], (name, lab, k, R.err(c['g%d' % lab][k], r['grads'][k]))


def test_layerwise_backward_is_the_autograd_gradient():
    c = R.module_case('ndf32_c7_32x32')
    for lab in (0, 1):
        a, b = R.module_reference(c, lab), R.autograd_reference(c['sd'], c['x'], lab)
        assert R.err(a['z'], b['z']) < 1e-13 and R.err(a['dx'], b['dx']) < 1e-12
        for k in R.PARAMS:
            assert R.err(a['grads'][k], b['grads'][k]) < 1e-12, k


def test_probabilities_restatement():
    x = torch.randn(2, 6, 2, 3, dtype=torch.float64)
    p = R.probs(x, (8, 9))
    assert p.shape == (2, 6, 8, 9) and torch.allclose(p.sum(1), torch.ones(2, 8, 9, dtype=torch.float64))
    assert torch.allclose(p[..., 0, 0], torch.softmax(x[..., 0, 0], 1)) and torch.allclose(p[..., -1, -1], torch.softmax(x[..., -1, -1], 1))
    assert torch.equal(R.probs(x, softmax=False), x)
    loss, dz = R.bce(torch.tensor([40.0, -40.0, 0.0]), 1)
    ref = torch.nn.functional.binary_cross_entropy_with_logits(torch.tensor([40.0, -40.0, 0.0], dtype=torch.float64),
                                                               torch.ones(3, dtype=torch.float64))
    assert abs(float(loss - ref)) < 1e-14 and torch.isfinite(dz).all()


def test_state_dict_round_trips_with_the_reference(gold):
    from regda_amd.models.Discriminator import FCDiscriminator
    base = gold('adv.npz')
    keys = [str(k) for k in base['keys']]
    m = FCDiscriminator(7, ndf=R.GOLDEN_NDF)
    assert list(m.state_dict().keys()) == keys == list(R.PARAMS)
    sd = R.golden_case(gold, 'c7_32x32')['sd']
    m.load_state_dict(sd, strict=True)
    for k, v in m.state_dict().items():
        assert torch.equal(v, sd[k]) and v.shape == sd[k].shape, k
    with pytest.raises(RuntimeError, match='size mismatch'):
        FCDiscriminator(6, ndf=R.GOLDEN_NDF).load_state_dict(sd)


def test_refusals_need_no_gpu():
    from regda_amd.models.Discriminator import FCDiscriminator
    with pytest.raises(ValueError, match='classes'):
        FCDiscriminator(5)(torch.zeros(2, 5, 32, 32))
    with pytest.raises(ValueError, match='classes'):
        FCDiscriminator(17)(torch.zeros(2, 17, 32, 32))
    with pytest.raises(ValueError, match='input channels'):
        FCDiscriminator(6)(torch.zeros(2, 7, 32, 32))
    with pytest.raises(ValueError, match='ndf'):
        FCDiscriminator(6, ndf=8)(torch.zeros(2, 6, 32, 32))
    with pytest.raises(ValueError, match='% 32'):
        FCDiscriminator(6)(torch.zeros(2, 6, 48, 32))
    with pytest.raises(ValueError, match='% 32'):
        FCDiscriminator(6)(torch.zeros(2, 6, 32, 16))
    with pytest.raises(ValueError, match=r'\(b, C, H, W\)'):
        FCDiscriminator(6)(torch.zeros(6, 32, 32))
    with pytest.raises(ValueError, match='f32'):
        FCDiscriminator(6)(torch.zeros(2, 6, 32, 32, dtype=torch.float64))
    with pytest.raises(RuntimeError, match='GPU'):                  # a served shape on the CPU: no fallback
        FCDiscriminator(6)(torch.zeros(2, 6, 32, 32))
    import regda_amd.models.Discriminator as D
    assert not hasattr(D, 'FCDiscriminator_Local') and not hasattr(D, 'PixelDiscriminator')


def test_argument_errors_before_any_launch():
    L = _lib.lib()
    p = ctypes.c_void_p(4096)          # non-null, aligned, never dereferenced: every call below returns before a launch
    odd = ctypes.c_void_p(4096 + 2)

    def pf(x=p, P=p, b=2, C=6, h=2, w=2, H=32, W=32, Cp=16, mode=0):
        return L.raw('rgda_adv_probs_fwd')(x, P, b, C, h, w, H, W, Cp, mode, None)

    def pb(dP=p, x=p, dx=p, b=2, C=6, h=2, w=2, H=32, W=32, Cp=16, mode=0, scale=1.0):
        return L.raw('rgda_adv_probs_bwd')(dP, x, dx, b, C, h, w, H, W, Cp, mode, scale, None)

    for kw in (dict(x=None), dict(P=None), dict(b=0), dict(h=0), dict(W=0), dict(mode=2), dict(mode=1), dict(P=odd)):
        assert pf(**kw) == ARG, kw
    for kw in (dict(C=5), dict(C=17), dict(Cp=32), dict(b=1 << 10, H=1 << 10, W=1 << 10)):
        assert pf(**kw) == UNSUP, kw
    for kw in (dict(dP=None), dict(dx=None), dict(x=None), dict(scale=float('nan')), dict(mode=1), dict(dP=odd)):
        assert pb(**kw) == ARG, kw
    assert pb(C=5) == UNSUP and pb(Cp=32) == UNSUP

    def cf(x=p, w=p, bias=p, y=p, N=2, H=8, W=8, Cin=64, Cout=64, slope=0.2):
        return L.raw('rgda_disc_conv_fwd')(x, w, bias, y, N, H, W, Cin, Cout, slope, None)

    def cb(dy=p, wt=p, below=p, dx=p, N=2, H=8, W=8, Cin=64, Cout=64, slope=0.2):
        return L.raw('rgda_disc_conv_bwd_data')(dy, wt, below, dx, N, H, W, Cin, Cout, slope, None)

    for f in (cf, cb):
        for kw in (dict(N=0), dict(H=0), dict(H=7), dict(W=9), dict(Cin=0), dict(slope=float('nan'))):
            assert f(**kw) == ARG, (f.__name__, kw)
        for kw in (dict(Cin=8), dict(Cin=48), dict(Cout=16), dict(Cout=72), dict(N=1 << 12, H=1 << 10, W=1 << 10)):
            assert f(**kw) == UNSUP, (f.__name__, kw)
    assert cf(x=None) == ARG and cf(w=None) == ARG and cf(y=None) == ARG and cf(x=odd) == ARG
    assert cb(dy=None) == ARG and cb(wt=None) == ARG and cb(dx=None) == ARG

    bg = L.raw('rgda_disc_bias_grad')
    assert L.size('rgda_disc_bias_grad_workspace', 4096, 64) == 2 * 64 * 4 and L.size('rgda_disc_bias_grad_workspace', 45, 128) == 512
    assert L.size('rgda_disc_bias_grad_workspace', 0, 64) == 0 and L.size('rgda_disc_bias_grad_workspace', 64, 48) == 0
    assert bg(None, 64, 64, p, p, 1 << 20, None) == ARG and bg(p, 0, 64, p, p, 1 << 20, None) == ARG
    assert bg(p, 64, 64, p, None, 1 << 20, None) == ARG and bg(p, 64, 48, p, p, 1 << 20, None) == UNSUP
    assert bg(p, 4096, 64, p, p, 64, None) == WS

    bl = L.raw('rgda_disc_bias_lrelu')
    assert bl(None, p, 64, 64, 0.2, None) == ARG and bl(p, None, 64, 64, 0.2, None) == ARG and bl(p, p, 0, 64, 0.2, None) == ARG
    assert bl(odd, p, 64, 64, 0.2, None) == ARG and bl(p, p, 64, 48, 0.2, None) == UNSUP

    def hf(a=p, w=p, bias=p, z=p, N=2, H=2, W=2, C=512):
        return L.raw('rgda_disc_head_fwd')(a, w, bias, z, N, H, W, C, None)

    def hb(dz=p, a=p, w=p, da=p, dw=p, db=p, N=2, H=2, W=2, C=512, slope=0.2):
        return L.raw('rgda_disc_head_bwd')(dz, a, w, da, dw, db, N, H, W, C, slope, None)

    for kw in (dict(a=None), dict(w=None), dict(z=None), dict(N=0), dict(H=3), dict(W=0)):
        assert hf(**kw) == ARG, kw
    assert hf(C=100) == UNSUP
    for kw in (dict(dz=None), dict(a=None), dict(da=None, dw=None, db=None), dict(dw=None), dict(db=None), dict(H=5)):
        assert hb(**kw) == ARG, kw
    assert hb(C=100) == UNSUP
    bce = L.raw('rgda_bce_logits')
    assert bce(None, 4, 0.0, 1.0, p, 0, p, None) == ARG and bce(p, 0, 0.0, 1.0, p, 0, p, None) == ARG
    assert bce(p, 4, 0.5, 1.0, p, 0, p, None) == ARG and bce(p, 4, 1.0, 1.0, None, 0, p, None) == ARG
    with pytest.raises(ValueError):
        L.call('rgda_disc_conv_fwd', None, None, None, None, 2, 8, 8, 64, 64, 0.2, None)


def test_committed_tolerances_are_what_the_derive_script_observes(tol):
    """every case of the GPU tests has its bounds in the file, and the file is what derive_adv_tolerances.py computes here
    (float64 on the CPU: another machine's summation order moves a bound in its last digits, far below 1e-3 of it)"""
    sys.path.insert(0, os.path.join(HERE, 'golden'))
    from derive_adv_tolerances import derive
    now = derive()
    assert tol['margin'] == 3.0
    assert set(tol['conv']) == set(R.CONV_CASES) and set(tol['probs']) == set(R.PROBS_CASES) and set(tol['head']) == set(R.HEAD_CASES)
    assert set(tol['bce']) == set(R.BCE_SIZES) and set(tol['module']) == set(R.MODULE_CASES) and set(tol['golden']) == set(R.GOLDEN_CASES)

    def same(a, b, path, rel=1e-3):
        if isinstance(a, dict):
            assert set(a) == set(b), path
            for k in a:
                same(a[k], b[k], path + (k,), rel)
        else:
            assert a == pytest.approx(b, rel=rel), path

    for group in ('conv', 'probs', 'head', 'bce'):
        same(tol[group], now[group], (group,))
    for n in R.MODULE_CASES:
        # (a whole-module deviation counts LeakyReLU branches that flip under bf16 rounding: one more or fewer on another
        # machine moves it by percents, not digits)
        same(tol['module'][n], now['module'][n], ('module', n), rel=0.25)
    for n in R.GOLDEN_CASES:           # float32 on this machine may round otherwise than where the file was written:
        for lab in ('0', '1'):         # the bounds stay within a factor of three of each other
            for q, v in tol['golden'][n][lab].items():
                assert v / 3 < now['golden'][n][lab][q] < v * 3, (n, lab, q)


def test_adam_first_step_check_holds_for_torch_adam():
    """the movement checks of the GPU tests against torch.optim.Adam itself in float32: they hold for the gradient the
    step was made from, and see a flipped gradient, a permuted one and a handful of flipped elements"""
    gen = torch.Generator().manual_seed(5)
    p = torch.nn.Parameter(torch.randn(4096, generator=gen) * 0.05)
    g = torch.randn(4096, generator=gen) * 10 ** torch.empty(4096).uniform_(-9, 0, generator=gen)
    before = p.detach().clone()
    p.grad = g.clone()
    torch.optim.Adam([p], lr=1e-4, betas=(0.9, 0.99)).step()
    assert R.adam_first_step_check(before, p, g)
    assert not R.adam_first_step_check(before, p, -g) and not R.adam_first_step_check(before, p, g.flip(0))
    few = g.clone()
    few[:5] = -few[:5]
    assert not R.adam_first_step_check(before, p, few)
    moved = p.detach() - before
    assert R.opposite(moved, -g.double()) == 0 and R.opposite(moved, g.double()) == 4096 and R.opposite(moved, -few.double()) == 5
    assert 1500 < R.opposite(moved, -g.flip(0).double()) < 2600          # an unrelated gradient: about half
    # the bound: three times (the model's own count + 1); a single value must agree
    assert R.opposite_bound(few.double(), g.double()) == 18 and R.opposite_bound(g.double(), g.double()) == 3
    assert R.opposite_bound(torch.tensor([1.0]), torch.tensor([-1.0])) == 0
