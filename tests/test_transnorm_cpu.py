"""CPU: TransNorm without a GPU -- the float64 restatement against the goldens minted from the reference, the module's
parameters, buffers and both checkpoint-loading paths, every refusal of the module, and the argument checks of
rgda_transnorm_fwd / rgda_transnorm_bwd (which return before anything is launched)."""
import ctypes

import pytest
import torch

import transnorm_ref as R
from regda_amd import _lib
from regda_amd.trans_norm import TransNorm1d, TransNorm2d, _TransNorm

KEYS = ['weight', 'bias', 'running_mean_source', 'running_mean_target', 'running_var_source', 'running_var_target',
        'num_batches_tracked']


@pytest.fixture(scope='module')
def g(gold):
    return gold('transnorm.npz')


@pytest.mark.parametrize('name', R.GOLDEN_CASES)
def test_restatement_matches_the_reference(g, name):
    """float64 against the reference's float32: the bound is a few fp32 roundings of the reference's own (its deviation
    from float64 is what derive_transnorm_tolerances.py records: at most 2.4e-6, in `shift`); a wrong formula is off by
    orders of magnitude more"""
    c = R.golden_case(g, name)
    s1, run, ev = R.golden_steps(c)
    tol = 1e-5 if name == 'shift' else 2e-6
    for q in ('y', 'dx', 'dweight', 'dbias'):
        assert R.rel(c[q], s1[q]) < tol, (name, q, R.rel(c[q], s1[q]))
    for q, r in zip(('rm_s', 'rv_s', 'rm_t', 'rv_t'), run):
        assert R.rel(c[q], r) < tol, (name, q)
    assert R.rel(c['y_eval'], ev['y']) < tol
    if name == 'one':
        assert s1['alpha'].tolist() == [1.0] and s1['dis'].shape == (1,)


def test_restatement_gradient_is_the_autograd_gradient():
    """the backward formulae of the contract against autograd through the forward formulae (alpha detached)"""
    gen = torch.Generator().manual_seed(3)
    x = torch.randn(5, 4, 3, 2, generator=gen, dtype=torch.float64, requires_grad=True)
    w = torch.rand(4, generator=gen, dtype=torch.float64).add(0.5).requires_grad_(True)
    b = torch.randn(4, generator=gen, dtype=torch.float64, requires_grad=True)
    gy = torch.randn(5, 4, 3, 2, generator=gen, dtype=torch.float64)
    r = R.transnorm_train(x.detach(), w.detach(), b.detach(), None, 1e-5, 0.1, gy)
    halves = []
    for h in (x[:2], x[2:]):
        m, v = h.mean((0, 2, 3), keepdim=True), h.var((0, 2, 3), unbiased=False, keepdim=True)
        halves.append((h - m) / (v + 1e-5).sqrt())
    y = (torch.cat(halves) * w.view(1, 4, 1, 1) + b.view(1, 4, 1, 1)) * (1 + r['alpha']).view(1, 4, 1, 1)
    y.backward(gy)
    assert torch.allclose(y.detach(), r['y'], rtol=1e-12, atol=1e-12)
    for got, ref in ((r['dx'], x.grad), (r['dweight'], w.grad), (r['dbias'], b.grad)):
        assert torch.allclose(got, ref, rtol=1e-10, atol=1e-12)


def test_module_state_matches_the_reference(g):
    m = TransNorm2d(5)
    assert list(m.state_dict().keys()) == [str(k) for k in g['keys']] == KEYS
    assert [n for n, _ in m.named_parameters()] == ['weight', 'bias']
    assert int(m.num_batches_tracked) == 0 and m.num_batches_tracked.dtype == torch.int64
    assert repr(m) == 'TransNorm2d(5, eps=1e-05, momentum=0.1, affine=True, track_running_stats=True)'
    p = TransNorm1d(3, eps=1e-3, momentum=0.5, affine=False, track_running_stats=False)
    assert list(p.state_dict().keys()) == [] and p.weight is None and p.running_mean_source is None
    assert issubclass(TransNorm1d, _TransNorm) and issubclass(TransNorm2d, torch.nn.Module)
    import regda_amd.trans_norm as T
    assert not hasattr(T, 'TransNorm3d')


def test_loading_a_batchnorm_checkpoint_fills_both_domains(g):
    bn = {k[len('pretrained_bn_'):]: torch.from_numpy(g[k]) for k in g.files if k.startswith('pretrained_bn_')}
    want = {k[len('pretrained_tn_'):]: torch.from_numpy(g[k]) for k in g.files if k.startswith('pretrained_tn_')}
    assert 'running_mean' in bn and 'running_mean_source' not in bn
    m = TransNorm2d(5)
    m.load_state_dict(bn)
    got = m.state_dict()
    assert list(got.keys()) == list(want.keys())
    for k in want:
        assert torch.equal(got[k], want[k]), k
    assert torch.equal(got['running_var_source'], bn['running_var']) and torch.equal(got['running_mean_target'], bn['running_mean'])
    # under a prefix, as a submodule loads it
    net = torch.nn.Sequential(torch.nn.Identity(), TransNorm2d(5))
    net.load_state_dict({'1.' + k: v for k, v in bn.items()})
    assert torch.equal(net[1].running_var_target, bn['running_var'])
    # a checkpoint without num_batches_tracked loads too; a wrong size is reported
    m2 = TransNorm2d(5)
    m2.load_state_dict({k: v for k, v in bn.items() if k != 'num_batches_tracked'})
    assert int(m2.num_batches_tracked) == 0
    with pytest.raises(RuntimeError, match='size mismatch'):
        TransNorm2d(4).load_state_dict(bn)
    with pytest.raises(RuntimeError, match='Missing'):
        TransNorm2d(5).load_state_dict({k: v for k, v in bn.items() if k != 'running_var'})


def test_loading_a_transnorm_checkpoint_is_key_for_key(g):
    want = {k[len('pretrained_tn_'):]: torch.from_numpy(g[k]).clone() for k in g.files if k.startswith('pretrained_tn_')}
    want['running_mean_target'] += 1.0            # the domains differ, so a mix-up shows
    want['running_var_source'] *= 3.0
    m = TransNorm2d(5)
    m.load_state_dict(want)
    for k, v in m.state_dict().items():
        assert torch.equal(v, want[k]), k
    with pytest.raises(RuntimeError, match='Missing'):
        TransNorm2d(5).load_state_dict({k: v for k, v in want.items() if k != 'running_var_target'})


def test_reset_parameters_ranges():
    torch.manual_seed(0)
    m = TransNorm1d(4096)
    w = m.weight.detach()
    assert 0.0 <= w.min() and w.max() < 1.0 and 0.45 < w.mean() < 0.55 and w.std() > 0.25      # U[0, 1), not ones
    assert (m.bias == 0).all()
    with torch.no_grad():
        m.running_mean_target.fill_(3.0)
        m.running_var_source.fill_(3.0)
    m.reset_parameters()
    assert (m.running_mean_target == 0).all() and (m.running_var_source == 1).all() and (m.bias == 0).all()


def test_refusals_need_no_gpu():
    with pytest.raises(ValueError, match='momentum'):
        TransNorm2d(4, momentum=None)
    with pytest.raises(ValueError, match='per'):
        TransNorm1d(4)(torch.zeros(4, 4, 3))                       # 3-D: the reference's per-position alpha
    with pytest.raises(ValueError, match='2D'):
        TransNorm1d(4)(torch.zeros(4, 4, 3, 3))
    with pytest.raises(ValueError, match='4D'):
        TransNorm2d(4)(torch.zeros(4, 4, 3))
    with pytest.raises(ValueError, match='4D'):
        TransNorm2d(4)(torch.zeros(2, 4, 3, 3, 3))                  # 5-D: no TransNorm3d
    with pytest.raises(ValueError, match='channels'):
        TransNorm2d(4)(torch.zeros(4, 5, 3, 3))
    with pytest.raises(ValueError, match='fewer than two'):
        TransNorm2d(4)(torch.zeros(1, 4, 3, 3))                     # an empty source half
    with pytest.raises(ValueError, match='fewer than two'):
        TransNorm1d(4)(torch.zeros(3, 4))                           # one source row
    with pytest.raises(ValueError, match='fewer than two'):
        TransNorm2d(4)(torch.zeros(2, 4, 1, 1))
    m = TransNorm2d(4, track_running_stats=False).eval()
    with pytest.raises(RuntimeError, match='track_running_stats'):
        m(torch.zeros(4, 4, 3, 3))
    with pytest.raises(RuntimeError, match='GPU'):                  # a served shape on the CPU: no fallback
        TransNorm2d(4)(torch.zeros(4, 4, 3, 3))


def test_abi_symbols_and_workspace_queries():
    L = _lib.lib()
    assert L.raw('rgda_abi_version')() == 10
    for name in ('rgda_transnorm_fwd', 'rgda_transnorm_bwd', 'rgda_transnorm_fwd_workspace', 'rgda_transnorm_bwd_workspace'):
        assert name in L.protos and name not in L.missing, name
    for name in ('rgda_transnorm_fwd', 'rgda_transnorm_bwd'):
        assert L.raw('rgda_plan_fn_id')(name.encode()) >= 0
    a = lambda x: (x + 255) // 256 * 256        # noqa: E731
    for q in ('rgda_transnorm_fwd_workspace', 'rgda_transnorm_bwd_workspace'):
        assert L.size(q, 8, 4, 2048, 1024, 1) > 0 and L.size(q, 16, 8, 2048, 1, 1) > 0
        assert L.size(q, 1, 0, 8, 16, 1) == 0          # an empty source half
        assert L.size(q, 2, 1, 8, 1, 1) == 0           # one value per half
        assert L.size(q, 4, 4, 8, 16, 1) == 0          # an empty target half
        assert L.size(q, 4, 2, 0, 16, 1) == 0 and L.size(q, 4, 2, 8, 0, 1) == 0 and L.size(q, 0, 0, 8, 16, 1) == 0
        assert L.size(q, 4, 2, (1 << 20) + 1, 16, 1) == 0 and L.size(q, 1 << 16, 1 << 15, 8, 1 << 15, 1) == 0
        assert L.size(q, 1, 0, 8, 16, 0) > 0           # eval serves one sample
    # records: double [C][2][K][3] forward, double [C][2][K][2] + f32 [6][C] backward, with the same K
    f, b = L.size('rgda_transnorm_fwd_workspace', 8, 4, 2048, 1024, 1), L.size('rgda_transnorm_bwd_workspace', 8, 4, 2048, 1024, 1)
    K = f // (2048 * 2 * 3 * 8)
    assert 1 <= K <= 64 and f == a(2048 * 2 * K * 24) and b == a(2048 * 2 * K * 16) + a(6 * 2048 * 4)


def test_argument_errors_before_any_launch():
    L = _lib.lib()
    p = ctypes.c_void_p(4096)          # a non-null, 256-byte aligned pointer that is never dereferenced: every call below
    big = 1 << 30                      # returns before a launch

    def fwd(x=p, n=4, n_src=2, C=8, s=16, ldc=16, ldb=128, w=p, b=p, run=(p, p, p, p), eps=1e-5, mom=0.1, training=1, y=p,
            ldcy=16, ldby=128, saved=p, ws=p, ws_bytes=big):
        return L.raw('rgda_transnorm_fwd')(x, n, n_src, C, s, ldc, ldb, w, b, *run, eps, mom, training, y, ldcy, ldby, saved,
                                           ws, ws_bytes, None)

    def bwd(g=p, ldcg=16, ldbg=128, x=p, n=4, n_src=2, C=8, s=16, ldc=16, ldb=128, w=p, saved=p, training=1, dx=p, ldcd=16,
            ldbd=128, dw=p, db=p, ws=p, ws_bytes=big):
        return L.raw('rgda_transnorm_bwd')(g, ldcg, ldbg, x, n, n_src, C, s, ldc, ldb, w, saved, training, dx, ldcd, ldbd, dw,
                                           db, ws, ws_bytes, None)

    ARG, WS, UNSUP = -1, -2, -4
    for kw in (dict(x=None), dict(y=None), dict(saved=None), dict(ws=None), dict(n=0), dict(C=0), dict(s=0), dict(eps=-1.0),
               dict(eps=float('nan')), dict(mom=1.5), dict(mom=float('nan')), dict(w=None), dict(b=None),
               dict(run=(p, None, p, p)), dict(run=(None,) * 4, training=0), dict(n_src=5), dict(n_src=-1), dict(ldc=15),
               dict(ldb=127), dict(ldcy=15), dict(ldby=100), dict(ws=ctypes.c_void_p(4096 + 16))):
        assert fwd(**kw) == ARG, kw
    for kw in (dict(n=1, n_src=0), dict(n_src=0), dict(n_src=4), dict(n=2, n_src=1, s=1, ldc=1, ldb=8, ldcy=1, ldby=8),
               dict(C=(1 << 20) + 1, ldb=big, ldby=big)):
        assert fwd(**kw) == UNSUP, kw
    assert fwd(ws_bytes=64) == WS
    for kw in (dict(g=None), dict(x=None), dict(saved=None), dict(ws=None), dict(n=0), dict(C=0), dict(s=0), dict(n_src=5),
               dict(ldc=15), dict(ldbg=127), dict(ldcd=15), dict(ws=ctypes.c_void_p(4096 + 16))):
        assert bwd(**kw) == ARG, kw
    for kw in (dict(n=1, n_src=0), dict(n_src=0), dict(n_src=4)):
        assert bwd(**kw) == UNSUP, kw
    assert bwd(ws_bytes=64) == WS
    # through the binding: argument errors and unserved sizes are ValueError
    with pytest.raises(ValueError):
        L.call('rgda_transnorm_fwd', None, 4, 2, 8, 16, 16, 128, None, None, None, None, None, None, 1e-5, 0.1, 1, None, 16,
               128, None, None, 0, None)
    with pytest.raises(ValueError):
        L.call('rgda_transnorm_bwd', None, 16, 128, None, 4, 2, 8, 16, 16, 128, None, None, 1, None, 16, 128, None, None,
               None, 0, None)
