"""GPU: every convolution route of tests/conv_routes.py against a float64 reference of the same operation on the same
bf16 operands (computed on the GPU in fp64), checked per element, per statistics group and channel, and -- for the
weight gradient -- per weight against the sum of |dy x| it is made of.  The rounding model: bf16 operands, fp32
accumulation, bf16 rounding of the convolution result before the fused epilogue and of the stored result after it."""
import pytest
import torch
import torch.nn.functional as F

import conv_routes as R
from conv_routes import U, U32

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
DEV = 'cuda'


@pytest.fixture(scope='module')
def ops():
    from regda_amd import ops
    torch.backends.cuda.matmul.allow_tf32 = False
    torch.backends.cudnn.allow_tf32 = False
    return ops


def _seed(*key):
    import zlib
    return zlib.crc32(repr(key).encode()) % 100000


def _rand(gen, *shape, scale=1.0):
    return (torch.randn(*shape, generator=gen) * scale).to(BF).to(DEV)


def _conv64(p, x, wk, absval=False):
    """fp64 convolution of pixel-major x [N*H*W][Cin] with wk [Cout][k*k][Cin] in the problem's mode -> [N*Ho*Wo][Cout]."""
    xs = x.double().reshape(p.N, p.H, p.W, p.Cin).permute(0, 3, 1, 2)
    w4 = wk.double().reshape(p.Cout, p.k, p.k, p.Cin)
    if absval:
        xs, w4 = xs.abs(), w4.abs()
    if p.mode == 0:
        y = F.conv2d(xs, w4.permute(0, 3, 1, 2), None, p.stride, p.pad, p.dil)
    else:
        y = torch.nn.grad.conv2d_input((p.N, p.Cout, p.Ho, p.Wo), w4.permute(3, 0, 1, 2).contiguous(), xs, p.stride, p.pad,
                                       p.dil)
    return y.permute(0, 2, 3, 1).reshape(-1, p.Cout)


def _mask_bits(keep):
    M, C = keep.shape
    return (keep.reshape(M, C // 8, 8).to(torch.uint8) << torch.arange(8, dtype=torch.uint8, device=keep.device)).sum(-1) \
        .to(torch.uint8).contiguous()


def _check_stats(stats, y, G, frac, weight=None, what='stats'):
    got = stats.double().sum(1) * 2.0 ** -frac                       # replicas added: [G][2][C]
    ref, absref = R.group_sums(y, G, weight)
    bad = R.stat_violations(got, ref, absref, y.shape[0] // G, frac)
    assert bad == 0, '%s: %d of %d (group, sum, channel) entries off; max |diff| %.3e' % (
        what, bad, got.numel(), float((got - ref).abs().max()))


def _run_fwd(ops, p, call, G, x, wk, c64):
    """One rgda_conv2d / _bneval / _bnbwd call on (x, wk) and its checks against c64 = the fp64 convolution."""
    M, Co = p.N * p.Ho * p.Wo, p.Cout
    gen = torch.Generator().manual_seed(_seed(tuple(p), call, G))
    y = torch.full((M, Co), float('nan'), dtype=BF, device=DEV)
    args = (p.N, p.H, p.W, p.Ho, p.Wo, p.k, p.k, p.stride, p.pad, p.dil)
    ca = c64.abs()
    if call in ('plain', 'stats', 'res', 'res_stats', 'res_mask'):
        res = _rand(gen, M, Co) if call.startswith('res') else None
        keep = (torch.rand(M, Co, generator=gen) > 0.4).to(DEV) if call == 'res_mask' else None
        stats = ops.new_stats(G, 8, 2, Co) if 'stats' in call else None
        ops.conv2d(x, wk, y, *args, p.mode, res, stats, G, res_mask=None if keep is None else _mask_bits(keep))
        ref, extra = c64, None
        if res is not None:
            r = res.double() if keep is None else torch.where(keep, res.double(), torch.zeros_like(c64))
            ref = c64 + r
            extra = U * (1 + U) * ca          # the convolution result is rounded to bf16 before the residual add
        bad = R.elem_violations(y, ref, extra=extra)
        assert bad == 0, '%s: %d of %d elements off; max |diff| %.3e' % (call, bad, y.numel(), float((y.double() - ref).abs().max()))
        if stats is not None:
            _check_stats(stats, y, G, ops.STAT_FRAC_FWD)
        return
    if call in ('ev', 'ev_relu'):
        relu = call == 'ev_relu'
        rm = (torch.randn(Co, generator=gen) * 0.3).to(DEV)
        rv = (torch.rand(Co, generator=gen) + 0.5).to(DEV)
        gamma = (torch.rand(Co, generator=gen) + 0.5).to(DEV)
        gamma[::5] *= -1
        beta = (torch.randn(Co, generator=gen) * 0.3).to(DEV)
        res = _rand(gen, M, Co) if relu else None
        ops.conv2d_bneval(x, wk, y, p.N, p.H, p.W, p.Ho, p.Wo, p.k, p.k, p.stride, p.pad, p.dil, rm, rv, gamma, beta, relu, res)
        sc = gamma.double() / torch.sqrt(rv.double() + 1e-5)
        sh = beta.double() - rm.double() * sc
        pre = c64 * sc + sh + (res.double() if relu else 0)
        ref = pre.clamp_min(0) if relu else pre
        # rounding points: bf16(conv) (U |conv sc|), fp32 scale / shift / adds (a few 2^-24 of every term), bf16 store
        # (U |pre|: the ReLU is 1-Lipschitz, so the pre-activation bound holds after it)
        terms = (c64 * sc).abs() + sh.abs() + (res.double().abs() if relu else 0)
        bad = R.elem_violations(y, ref, mag=pre.abs(), extra=U * (1 + U) * (c64 * sc).abs() + 8 * U32 * terms)
        assert bad == 0, '%s: %d of %d elements off; max |diff| %.3e' % (call, bad, y.numel(), float((y.double() - ref).abs().max()))
        return
    # bnbwd1 / bnbwd2: the data gradient (+ residual) with the consumer BatchNorm's backward sums fused
    relu = 1 if call == 'bnbwd1' else 2
    res = _rand(gen, M, Co) if relu == 1 else None
    bn_x = _rand(gen, M, Co)
    bn_y = _rand(gen, M, Co) if relu == 1 else None
    mean = torch.randn(G, Co, generator=gen) * 0.2
    istd = torch.rand(G, Co, generator=gen) + 0.5
    mi = torch.stack([mean, istd], 1).to(DEV).contiguous()
    ns = ((torch.rand(p.N, Co, generator=gen) > 0.2).float() / 0.8).to(DEV)
    gamma = (torch.rand(Co, generator=gen) + 0.5).to(DEV)
    gamma[::3] *= -1
    beta = (torch.randn(Co, generator=gen) * 0.3).to(DEV)
    sums = ops.new_stats(G, 8, 2, Co)
    ops.conv2d_bnbwd(x, wk, y, p.N, p.H, p.W, p.Ho, p.Wo, p.k, p.k, p.stride, p.pad, p.dil, p.mode, res, sums, G, bn_y, bn_x, mi,
                     relu, ns, p.Ho * p.Wo, bn_gamma=gamma if relu == 2 else None, bn_beta=beta if relu == 2 else None)
    ref = c64 + (res.double() if res is not None else 0)
    extra = U * (1 + U) * ca if res is not None else None
    bad = R.elem_violations(y, ref, extra=extra)
    assert bad == 0, '%s: %d of %d elements off; max |diff| %.3e' % (call, bad, y.numel(), float((y.double() - ref).abs().max()))
    # the sums of the STORED gradient: g' = y [sign] nscale[image], xhat = (bn_x - mean) invstd, per group of rows
    grp = torch.arange(M, device=DEV) // (M // G)
    m_, i_ = mi[:, 0].double()[grp], mi[:, 1].double()[grp]
    if relu == 1:
        on = bn_y.double() > 0
    else:       # the forward's own fp32 (scale, shift) = (gamma invstd, fma(-mean, scale, beta)); the sign of the fma is exact here
        sc32 = (gamma[None] * mi[:, 1]).double()
        sh32 = (-mi[:, 0].double() * sc32 + beta.double()[None]).float().double()
        on = bn_x.double() * sc32[grp] + sh32[grp] > 0
    g = torch.where(on, y.double(), torch.zeros_like(c64)) * ns.double()[torch.arange(M, device=DEV) // (p.Ho * p.Wo)]
    xhat = (bn_x.double() - m_) * i_
    got = sums.double().sum(1) * 2.0 ** -ops.STAT_FRAC_BWD
    refs, absref = R.group_sums(g, G, xhat)
    # xhat and g' are formed in fp32 too: a few 2^-24 of each term on top of the partial sums' bound
    bad = R.stat_violations(got, refs, absref * (1 + 16.0 / R.PARTIAL_ROWS), M // G, ops.STAT_FRAC_BWD)
    assert bad == 0, '%s sums: %d entries off; max |diff| %.3e' % (call, bad, float((got - refs).abs().max()))


def _run_bnin(ops, p, G):
    """rgda_conv2d_bnin: conv(relu(BatchNorm(c))) with the BatchNorm on the operand path, its fused statistics, (mean, invstd)
    and the running statistics."""
    gen = torch.Generator().manual_seed(_seed(tuple(p), 'bnin', G))
    M, Ci, Co = p.N * p.Ho * p.Wo, p.Cin, p.Cout
    rows = p.N * p.H * p.W
    c = (torch.randn(rows, Ci, generator=gen) * (0.5 + torch.rand(1, Ci, generator=gen)) + torch.randn(1, Ci, generator=gen))
    c = c.to(BF).to(DEV)
    gamma = (0.5 + torch.rand(Ci, generator=gen)).to(DEV)
    gamma[::7] *= -1
    beta = (0.3 * torch.randn(Ci, generator=gen)).to(DEV)
    wk = _rand(gen, Co, p.k * p.k, Ci, scale=(2.0 / (Ci * p.k * p.k)) ** 0.5)
    # the producer's accumulators, exactly representable: fp64 sums rounded to the 2^-26 step, in replica 0
    cg = c.double().reshape(G, rows // G, Ci)
    sq = torch.stack([cg.sum(1), (cg * cg).sum(1)], 1)                   # [G][2][Ci]
    fix = torch.round(sq * 2.0 ** ops.STAT_FRAC_FWD).to(torch.int64)
    pst = ops.new_stats(G, 8, 2, Ci)
    pst[:, 0] = fix
    n = rows // G
    SQ = fix.double() * 2.0 ** -ops.STAT_FRAC_FWD
    S, Q = SQ[:, 0], SQ[:, 1]
    mean = S / n
    var = (Q / n - mean * mean).clamp_min(0)
    invstd = 1.0 / torch.sqrt(var + 1e-5)
    mi = torch.zeros(G, 2, Ci, device=DEV)
    rm = torch.full((Ci,), 0.25, device=DEV)
    rv = torch.full((Ci,), 2.0, device=DEV)
    nbt = torch.zeros((), dtype=torch.int64, device=DEV)
    bnop = ops.bn_operand(pst, gamma, beta, mi, rm, rv, nbt, G, True)
    y = torch.full((M, Co), float('nan'), dtype=BF, device=DEV)
    stats = ops.new_stats(G, 8, 2, Co)
    ops.conv2d_bnin(bnop, c, wk, y, p.N, p.H, p.W, p.Ho, p.Wo, p.k, p.k, p.stride, p.pad, p.dil, None, stats, G)
    # (mean, invstd): fp64 moments of the accumulators, rounded to fp32; the variance's cancellation scales with Q/n
    m_, i_ = mi[:, 0].double(), mi[:, 1].double()
    assert bool(((m_ - mean).abs() <= 4 * U32 * (mean.abs() + 1e-30)).all()), 'bnin mean'
    ivb = 4 * U32 * invstd * (1 + (Q / n) / (var + 1e-5))
    assert bool(((i_ - invstd).abs() <= ivb).all()), 'bnin invstd'
    # the operand as the kernel forms it from those (mean, invstd) of ITS image's group: scale = gamma invstd (fp32),
    # shift = fma(-mean, scale, beta), a = bf16(relu(fma(c, scale, shift))) -- fp32 products of fp32 / bf16 values are exact in
    # fp64, so each fma is one rounding here as there.  The bf16 operand is a documented rounding point: modelled, not
    # bounded, so a tile that used another group's table fails the plain per-element bound below.
    grp = torch.arange(rows, device=DEV) // n
    sc32 = gamma[None] * mi[:, 1]
    sh32 = (-mi[:, 0].double() * sc32.double() + beta.double()[None]).float()
    a32 = (c.double() * sc32.double()[grp] + sh32.double()[grp]).float()
    a = a32.clamp_min(0).to(BF).double()
    ref = _conv64(p, a, wk)
    bad = R.elem_violations(y, ref)
    assert bad == 0, 'bnin: %d of %d elements off; max |diff| %.3e' % (bad, y.numel(), float((y.double() - ref).abs().max()))
    # and that operand is the fp64 BatchNorm + ReLU of c within its bf16 rounding, the fp32 (mean, invstd) bounded above
    # (relative rel of the scale, and of mean x scale) and the fp32 scale / shift / fma (a few 2^-24 of each term)
    sc = gamma.double()[None] * invstd[grp]
    sh64 = beta.double()[None] - mean[grp] * sc
    a64 = (c.double() * sc + sh64).clamp_min(0)
    rel = (ivb / invstd)[grp]
    csc, msc = (c.double() * sc).abs(), (mean[grp] * sc).abs()
    abound = U * a64 + rel * (csc + msc) + 8 * U32 * (csc + sh64.abs() + msc)
    assert bool(((a - a64).abs() <= abound).all()), 'bnin operand'
    _check_stats(stats, y, G, ops.STAT_FRAC_FWD, what='bnin stats')
    # running statistics, group after group in fp32 (momentum 0.1, unbiased variance), and num_batches_tracked += G
    erm, erv = torch.full((Ci,), 0.25, dtype=torch.float64, device=DEV), torch.full((Ci,), 2.0, dtype=torch.float64, device=DEV)
    for g in range(G):
        erm = 0.9 * erm + 0.1 * mean[g]
        erv = 0.9 * erv + 0.1 * var[g] * n / (n - 1)
    assert bool(((rm.double() - erm).abs() <= 16 * U32 * (erm.abs() + mean.abs().max(0).values + 1)).all()), 'running_mean'
    assert bool(((rv.double() - erv).abs() <= 16 * U32 * (erv.abs() + (Q / n).max(0).values + 1)).all()), 'running_var'
    assert int(nbt) == G


def _run_wgrad(ops, p, use_ws):
    from regda_amd._lib import lib
    gen = torch.Generator().manual_seed(_seed(tuple(p), 'wgrad'))
    x = _rand(gen, p.N * p.H * p.W, p.Cin)
    dy = _rand(gen, p.N * p.Ho * p.Wo, p.Cout)
    dw = torch.zeros(p.Cout, p.k * p.k, p.Cin, device=DEV)
    if use_ws:
        # the problem is large enough to split its pixels over workgroups: partial tiles through the workspace
        assert R.wgrad_workspace(lib(), p) > R.WGRAD_WS_COUNTERS
        ops.conv2d_wgrad(x, dy, dw, p.N, p.H, p.W, p.Ho, p.Wo, p.k, p.k, p.stride, p.pad, p.dil)
    else:
        lib().call('rgda_conv2d_wgrad', x.data_ptr(), p.Cin, dy.data_ptr(), p.Cout, dw.data_ptr(), p.N, p.H, p.W, p.Cin, p.Ho,
                   p.Wo, p.Cout, p.k, p.k, p.stride, p.pad, p.dil, None, 0, ops._stream())
    xs = x.double().reshape(p.N, p.H, p.W, p.Cin).permute(0, 3, 1, 2)
    ds = dy.double().reshape(p.N, p.Ho, p.Wo, p.Cout).permute(0, 3, 1, 2)
    shape = (p.Cout, p.Cin, p.k, p.k)
    ref = torch.nn.grad.conv2d_weight(xs, shape, ds, p.stride, p.pad, p.dil).permute(0, 2, 3, 1).reshape(dw.shape)
    mag = torch.nn.grad.conv2d_weight(xs.abs(), shape, ds.abs(), p.stride, p.pad, p.dil).permute(0, 2, 3, 1).reshape(dw.shape)
    # products of bf16 operands are exact in fp32; the pixel sum runs in fp32 MFMA steps of 16 products, then over K tiles
    # and splits: at most P / 16 + 64 roundings of a partial, each within 2^-24 of the magnitudes summed so far
    P = p.N * p.Ho * p.Wo
    bound = U32 * (P / 16 + 64) * mag
    bad = int(((dw.double() - ref).abs() > bound).sum())
    assert bad == 0, 'wgrad (ws=%s): %d of %d weights off; max |diff| %.3e' % (use_ws, bad, dw.numel(),
                                                                              float((dw.double() - ref).abs().max()))


def _ids(r):
    p = r.problem
    return '%s|%dx%dx%dx%d-%d-k%ds%dd%dm%d' % (r.name.replace(' ', ''), p.N, p.H, p.W, p.Cin, p.Cout, p.k, p.stride, p.dil,
                                               p.mode)


@pytest.mark.parametrize('route', R.ROUTES, ids=[_ids(r) for r in R.ROUTES])
def test_route_matches_float64_reference(ops, route):
    from regda_amd._lib import lib
    p = route.problem
    fwd = [(c, g) for c, g in R.expand(route) if c not in R.WGRAD and c != 'bnin']
    if fwd:
        gen = torch.Generator().manual_seed(_seed(tuple(p)))
        K = p.Cin * p.k * p.k
        x = _rand(gen, p.N * p.H * p.W, p.Cin)
        wk = _rand(gen, p.Cout, p.k * p.k, p.Cin, scale=(2.0 / K) ** 0.5)
        c64 = _conv64(p, x, wk)
        for call, G in fwd:
            assert R.route_of(lib(), call, p, G) == route.name
            _run_fwd(ops, p, call, G, x, wk, c64)
    for call, G in R.expand(route):
        if call == 'bnin':
            _run_bnin(ops, p, G)
        elif call in R.WGRAD:
            _run_wgrad(ops, p, call == 'wgrad')
    torch.cuda.synchronize()


@pytest.mark.parametrize('call,p,G', R.SUB_IMAGE, ids=['%s-%dimg-%dgroups' % (c, p.N, g) for c, p, g in R.SUB_IMAGE])
def test_sub_image_statistics_groups_are_refused_or_correct(ops, call, p, G):
    """Statistics groups that are not whole images: refused (ValueError).  A library that accepts one must still be right
    per element and per group."""
    gen = torch.Generator().manual_seed(_seed(tuple(p), 'sub'))
    try:
        if call == 'bnin':
            _run_bnin(ops, p, G)
        else:
            x = _rand(gen, p.N * p.H * p.W, p.Cin)
            wk = _rand(gen, p.Cout, p.k * p.k, p.Cin, scale=(2.0 / (p.Cin * p.k * p.k)) ** 0.5)
            _run_fwd(ops, p, call, G, x, wk, _conv64(p, x, wk))
    except ValueError:
        return
    torch.cuda.synchronize()
