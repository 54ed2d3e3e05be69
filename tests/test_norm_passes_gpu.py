"""GPU: the BatchNorm, small-map BatchNorm, max-pool and InstanceNorm passes on every case of tests/norm_cases.py, per
element and per (group, channel), against float64 references on the same stored bf16 inputs (computed on the GPU).

Technique (as tests/test_conv_routes_gpu.py: _run_bnin): where a pass consumes fixed-point accumulators they are exact
integers, so the (mean, invstd) it must form are known; the documented rounding points (the fp32 scale, the fp32 moments
of the backward, the bf16 store) are modelled, only the fp32 arithmetic between them is bounded.  Where a pass forms its
own statistics (the small-map kernels, InstanceNorm) the bounds of the outputs are derived from the bound of the sums."""
import pytest
import torch
import torch.nn.functional as F

import norm_cases as N
from norm_cases import U, U32

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
DEV = 'cuda'
EPS, MOM = 1e-5, 0.1


@pytest.fixture(scope='module')
def ops():
    from regda_amd import ops
    return ops


def _gen(*key):
    import zlib
    return torch.Generator(device=DEV).manual_seed(zlib.crc32(repr(key).encode()) % 100000)


def _strided(rows, C, pad, dtype=BF, fill=float('nan')):
    """[rows][C] view of a [rows][C + pad] buffer (every row stride tested is C + pad); the pad is NaN-filled."""
    return torch.full((rows, C + pad), fill, dtype=dtype, device=DEV)[:, :C]


def _bf(gen, rows, C, pad, scale=1.0, offset=0.0):
    t = _strided(rows, C, pad)
    t.copy_((torch.randn(rows, C, generator=gen, device=DEV) * scale + offset).to(BF))
    return t


def _bad(got, ref, bound):
    d = (got.double() - ref).abs()
    return int((~(d <= bound)).sum()), float(d[torch.isfinite(d)].max()) if bool(torch.isfinite(d).any()) else float('nan')


def _check(name, got, ref, bound):
    n, mx = _bad(got, ref, bound)
    assert n == 0, '%s: %d of %d off; max |diff| %.3e' % (name, n, got.numel(), mx)


def _mask_bits(keep):
    M, C = keep.shape
    return (keep.reshape(M, C // 8, 8).to(torch.uint8) << torch.arange(8, dtype=torch.uint8, device=keep.device)).sum(-1) \
        .to(torch.uint8).contiguous()


def _moments_of(stats, n, frac=N.FRAC_FWD):
    """(S, Q, mean, var, invstd) in fp64 of exact fixed-point accumulators [G][8][2][C]."""
    SQ = stats.double().sum(1) * 2.0 ** -frac
    S, Q = SQ[:, 0], SQ[:, 1]
    mean = S / n
    var = (Q / n - mean * mean).clamp_min(0)
    return S, Q, mean, var, 1.0 / torch.sqrt(var + EPS)


def _check_mi(name, mi, S, Q, n, mean, var, invstd):
    """(mean, invstd) from exact totals: fp64 moments rounded to fp32; the variance's cancellation scales with Q / n."""
    _check(name + ' mean', mi[:, 0], mean, 4 * U32 * mean.abs())
    _check(name + ' invstd', mi[:, 1], invstd, 4 * U32 * invstd * (1 + (Q / n) / (var + EPS)))


def _running(G, n, mean, var, rm0, rv0):
    erm, erv = rm0.double().clone(), rv0.double().clone()
    for g in range(G):
        erm = (1 - MOM) * erm + MOM * mean[g]
        erv = (1 - MOM) * erv + MOM * var[g] * n / (n - 1)
    return erm, erv


def _check_running(rm, rv, erm, erv, mean, Q, n):
    _check('running_mean', rm, erm, 16 * U32 * (erm.abs() + mean.abs().max(0).values + 1))
    _check('running_var', rv, erv, 16 * U32 * (erv.abs() + (Q / n).max(0).values + 1))


def _apply_ref(c, x, mi, gamma, beta, res, ns_rows, relu):
    """The apply pass given the (mean, invstd) it read: sc = fp32(invstd gamma) (modelled), then
    y = bf16([relu]((x - mean) sc + beta [+ res]) [* nscale]).  fp32 between: the subtraction, the product / fma, the
    residual add and the scale are each one rounding of at most 2^-24 of the magnitudes involved -> 4 2^-24 of
    |x - mean| |sc| + |beta| + |res|, times the scale; the ReLU is 1-Lipschitz."""
    G = c.G
    grp = torch.arange(c.Mg * G, device=DEV) // c.Mg
    mean = mi[:, 0].double()[grp]
    sc = (mi[:, 1] * gamma[None]).double()[grp]
    d = (x.double() - mean) * sc
    pre = d + beta.double()[None]
    terms = d.abs() + beta.double().abs()[None]
    if res is not None:
        pre = pre + res.double()
        terms = terms + res.double().abs()
    if relu:
        pre = pre.clamp_min(0)
    s = ns_rows if ns_rows is not None else 1.0
    ref = pre * s
    bound = U * ref.abs() + 5 * U32 * terms * (s.abs() if ns_rows is not None else 1.0)
    return ref, bound


def _exact_stats(x, G):
    """Exactly representable accumulators of x's per-group sums, spread over the eight replicas (the 2^-26 step)."""
    M, C = x.shape
    xg = x.double().reshape(G, M // G, C)
    fix = torch.round(torch.stack([xg.sum(1), (xg * xg).sum(1)], 1) * 2.0 ** N.FRAC_FWD).to(torch.int64)   # [G][2][C]
    st = torch.zeros(G, 8, 2, C, dtype=torch.int64, device=DEV)
    q = torch.div(fix, 8, rounding_mode='floor')
    st[:] = q[:, None]
    st[:, 7] = fix - 7 * q
    return st


def _forward(ops, c, gen):
    """Every forward pass of one case.  -> what the backward needs."""
    M, C, G, n = c.Mg * c.G, c.C, c.G, c.Mg
    # per-channel spread and offset (the variance's cancellation shows), a few channels of large magnitude
    scale = 0.5 + torch.rand(1, C, generator=gen, device=DEV) * 2
    off = torch.randn(1, C, generator=gen, device=DEV)
    x = _bf(gen, M, C, c.pad, scale, off)
    gamma = 0.5 + torch.rand(C, generator=gen, device=DEV)
    gamma[::7] *= -1
    beta = 0.3 * torch.randn(C, generator=gen, device=DEV)
    res = _bf(gen, M, C, c.pad) if c.res else None
    images = M // c.rpi
    nscale = ((torch.rand(images, C, generator=gen, device=DEV) > 0.2).float() * 1.25).contiguous() if c.nscale else None
    ns_rows = nscale.double()[torch.arange(M, device=DEV) // c.rpi] if c.nscale else None

    # ---- rgda_bn_stats: fp32 partials of one workgroup's rows_per_block rows, then the 2^-26 step
    stats = ops.new_stats(G, 8, 2, C)
    for g in range(G):
        ops.bn_stats(x[g * n:(g + 1) * n], stats[g], n, C)
    prows = N.stats_grid(n, C)[0]
    xg = x.double().reshape(G, n, C)
    ref = torch.stack([xg.sum(1), (xg * xg).sum(1)], 1)
    absref = torch.stack([xg.abs().sum(1), (xg * xg).sum(1)], 1)
    got = stats.double().sum(1) * 2.0 ** -N.FRAC_FWD
    bad = N.stat_violations(got, ref, absref, n, N.FRAC_FWD, partial_rows=prows)
    assert bad == 0, 'bn_stats: %d entries off; max |diff| %.3e' % (bad, float((got - ref).abs().max()))

    # ---- rgda_bn_finalize + rgda_bn_apply on those (exact) accumulators
    S, Q, mean, var, invstd = _moments_of(stats, n)
    mi = torch.full((G, 2, C), float('nan'), device=DEV)
    rm0 = 0.2 * torch.randn(C, generator=gen, device=DEV)
    rv0 = 0.5 + torch.rand(C, generator=gen, device=DEV)
    rm, rv = rm0.clone(), rv0.clone()
    nbt = torch.full((), 5, dtype=torch.int64, device=DEV)
    ops.bn_finalize(stats, mi, rm, rv, nbt, M, C, EPS, MOM, G)
    _check_mi('finalize', mi, S, Q, n, mean, var, invstd)
    erm, erv = _running(G, n, mean, var, rm0, rv0)
    _check_running(rm, rv, erm, erv, mean, Q, n)
    assert int(nbt) == 5 + G
    y = _strided(M, C, c.pad)
    ops.bn_apply(x, mi, gamma, beta, y, M, C, c.relu, res, nscale, c.rpi, G)
    ref, bound = _apply_ref(c, x, mi, gamma, beta, res, ns_rows, c.relu)
    _check('bn_apply', y, ref, bound)

    # ---- rgda_bn_train_apply (finalize folded in): bit-identical to stats + finalize + apply
    mi2 = torch.full((G, 2, C), float('nan'), device=DEV)
    rm2, rv2 = rm0.clone(), rv0.clone()
    nbt2 = torch.full((), 5, dtype=torch.int64, device=DEV)
    y2 = _strided(M, C, c.pad)
    mask = torch.zeros(M, C // 8, dtype=torch.uint8, device=DEV) if c.relu else None
    ops.bn_train_apply(x, stats, mi2, rm2, rv2, nbt2, gamma, beta, y2, M, C, c.relu, res, nscale, c.rpi, G, EPS, MOM, mask)
    assert torch.equal(mi2, mi), 'train_apply mi'
    assert torch.equal(rm2, rm) and torch.equal(rv2, rv) and int(nbt2) == int(nbt), 'train_apply running statistics'
    assert torch.equal(y2.view(torch.int16), y.view(torch.int16)), 'train_apply y'
    if mask is not None:
        assert torch.equal(mask, _mask_bits(y2.float() > 0)), 'train_apply relu mask'
    return dict(x=x, y=y, mask=mask, mi=mi, gamma=gamma, beta=beta, nscale=nscale, ns_rows=ns_rows)


def _backward(ops, c, gen, f, mode):
    M, C, G, n = c.Mg * c.G, c.C, c.G, c.Mg
    x, mi, gamma, beta = f['x'], f['mi'], f['gamma'], f['beta']
    g = _bf(gen, M, C, c.pad)
    grp = torch.arange(M, device=DEV) // n
    mean, istd = mi[:, 0].double()[grp], mi[:, 1].double()[grp]
    relu = {0: 0, 'y': 1, 'mask': 1, 2: 2}[mode]
    yarg = f['y'] if mode == 'y' else None
    marg = f['mask'] if mode == 'mask' else None
    if mode in ('y', 'mask'):
        on = f['y'].double() > 0
    elif mode == 2:     # the forward operand path's fp32 (scale, shift): the sign of the fma is exact in fp64 here
        sc32 = (gamma[None] * mi[:, 1]).double()
        sh32 = (-mi[:, 0].double() * sc32 + beta.double()[None]).float().double()
        a64 = x.double() * sc32[grp] + sh32[grp]
        on = a64 > 0
    else:
        on = torch.ones(M, C, dtype=torch.bool, device=DEV)
    gp = torch.where(on, g.double(), torch.zeros((), dtype=torch.float64, device=DEV))
    if f['ns_rows'] is not None:
        gp = gp * f['ns_rows']
    xhat = (x.double() - mean) * istd
    kw = dict(gamma=gamma, beta=beta) if relu == 2 else {}

    # ---- rgda_bn_bwd_reduce: sums of g' and g' xhat per group; xhat and g' are formed in fp32 (a few 2^-24 of
    # |g'| (|x| + |mean|) invstd per term: the +8 terms of stat_violations' n)
    sums = ops.new_stats(G, 8, 2, C)
    ops.bn_bwd_reduce(g, yarg, x, mi, sums, M, C, relu, f['nscale'], c.rpi, G, marg, **kw)
    prows = N.bwd_reduce_grid(M, C, G)[0]
    gpg, xhg = gp.reshape(G, n, C), xhat.reshape(G, n, C)
    ref = torch.stack([gpg.sum(1), (gpg * xhg).sum(1)], 1)
    wabs = (gp.abs() * (x.double().abs() + mean.abs()) * istd).reshape(G, n, C).sum(1)
    absref = torch.stack([gpg.abs().sum(1), wabs], 1)
    got = sums.double().sum(1) * 2.0 ** -N.FRAC_BWD
    bad = N.stat_violations(got, ref, absref, n, N.FRAC_BWD, partial_rows=prows)
    assert bad == 0, 'bn_bwd_reduce %s: %d entries off; max |diff| %.3e' % (mode, bad, float((got - ref).abs().max()))

    # ---- rgda_bn_bwd_apply on those exact sums: k1 = fp32(t1) * fp32(1 / n), k2 likewise, k0 = fp32(gamma invstd)
    # (modelled); dx = bf16(k0 (g' - k1 - (x - mean) invstd k2)): fp32 subtraction, products and differences between,
    # 8 2^-24 of |k0| (|g'| + |k1| + |xhat k2|)
    t = sums.double().sum(1) * 2.0 ** -N.FRAC_BWD            # exact totals [G][2][C]
    invM = torch.tensor(1.0 / n, dtype=torch.float32, device=DEV)
    k1 = (t[:, 0].float() * invM).double()[grp]
    k2 = (t[:, 1].float() * invM).double()[grp]
    k0 = (gamma[None] * mi[:, 1]).double()[grp]
    dx = _strided(M, C, c.pad)
    gmask = _strided(M, C, c.pad)
    dgamma = torch.zeros(C, device=DEV)
    dbeta = torch.zeros(C, device=DEV)
    act = _strided(M, C, c.pad) if relu == 2 else None
    ops.bn_bwd_apply(g, yarg, x, mi, gamma, sums, dx, M, C, relu, gmask, dgamma, dbeta, f['nscale'], c.rpi, G, marg,
                     beta if relu == 2 else None, act)
    ref = k0 * (gp - k1 - xhat * k2)
    bound = U * ref.abs() + 8 * U32 * k0.abs() * (gp.abs() + k1.abs() + (xhat * k2).abs())
    _check('bn_bwd_apply dx %s' % mode, dx, ref, bound)
    # the gradient through the gate and the scale, as stored: bf16(g') exactly
    assert torch.equal(gmask.view(torch.int16), gp.float().to(BF).view(torch.int16)), 'gmask %s' % mode
    # dgamma / dbeta: fp32 totals of the groups added in order (one rounding each)
    for name, got, tt in (('dbeta', dbeta, t[:, 0]), ('dgamma', dgamma, t[:, 1])):
        _check('%s %s' % (name, mode), got, tt.sum(0), (G + 1) * U32 * tt.abs().sum(0))
    if act is not None:     # the activation the forward operand path would have formed: bf16(relu(fma(x, sc, sh)));
        # one bf16 step where the fp64 model of the fma rounds to another fp32 value (double rounding)
        a = a64.float().clamp_min(0).to(BF)
        _check('act_out', act, a.double(), 2 * U * a.double().abs())


@pytest.mark.parametrize('case', N.BN_CASES, ids=[c.name for c in N.BN_CASES])
def test_batchnorm_passes(ops, case):
    gen = _gen(case)
    f = _forward(ops, case, gen)
    for mode in case.modes:
        _backward(ops, case, gen, f, mode)
    torch.cuda.synchronize()


# ---------------------------------------------------------------- range: totals beyond the fixed-point range
BAD = 5     # the channel that goes out of range; its neighbours must stay finite and right


@pytest.mark.parametrize('kind', ['many', 'single'])
def test_forward_total_out_of_range_is_nan(ops, kind):
    """The worked example (2^18 rows, +-1024 in one channel: 512 in-range partials whose eight replicas sum to 2^64), and a
    single partial out of range (one row of 2^17: x^2 = 2^34 >= 2^33) -- (mean, invstd) and y of that channel are NaN."""
    Mg = (1 << 18) if kind == 'many' else 4096
    gen = _gen('range', kind)
    C = 64
    x = (torch.randn(Mg, C, generator=gen, device=DEV)).to(BF)
    if kind == 'many':
        x[:, BAD] = torch.where(torch.arange(Mg, device=DEV) % 2 == 0, 1024.0, -1024.0).to(BF)
    else:
        x[100, BAD] = 2.0 ** 17
    stats = ops.new_stats(1, 8, 2, C)
    ops.bn_stats(x, stats[0], Mg, C)
    mi = torch.zeros(1, 2, C, device=DEV)
    rm, rv = torch.zeros(C, device=DEV), torch.ones(C, device=DEV)
    nbt = torch.zeros((), dtype=torch.int64, device=DEV)
    gamma, beta = torch.ones(C, device=DEV), torch.zeros(C, device=DEV)
    y = torch.empty(Mg, C, dtype=BF, device=DEV)
    ops.bn_train_apply(x, stats, mi, rm, rv, nbt, gamma, beta, y, Mg, C, False, groups=1)
    torch.cuda.synchronize()
    assert not bool(torch.isfinite(mi[0, :, BAD]).all()), '%s: mi of the out-of-range channel is finite: %s' % (
        kind, mi[0, :, BAD].tolist())
    assert not bool(torch.isfinite(y[:, BAD].float()).any()), '%s: y of the out-of-range channel is finite' % kind
    assert not bool(torch.isfinite(rv[BAD])), '%s: running_var of the out-of-range channel is finite' % kind
    ok = [c for c in range(C) if c != BAD]
    S, Q, mean, var, invstd = _moments_of(stats[:, :, :, ok], Mg)
    _check_mi(kind + ' neighbours', mi[:, :, ok], S, Q, Mg, mean, var, invstd)
    sc = (mi[0, 1, ok] * gamma[ok]).double()
    ref = (x[:, ok].double() - mi[0, 0, ok].double()) * sc
    _check(kind + ' neighbours y', y[:, ok], ref, U * ref.abs() + 5 * U32 * ref.abs())


@pytest.mark.parametrize('kind', ['many', 'single'])
def test_backward_total_out_of_range_is_nan(ops, kind):
    """Backward sums: 2^18 rows of g' xhat = 128 (partials of 2^16 in range, replicas of 2^62, a total of 2^65 that wrapped
    to 0 in 64 bits), and a single partial out of range (g' xhat = 2^20 >= 2^19) -- dx, dgamma of that channel are NaN."""
    Mg = (1 << 18) if kind == 'many' else 4096
    gen = _gen('brange', kind)
    C = 64
    x = torch.randn(Mg, C, generator=gen, device=DEV).to(BF)
    g = torch.randn(Mg, C, generator=gen, device=DEV).to(BF)
    sign = torch.where(torch.arange(Mg, device=DEV) % 2 == 0, 1.0, -1.0)
    if kind == 'many':
        x[:, BAD] = sign.to(BF)
        g[:, BAD] = (128 * sign).to(BF)
    else:
        x[7, BAD], g[7, BAD] = 1024.0, 1024.0
    mi = torch.stack([torch.zeros(C, device=DEV), torch.ones(C, device=DEV)])[None].contiguous()    # mean 0, invstd 1
    gamma = torch.ones(C, device=DEV)
    sums = ops.new_stats(1, 8, 2, C)
    ops.bn_bwd_reduce(g, None, x, mi, sums, Mg, C, 0)
    dx = torch.empty(Mg, C, dtype=BF, device=DEV)
    dgamma, dbeta = torch.zeros(C, device=DEV), torch.zeros(C, device=DEV)
    ops.bn_bwd_apply(g, None, x, mi, gamma, sums, dx, Mg, C, 0, None, dgamma, dbeta)
    torch.cuda.synchronize()
    assert not bool(torch.isfinite(dx[:, BAD].float()).any()), '%s: dx of the out-of-range channel is finite' % kind
    assert not bool(torch.isfinite(dgamma[BAD])), '%s: dgamma of the out-of-range channel is finite' % kind
    ok = [c for c in range(C) if c != BAD]
    t = sums[0, :, :, ok].double().sum(0) * 2.0 ** -N.FRAC_BWD
    gd, xd = g[:, ok].double(), x[:, ok].double()
    refs = torch.stack([gd.sum(0), (gd * xd).sum(0)])
    assert bool(((t - refs).abs() <= U32 * 600 * torch.stack([gd.abs().sum(0), (gd * xd).abs().sum(0)]) + 1e-6).all())
    k1 = (t[0].float() / Mg).double()
    k2 = (t[1].float() / Mg).double()
    ref = gd - k1 - xd * k2
    _check(kind + ' neighbours dx', dx[:, ok], ref, U * ref.abs() + 8 * U32 * (gd.abs() + k1.abs() + (xd * k2).abs()))
    _check(kind + ' neighbours dgamma', dgamma[ok], t[1], U32 * t[1].abs())


# ---------------------------------------------------------------- the small-map kernels
def _small_inputs(gen, C, G, Mg):
    M = G * Mg
    x = _bf(gen, M, C, 8, 0.5 + torch.rand(1, C, generator=gen, device=DEV) * 2, torch.randn(1, C, generator=gen, device=DEV))
    gamma = 0.5 + torch.rand(C, generator=gen, device=DEV)
    gamma[::5] *= -1
    beta = 0.3 * torch.randn(C, generator=gen, device=DEV)
    return x, gamma, beta


def test_small_map_batchnorm(ops):
    """rgda_bn_train_small / rgda_bn_bwd_small on every SMALL descriptor in ONE call each (more than BN_SMALL_MAX of every
    kind).  The kernels sum the stored values themselves: fp32 over <= 5 rows per thread and three shuffles, fp64 over the
    eight waves -- at most 8 roundings of a running partial, so |d S| <= 10 2^-24 sum |x|, |d Q| <= 10 2^-24 sum x^2;
    (mean, var, invstd) and y are bounded from those (norm_cases.moment_bounds)."""
    gen = _gen('small')
    fwd, keep = [], []
    for i, (C, G, Mg, relu) in enumerate(N.SMALL):
        x, gamma, beta = _small_inputs(gen, C, G, Mg)
        M = G * Mg
        y = _strided(M, C, 16)
        mi = torch.full((G, 2, C), float('nan'), device=DEV)
        rm0, rv0 = 0.2 * torch.randn(C, generator=gen, device=DEV), 0.5 + torch.rand(C, generator=gen, device=DEV)
        rm, rv = rm0.clone(), rv0.clone()
        nbt = torch.zeros((), dtype=torch.int64, device=DEV)
        mask = torch.zeros(M, C // 8, dtype=torch.uint8, device=DEV) if relu else None
        fwd.append((x, y, mi, rm, rv, nbt, gamma, beta, M, C, relu, G, mask))
        keep.append((rm0, rv0))
    ops.bn_train_small(fwd, EPS, MOM)
    bwd, refs = [], []
    for (x, y, mi, rm, rv, nbt, gamma, beta, M, C, relu, G, mask), (rm0, rv0) in zip(fwd, keep):
        Mg = M // G
        xg = x.double().reshape(G, Mg, C)
        S, Q = xg.sum(1), (xg * xg).sum(1)
        mean, var, invstd, dm, dv, rel = N.moment_bounds(S, Q, Mg, 10 * U32 * xg.abs().sum(1), 10 * U32 * Q)
        _check('small mean C%d' % C, mi[:, 0], mean, dm)
        _check('small invstd C%d' % C, mi[:, 1], invstd, rel * invstd)
        # y = (x - mean) (invstd gamma) + beta: the statistics' errors move it by |gamma| (dm invstd + |x - mean| invstd rel)
        grp = torch.arange(M, device=DEV) // Mg
        pre = (x.double() - mean[grp]) * (invstd * gamma.double()[None])[grp] + beta.double()[None]
        ref = pre.clamp_min(0) if relu else pre
        stat = gamma.double().abs()[None] * (dm * invstd)[grp] + \
            ((x.double() - mean[grp]).abs() * (invstd * rel * gamma.double().abs()[None])[grp])
        bound = U * ref.abs() + stat * (1 + U) + 5 * U32 * (pre - beta.double()[None]).abs() + 5 * U32 * beta.double().abs()[None]
        _check('small y C%d G%d rows%d' % (C, G, Mg), y, ref, bound)
        if mask is not None:
            assert torch.equal(mask, _mask_bits(y.float() > 0))
        erm, erv = _running(G, Mg, mean, var, rm0, rv0)
        _check('small running_mean', rm, erm, 16 * U32 * (erm.abs() + mean.abs().max(0).values + 1) + MOM * dm.max(0).values)
        _check('small running_var', rv, erv, 16 * U32 * (erv.abs() + (Q / Mg).max(0).values + 1) +
               MOM * dv.max(0).values * Mg / (Mg - 1) * G)
        assert int(nbt) == G
        # the backward: gated by y and by the mask (relu 1), or not at all (relu 0)
        for gate in (('y', 'mask') if relu else (None,)):
            g = _bf(gen, M, C, 8)
            dx = _strided(M, C, 8)
            dgamma, dbeta = torch.zeros(C, device=DEV), torch.zeros(C, device=DEV)
            bwd.append((g, y if gate == 'y' else None, x, mi, gamma, dx, dgamma, dbeta, M, C, relu, G,
                        mask if gate == 'mask' else None))
            refs.append((gate, g, dx, dgamma, dbeta))
    ops.bn_bwd_small(bwd)
    for (g, yb, x, mi, gamma, dx, dgamma, dbeta, M, C, relu, G, mask), (gate, _, _, _, _) in zip(bwd, refs):
        Mg = M // G
        y = next(f[1] for f in fwd if f[0] is x)
        grp = torch.arange(M, device=DEV) // Mg
        on = (y.double() > 0) if relu else torch.ones(M, C, dtype=torch.bool, device=DEV)
        gp = torch.where(on, g.double(), torch.zeros((), dtype=torch.float64, device=DEV))
        m_, i_ = mi[:, 0].double()[grp], mi[:, 1].double()[grp]
        xhat = (x.double() - m_) * i_
        t1 = gp.reshape(G, Mg, C).sum(1)
        t2 = (gp * xhat).reshape(G, Mg, C).sum(1)
        # fp32 sums as in the forward (10 2^-24 of the magnitudes; xhat itself two roundings)
        d1 = 10 * U32 * gp.abs().reshape(G, Mg, C).sum(1)
        d2 = 12 * U32 * (gp.abs() * (x.double().abs() + m_.abs()) * i_).reshape(G, Mg, C).sum(1)
        k0 = (gamma[None] * mi[:, 1]).double()[grp]
        k1, k2 = (t1 / Mg)[grp], (t2 / Mg)[grp]
        ref = k0 * (gp - k1 - xhat * k2)
        bound = U * ref.abs() + k0.abs() * ((d1 / Mg)[grp] * (1 + U) + xhat.abs() * (d2 / Mg)[grp] * (1 + U)) + \
            8 * U32 * k0.abs() * (gp.abs() + k1.abs() + (xhat * k2).abs())
        _check('small dx C%d G%d rows%d gate %s' % (C, G, Mg, gate), dx, ref, bound)
        _check('small dbeta', dbeta, t1.sum(0), d1.sum(0) + (G + 1) * U32 * t1.abs().sum(0))
        _check('small dgamma', dgamma, t2.sum(0), d2.sum(0) + (G + 1) * U32 * t2.abs().sum(0))
    torch.cuda.synchronize()


def test_small_map_matches_the_general_kernels(ops):
    """bn_train_small and bn_train_apply on the same input: both within their bounds of the fp64 BatchNorm, so within the
    sum of the two of each other (the general path's statistics are exact fixed-point totals, its (mean, invstd) within
    4 2^-24)."""
    gen = _gen('small-vs-general')
    C, G, Mg = 72, 3, 320
    x, gamma, beta = _small_inputs(gen, C, G, Mg)
    M = G * Mg
    ys, mis = [], []
    for path in ('small', 'general'):
        y = _strided(M, C, 8)
        mi = torch.zeros(G, 2, C, device=DEV)
        rm, rv = torch.zeros(C, device=DEV), torch.ones(C, device=DEV)
        nbt = torch.zeros((), dtype=torch.int64, device=DEV)
        if path == 'small':
            ops.bn_train_small([(x, y, mi, rm, rv, nbt, gamma, beta, M, C, 1, G, None)], EPS, MOM)
        else:
            st = _exact_stats(x, G)
            ops.bn_train_apply(x, st, mi, rm, rv, nbt, gamma, beta, y, M, C, 1, groups=G, eps=EPS, momentum=MOM)
        ys.append(y)
        mis.append(mi)
    xg = x.double().reshape(G, Mg, C)
    S, Q = xg.sum(1), (xg * xg).sum(1)
    mean, var, invstd, dm, dv, rel = N.moment_bounds(S, Q, Mg, 10 * U32 * xg.abs().sum(1), 10 * U32 * Q)
    grp = torch.arange(M, device=DEV) // Mg
    pre = (x.double() - mean[grp]) * (invstd * gamma.double()[None])[grp] + beta.double()[None]
    stat = gamma.double().abs()[None] * (dm * invstd)[grp] + \
        ((x.double() - mean[grp]).abs() * (invstd * rel * gamma.double().abs()[None])[grp])
    bound = 2 * (U * pre.abs() + stat * (1 + U) + 5 * U32 * (pre.abs() + beta.double().abs()[None]))
    _check('small vs general y', ys[0], ys[1].double(), bound)
    _check('small vs general mean', mis[0][:, 0], mis[1][:, 0].double(), 2 * dm)
    _check('small vs general invstd', mis[0][:, 1], mis[1][:, 1].double(), 2 * rel * invstd)


# ---------------------------------------------------------------- max-pool 3x3 / 2 / pad 1
def _pool_ref(a, N_, H, W, C):
    """fp64 max-pool of pixel-major a [N*H*W][C] and torch's argmax (the first maximum in scan order, as the kernel)."""
    t = a.double().reshape(N_, H, W, C).permute(0, 3, 1, 2)
    y, idx = F.max_pool2d(t, 3, 2, 1, return_indices=True)
    return y, idx


def _check_pool(name, y, idx_k, gx, gy, ref_y, ref_idx, N_, H, W, C, Ho, Wo):
    yk = y.double().reshape(N_, Ho, Wo, C).permute(0, 3, 1, 2)
    assert torch.equal(yk, ref_y), '%s: y not bit-exact (%d elements differ)' % (name, int((yk != ref_y).sum()))
    # the gradient: every gy element routed to the element torch's tie rule picks, summed in fp32, stored as bf16
    g = gy.double().reshape(N_, Ho, Wo, C).permute(0, 3, 1, 2).reshape(N_, C, -1)
    ref = torch.zeros(N_, C, H * W, dtype=torch.float64, device=DEV).scatter_add_(2, ref_idx.reshape(N_, C, -1), g)
    mag = torch.zeros_like(ref).scatter_add_(2, ref_idx.reshape(N_, C, -1), g.abs())
    ref = ref.reshape(N_, C, H, W).permute(0, 2, 3, 1).reshape(-1, C)
    mag = mag.reshape(N_, C, H, W).permute(0, 2, 3, 1).reshape(-1, C)
    _check(name + ' gx', gx, ref, U * ref.abs() + 4 * U32 * mag)


@pytest.mark.parametrize('shape', N.POOL, ids=['%dx%dx%dx%d' % s for s in N.POOL])
def test_maxpool(ops, shape):
    N_, H, W, C = shape
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    gen = _gen('pool', shape)
    # few distinct values: many ties inside a window
    x = torch.randint(-3, 4, (N_ * H * W, C), generator=gen, device=DEV).to(BF)
    y = torch.empty(N_ * Ho * Wo, C, dtype=BF, device=DEV)
    idx = torch.empty(N_ * Ho * Wo, C, dtype=torch.uint8, device=DEV)
    ops.maxpool_fwd(x, y, idx, N_, H, W, C, Ho, Wo)
    gy = torch.randn(N_ * Ho * Wo, C, generator=gen, device=DEV).to(BF)
    gx = torch.empty(N_ * H * W, C, dtype=BF, device=DEV)
    ops.maxpool_bwd(gy, idx, gx, N_, H, W, C, Ho, Wo)
    ry, ridx = _pool_ref(x, N_, H, W, C)
    _check_pool('maxpool', y, idx, gx, gy, ry, ridx, N_, H, W, C, Ho, Wo)


@pytest.mark.parametrize('shape', N.POOL_BNIN, ids=['%dx%dx%dx%d-g%d' % s for s in N.POOL_BNIN])
def test_maxpool_with_batchnorm_operand(ops, shape):
    """rgda_maxpool_fwd_bnin: max over bf16(relu(fma(x, scale, shift))) with (scale, shift) from exact accumulators of
    ITS image's group (modelled as in _run_bnin); y bit-exact, the gradient routed as torch routes it."""
    N_, H, W, C, G = shape
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    gen = _gen('poolbn', shape)
    rows = N_ * H * W
    x = (torch.randn(rows, C, generator=gen, device=DEV) + torch.randn(1, C, generator=gen, device=DEV)).to(BF)
    gamma = 0.5 + torch.rand(C, generator=gen, device=DEV)
    gamma[::7] *= -1
    beta = 0.3 * torch.randn(C, generator=gen, device=DEV)
    st = _exact_stats(x, G)
    n = rows // G
    S, Q, mean, var, invstd = _moments_of(st, n)
    mi = torch.zeros(G, 2, C, device=DEV)
    rm0, rv0 = torch.full((C,), 0.25, device=DEV), torch.full((C,), 2.0, device=DEV)
    rm, rv = rm0.clone(), rv0.clone()
    nbt = torch.zeros((), dtype=torch.int64, device=DEV)
    bnop = ops.bn_operand(st, gamma, beta, mi, rm, rv, nbt, G, True)
    y = torch.empty(N_ * Ho * Wo, C, dtype=BF, device=DEV)
    idx = torch.empty(N_ * Ho * Wo, C, dtype=torch.uint8, device=DEV)
    ops.maxpool_fwd_bnin(bnop, x, y, idx, N_, H, W, C, Ho, Wo)
    _check_mi('pool bnin', mi, S, Q, n, mean, var, invstd)
    erm, erv = _running(G, n, mean, var, rm0, rv0)
    _check_running(rm, rv, erm, erv, mean, Q, n)
    assert int(nbt) == G
    grp = torch.arange(rows, device=DEV) // n
    sc32 = gamma[None] * mi[:, 1]
    sh32 = (-mi[:, 0].double() * sc32.double() + beta.double()[None]).float()
    a = (x.double() * sc32.double()[grp] + sh32.double()[grp]).float().clamp_min(0).to(BF)
    gy = torch.randn(N_ * Ho * Wo, C, generator=gen, device=DEV).to(BF)
    gx = torch.empty(rows, C, dtype=BF, device=DEV)
    ops.maxpool_bwd(gy, idx, gx, N_, H, W, C, Ho, Wo)
    ry, ridx = _pool_ref(a, N_, H, W, C)
    _check_pool('maxpool bnin', y, idx, gx, gy, ry, ridx, N_, H, W, C, Ho, Wo)


# ---------------------------------------------------------------- InstanceNorm (no affine)
@pytest.mark.parametrize('shape', N.INORM, ids=['%dx%dx%d-pad%d' % s for s in N.INORM])
def test_instnorm(ops, shape):
    """Statistics in fp32: a thread sums HW / 32 rows, then 32 lanes in order: |d S| <= (HW / 32 + 34) 2^-24 sum |x|;
    mean, E[x^2] - mean^2 and invstd in fp32 (norm_cases.moment_bounds), y = bf16((x - mean) invstd), feat the same in
    fp32.  Backward: k1 = sum g / HW, k2 = sum g xhat / HW likewise, dx = bf16(invstd (g - k1 - xhat k2))."""
    N_, HW, C, pad = shape
    gen = _gen('inorm', shape)
    M = N_ * HW
    x = _bf(gen, M, C, pad, 0.5 + torch.rand(1, C, generator=gen, device=DEV) * 2, torch.randn(1, C, generator=gen, device=DEV))
    y0, y1 = _strided(M, C, pad), _strided(M, C, pad)
    feat = torch.full((N_, C, HW), float('nan'), device=DEV)
    mi = torch.full((N_, 2, C), float('nan'), device=DEV)
    ops.instnorm_fwd(x, y0, y1, feat, mi, N_, HW, C, EPS)
    xg = x.double().reshape(N_, HW, C)
    S, Q = xg.sum(1), (xg * xg).sum(1)
    k = HW / 32 + 34
    mean, var, invstd, dm, dv, rel = N.moment_bounds(S, Q, HW, k * U32 * xg.abs().sum(1), k * U32 * Q)
    _check('instnorm mean', mi[:, 0], mean, dm)
    _check('instnorm invstd', mi[:, 1], invstd, rel * invstd)
    img = torch.arange(M, device=DEV) // HW
    d = (x.double() - mean[img])
    ref = d * invstd[img]
    stat = dm[img] * invstd[img] + d.abs() * (invstd * rel)[img]
    bound = stat * (1 + U) + 3 * U32 * (ref.abs() + mean[img].abs() * invstd[img])
    _check('instnorm feat', feat.permute(0, 2, 1).reshape(M, C), ref, bound)
    _check('instnorm y0', y0, ref, U * ref.abs() + bound * (1 + U))
    assert torch.equal(y0.view(torch.int16), y1.view(torch.int16)), 'instnorm y1'
    # backward on the forward's (mean, invstd), three gradient sources (gc with its own stride)
    ga, gb = _bf(gen, M, C, pad), _bf(gen, M, C, pad)
    gc = _bf(gen, M, C, pad + 8)
    dx = _strided(M, C, pad)
    ops.instnorm_bwd(ga, gb, gc, x, mi, dx, N_, HW, C)
    gs = ga.double() + gb.double() + gc.double()
    gabs = ga.double().abs() + gb.double().abs() + gc.double().abs()
    m_, i_ = mi[:, 0].double()[img], mi[:, 1].double()[img]
    xhat = (x.double() - m_) * i_
    t1, t2 = gs.reshape(N_, HW, C).sum(1), (gs * xhat).reshape(N_, HW, C).sum(1)
    d1 = k * U32 * gabs.reshape(N_, HW, C).sum(1)
    d2 = (k + 6) * U32 * (gabs * (x.double().abs() + m_.abs()) * i_).reshape(N_, HW, C).sum(1)
    k1, k2 = (t1 / HW)[img], (t2 / HW)[img]
    ref = i_ * (gs - k1 - xhat * k2)
    bound = U * ref.abs() + i_ * ((d1 / HW)[img] * (1 + U) + xhat.abs() * (d2 / HW)[img] * (1 + U)) + \
        8 * U32 * i_ * (gabs + k1.abs() + (xhat * k2).abs())
    _check('instnorm dx', dx, ref, bound)
