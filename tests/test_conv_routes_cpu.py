"""CPU: the convolution route table (tests/conv_routes.py) against the library's own dispatch queries (nothing is
launched), the refusal of statistics groups that are not whole images, and a self-test of the GPU route tests' checks:
each must flag each injected fault."""
import itertools

import pytest
import torch
import torch.nn.functional as F

import conv_routes as R


@pytest.fixture(scope='module')
def L():
    from regda_amd import _lib
    return _lib.lib()


def _sweep_problems():
    maps = [(4, 4), (8, 8), (16, 16), (17, 13), (32, 32), (40, 32), (32, 40), (32, 48), (32, 64), (40, 96), (64, 64),
            (128, 128), (8, 128), (16, 64), (8, 16), (8, 32)]
    geoms = [(1, 1, 0, 1), (3, 1, 1, 1), (3, 1, 2, 2), (3, 2, 1, 1), (1, 2, 0, 1)]
    for N, (H, W), Cin, Cout, (k, s, p, d) in itertools.product((1, 2, 3, 4, 7, 8, 16), maps, (64, 128, 192, 256, 512, 1024),
                                                                   (64, 72, 128, 136, 256, 512, 1032, 2048), geoms):
        Ho = (H + 2 * p - d * (k - 1) - 1) // s + 1
        Wo = (W + 2 * p - d * (k - 1) - 1) // s + 1
        if Ho > 0 and Wo > 0:
            yield R.Problem(N, H, W, Cin, Cout, k, s, p, d, 0, Ho, Wo)


def test_every_reachable_instantiation_has_a_route(L):
    """Sweep both dispatch queries over shapes, variants, statistics and groups (1, 2, N and sub-image counts): every
    instantiation they name is in ROUTES, so a kernel added without a case fails here."""
    listed = {r.name for r in R.ROUTES}
    seen = set()
    for p in _sweep_problems():
        for variant, mode, has_stats in ((0, 0, 0), (0, 0, 1), (0, 1, 0), (1, 0, 0), (2, 0, 1), (2, 1, 1), (3, 0, 1)):
            for G in sorted({1, 2, p.N, 2 * p.N}):
                name = R.query(L, variant, p._replace(mode=mode), has_stats, G)
                if name:
                    seen.add(name)
                    if name.startswith(R.PER_KIND):     # the per-epilogue kinds the query cannot name (see conv_routes.py)
                        seen.update(name[:name.rindex(',') + 2] + '%d>' % k for k in range(7))
    for N, (H, W), Cin, Cout, (k, s, p, d) in itertools.product((1, 3), [(4, 4), (8, 16), (17, 13), (8, 32), (16, 32), (8, 64),
                                                                         (16, 64), (32, 32)],
                                                                (8, 64, 72, 128, 256), (8, 64, 72, 128, 136, 256, 512),
                                                                [(1, 1, 0, 1), (3, 1, 1, 1), (3, 1, 2, 2), (3, 2, 1, 1)]):
        Ho = (H + 2 * p - d * (k - 1) - 1) // s + 1
        Wo = (W + 2 * p - d * (k - 1) - 1) // s + 1
        name = R.wgrad_query(L, R.Problem(N, H, W, Cin, Cout, k, s, p, d, 0, Ho, Wo))
        if name:
            seen.add(name)
    assert seen - listed == set(), 'instantiations without a route: %s' % sorted(seen - listed)
    assert listed - seen == set(), 'routes the sweep never reaches (widen the sweep): %s' % sorted(listed - seen)


def test_every_route_dispatches_to_its_declared_instantiation(L):
    for r in R.ROUTES:
        assert r.calls, r
        for call, G in R.expand(r):
            assert R.route_of(L, call, r.problem, G) == r.name, (r.name, r.problem, call, G)


def test_weight_gradient_routes_split_with_the_workspace(L):
    """Every weight-gradient problem splits its K tiles when given the workspace: 'wgrad' runs the split-K combine,
    'wgrad_nows' the unsplit walk of the same layer."""
    for r in R.ROUTES:
        if 'wgrad' in r.calls:
            assert R.wgrad_workspace(L, r.problem) > R.WGRAD_WS_COUNTERS, (r.name, r.problem)


def test_sub_image_statistics_groups_are_refused(L):
    """A statistics group is a whole number of images: anything finer is refused (the query returns NULL), on every
    entry point -- also where a tile would not straddle a group, so that the contract is one rule."""
    for call, p, G in R.SUB_IMAGE:
        assert p.N % G != 0
        assert R.route_of(L, call, p, G) is None, (call, p, G)
    # rgda_conv2d_bnin_supported gives the same answer as the call (the model trusts it and does not fall back)
    from regda_amd import ops
    for call, p, G in R.SUB_IMAGE:
        if call == 'bnin':
            M = p.N * p.Ho * p.Wo
            args = (M, p.Cout, p.Cin, p.k, p.k, p.stride, p.pad, p.dil, p.H, p.W, p.Ho, p.Wo)
            assert ops.conv2d_bnin_supported(*args, G) == 0, (p, G)
            assert ops.conv2d_bnin_supported(*args, p.N) > 0, p
    # the same geometries with whole-image groups are served
    for call, p, G in R.SUB_IMAGE:
        assert R.route_of(L, call, p, p.N) is not None or R.route_of(L, call, p, 1) is not None, (call, p)


def test_grouped_launch_count_refuses_sub_image_groups(L):
    """rgda_conv2d_grouped validates every descriptor by the same rule (host tensors: nothing is launched or read)."""
    from regda_amd import ops
    p = R.P(4, 32, 64, 512, 512, 3)
    x = torch.empty(p.N * p.H * p.W, 512, dtype=torch.bfloat16)
    w = torch.empty(512, 9, 512, dtype=torch.bfloat16)
    y = torch.empty(p.N * p.Ho * p.Wo, 512, dtype=torch.bfloat16)
    stats = torch.zeros(32, 8, 2, 512, dtype=torch.int64)
    item = (x, w, y, p.N, p.H, p.W, p.Ho, p.Wo, 3, 3, 1, 1, 1, 0, None, stats)
    with pytest.raises(ValueError):
        ops.conv2d_grouped_launches([item + (32,)])
    assert ops.conv2d_grouped_launches([item + (4,)]) == 1


# ---------------------------------------------------------------- self-test of the checks


def _conv_problem():
    g = torch.Generator().manual_seed(5)
    N, H, W, Ci, Co = 2, 16, 64, 64, 32
    x = torch.randn(N, Ci, H, W, generator=g).to(torch.bfloat16).double()
    w = (torch.randn(Co, Ci, 3, 3, generator=g) * (2.0 / (Ci * 9)) ** 0.5).to(torch.bfloat16).double()
    ref = F.conv2d(x, w, None, 1, 1, 1)                              # exact (fp64) NCHW
    y = ref.to(torch.bfloat16).double()                               # what a correct kernel stores
    return x, w, ref, y


def _rows(t):
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1])


def test_checks_pass_a_correct_result():
    x, w, ref, y = _conv_problem()
    assert R.elem_violations(_rows(y), _rows(ref)) == 0
    yr = _rows(y)
    s, a = R.group_sums(yr, 2)
    assert R.stat_violations(s, *R.group_sums(yr, 2), yr.shape[0] // 2, 26) == 0


def test_checks_flag_each_injected_fault():
    x, w, ref, y = _conv_problem()
    rref = _rows(ref)
    # 1: one tap missing in one 8 x 32 tile (image 1, rows 8 - 15, columns 32 - 63)
    tap = torch.zeros_like(w)
    tap[:, :, 0, 0] = w[:, :, 0, 0]
    f1 = y.clone()
    f1[1, :, 8:16, 32:64] = (ref - F.conv2d(x, tap, None, 1, 1, 1))[1, :, 8:16, 32:64].to(torch.bfloat16).double()
    # 2: one 32-column band shifted by one image row (image 0, columns 32 - 63)
    f2 = y.clone()
    f2[0, :, 1:, 32:64] = y[0, :, :-1, 32:64]
    # 3: one channel tile (8 channels) of 4 rows scaled by 1 + 2^-7
    f3r = _rows(y).clone()
    f3r[100:104, 8:16] = (f3r[100:104, 8:16] * (1 + 2.0 ** -7)).to(torch.bfloat16).double()
    for name, fy in (('missing tap', _rows(f1)), ('shifted band', _rows(f2)), ('scaled channel tile', f3r)):
        assert R.elem_violations(fy, rref) > 0, name
    # the suite's older whole-tensor measure misses the third
    assert R.relerr(f3r, rref) < 1e-2
    # 4: one 256-row tile's statistics credited to the neighbouring group (rows 1792 - 2047 of group 0 -> group 1)
    yr = _rows(y)
    G, rpg = 2, yr.shape[0] // 2
    ref_s, ref_a = R.group_sums(yr, G)
    fix = lambda s: torch.round(s * 2.0 ** 26) * 2.0 ** -26           # the accumulators' fixed point
    good, _ = R.group_sums(yr, G)
    assert R.stat_violations(fix(good), ref_s, ref_a, rpg, 26) == 0
    moved = torch.stack([yr[rpg - 256:rpg].sum(0), (yr[rpg - 256:rpg] ** 2).sum(0)], 0)
    bad = good.clone()
    bad[0] -= moved
    bad[1] += moved
    assert R.stat_violations(fix(bad), ref_s, ref_a, rpg, 26) > 0
