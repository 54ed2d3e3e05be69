"""GPU: rgda_hist_style / rgda_hist_style_write_table (regda_amd.aug.histogram: hist_style, hist_style_write_table)
against the numpy / Python-integer restatement of the contract (tests/hist_ref.py).

What is compared, per case: hist= with np.bincount of the levels; lut= with the restatement's L, BIT-EQUAL as fp64 (exact
integers, one correctly rounded division, one addition); every output element with the fp32 x + D_ref[v] to 2^-20 absolute:
D may differ by one fp32 ulp if the compiler contracts the fp64 product, every value here is below 8 in magnitude (ulp
<= 2^-21), and one grey level is about 2^-6, so the bound cannot hide a wrong level.  Rows that are off, a twin partner
and blend_q = 0 are compared bitwise.

The tiles are uint8 levels normalised in fp32 (the round trip recovers every level: tests/test_hist_cpu.py), 'noise' adds
sub-level offsets of |.| <= 0.4, 'norms' gives source and target different normalisations.

Shapes (N, M, H, W), the smallest at which each route can go wrong: (1, 1, 1, 1) one pixel, a scalar tail only;
(2, 3, 8, 8) 16-byte groups only; (3, 2, 33, 47) planes of 1551 floats, whose bases sit at every 4-byte offset of a
16-byte line: scalar head and tail; (2, 2, 64, 64) half a workgroup's chunk; (1, 2, 192, 160) 3.75 chunks per plane."""
import numpy as np
import pytest
import torch

import hist_ref
from hist_ref import BLEND_ONE, MEAN, MEAN_T, STD, STD_T

pytestmark = pytest.mark.gpu

NORM = (MEAN, STD, MEAN, STD)
FULL = BLEND_ONE


def fill(rng, kind, shape):
    """uint8 levels of one content kind"""
    if kind == 'all':           # all 256 levels (where the plane has room)
        return rng.integers(0, 256, shape).astype(np.uint8)
    if kind == 'two':
        return rng.choice(np.array([40, 200], np.uint8), shape)
    if kind == 'const':
        return np.full(shape, 77, np.uint8)
    if kind == 'spike':         # one bin holds 99 % of the pixels
        v = np.full(shape, 128, np.uint8)
        rest = rng.random(shape) < 0.01
        v[rest] = rng.integers(0, 256, int(rest.sum()))
        return v
    if kind == 'low':
        return rng.integers(0, 60, shape).astype(np.uint8)
    if kind == 'high':
        return rng.integers(180, 256, shape).astype(np.uint8)
    raise KeyError(kind)


CASES = {       # (N, M, H, W), source kind, target kind, rows {partner, blend_q, on, 0}, norms, sub-level noise
    'pixel': ((1, 1, 1, 1), 'all', 'all', [[0, FULL, 1, 0]], NORM, False),
    'two': ((2, 3, 8, 8), 'all', 'two', [[2, FULL, 1, 0], [0, 32768, 1, 0]], NORM, False),
    'const_t': ((2, 3, 8, 8), 'all', 'const', [[1, FULL, 1, 0], [2, 12345, 1, 0]], NORM, False),
    'odd': ((3, 2, 33, 47), 'all', 'all', [[1, FULL, 1, 0], [0, FULL, 0, 0], [0, 40000, 1, 0]], NORM, False),
    'norms': ((3, 2, 33, 47), 'all', 'spike', [[0, FULL, 1, 0], [1, 50000, 1, 0], [1, FULL, 0, 0]], (MEAN, STD, MEAN_T, STD_T), False),
    'below': ((3, 2, 33, 47), 'low', 'high', [[0, FULL, 1, 0], [1, FULL, 1, 0], [0, 1, 1, 0]], NORM, False),
    'above': ((2, 2, 64, 64), 'high', 'low', [[1, FULL, 1, 0], [0, 65535, 1, 0]], NORM, False),
    'noise': ((2, 2, 64, 64), 'all', 'all', [[0, FULL, 1, 0], [1, 20000, 1, 0]], (MEAN, STD, MEAN_T, STD_T), True),
    'const_s': ((2, 2, 64, 64), 'const', 'all', [[1, FULL, 1, 0], [0, FULL, 1, 0]], NORM, False),
    'spike': ((1, 2, 192, 160), 'spike', 'all', [[1, FULL, 1, 0]], NORM, False),
    'chunks': ((1, 2, 192, 160), 'all', 'spike', [[0, FULL, 1, 0]], NORM, True),
}
_REF = {}


def case(name):
    """(xs f32, xt f32, table int32, norms, (out, hist, lut) of the restatement) of a case: made once, shared, never
    written"""
    if name not in _REF:
        (n, m, h, w), ks, kt, rows, norm, noisy = CASES[name]
        rng = np.random.default_rng(900 + sorted(CASES).index(name))
        ls, lt = fill(rng, ks, (n, 3, h, w)), fill(rng, kt, (m, 3, h, w))
        xs = hist_ref.tiles(ls, norm[0], norm[1], rng.uniform(-0.4, 0.4, ls.shape) if noisy else None)
        xt = hist_ref.tiles(lt, norm[2], norm[3], rng.uniform(-0.4, 0.4, lt.shape) if noisy else None)
        assert np.array_equal(hist_ref.levels_of(xs, norm[0], norm[1]), ls) and np.array_equal(hist_ref.levels_of(xt, norm[2], norm[3]), lt)
        table = np.asarray(rows, np.int32)
        _REF[name] = (xs, xt, table, norm, hist_ref.hist_ref(xs, xt, table, *norm))
    return _REF[name]


def run(xs, xt, table, norm, device_table=None, **kw):
    from regda_amd.aug import histogram
    sd = xs if torch.is_tensor(xs) else torch.from_numpy(xs).cuda()
    ti = xt if torch.is_tensor(xt) else torch.from_numpy(xt).cuda()
    if device_table is None:
        device_table = torch.empty(table.shape, dtype=torch.int32, device='cuda')
        histogram.hist_style_write_table(device_table, table, ti.shape[0], sd.shape[-2:])
    res = histogram.hist_style(sd, ti, device_table, *norm, **kw)
    torch.cuda.synchronize()
    assert torch.equal(device_table.cpu(), torch.from_numpy(table))
    return res


def bits(t):
    return t.view(torch.int32)


@pytest.mark.parametrize('name', sorted(CASES))
def test_histograms_levels_and_every_element_against_the_restatement(name):
    xs, xt, table, norm, (want, want_hist, want_lut) = case(name)
    n, m = xs.shape[0], xt.shape[0]
    sd, ti = torch.from_numpy(xs).cuda(), torch.from_numpy(xt).cuda()
    flag = torch.zeros(1, dtype=torch.int32, device='cuda')
    hist = torch.full((n + m, 3, 256), -1, dtype=torch.int32, device='cuda')
    lut = torch.full((n, 3, 256), -1.0, dtype=torch.float64, device='cuda')
    got = run(sd, ti, table, norm, flag=flag, hist=hist, lut=lut)
    assert torch.equal(sd.cpu(), torch.from_numpy(xs)) and torch.equal(ti.cpu(), torch.from_numpy(xt)), 'an input was written'
    assert np.array_equal(hist.cpu().numpy(), want_hist), 'hist differs from np.bincount'
    assert np.array_equal(lut.cpu().numpy().view(np.int64), want_lut.view(np.int64)), 'L is not the restatement bit for bit'
    g = got.cpu().numpy()
    for i in range(n):
        if not table[i, 2]:
            assert np.array_equal(g[i].view(np.int32), xs[i].view(np.int32)), 'image %d is not the input bit for bit' % i
            continue
        d = np.abs(g[i].astype(np.float64) - want[i].astype(np.float64)).max()
        print('%s image %d blend_q %d: max |out - ref| %.3e, change %.3f, max |x| %.2f'
              % (name, i, table[i, 1], d, np.abs(want[i] - xs[i]).max(), np.abs(want[i]).max()))
        assert np.abs(want[i]).max() < 8.0
        assert d <= 2.0 ** -20, 'image %d: |out - ref| up to %.3e' % (i, d)
    again = run(sd, ti, table, norm, flag=flag)
    assert torch.equal(bits(got), bits(again)), 'two runs differ'
    assert flag.item() == 0


def test_a_twin_partner_and_blend_zero_return_the_source():
    xs, xt, _, norm, _ = case('odd')
    sd = torch.from_numpy(xs).cuda()
    twins = torch.stack([sd[1], sd[0], sd[2]])              # source n's twin is target (1, 0, 2)[n]
    got = run(sd, twins, np.array([[1, FULL, 1, 0], [0, 30000, 1, 0], [2, 1, 1, 0]], np.int32), norm)
    assert torch.equal(got, sd) and got.data_ptr() != sd.data_ptr()
    got = run(sd, xt, np.array([[1, 0, 1, 0], [0, 0, 1, 0], [1, 0, 1, 0]], np.int32), norm)
    assert torch.equal(got, sd)
    lut = torch.empty(3, 3, 256, dtype=torch.float64, device='cuda')
    run(sd, twins, np.array([[1, FULL, 1, 0], [0, FULL, 1, 0], [2, FULL, 1, 0]], np.int32), norm, lut=lut)
    assert torch.equal(lut.cpu(), torch.arange(256.0, dtype=torch.float64).expand(3, 3, 256))


def test_a_given_workspace_and_out_and_a_misaligned_tensor_give_the_same_bits():
    from regda_amd import _lib
    xs, xt, table, norm, _ = case('noise')
    sd = torch.from_numpy(xs).cuda()
    want = run(sd, xt, table, norm)
    need = _lib.lib().size('rgda_hist_style_workspace', 2, 2, 64, 64)
    ws = torch.full((need,), 0xAB, dtype=torch.uint8, device='cuda')        # any contents on entry
    out = torch.empty_like(sd)
    assert run(sd, xt, table, norm, out=out, ws=ws) is out and torch.equal(bits(out), bits(want))
    flat, oflat = (torch.empty(xs.size + 2, dtype=torch.float32, device='cuda') for _ in range(2))
    shifted = flat[1:-1].view(xs.shape)
    shifted.copy_(sd)
    got = run(shifted, xt, table, norm, out=oflat[1:-1].view(xs.shape))                 # both 4 bytes past a boundary
    assert shifted.data_ptr() % 16 == 4 and torch.equal(bits(got), bits(want))
    got = run(shifted, xt, table, norm, out=oflat[2:].view(xs.shape))                   # source and result apart: no 16-byte route
    assert got.data_ptr() % 16 == 8 and torch.equal(bits(got), bits(want))


def test_nan_and_inf_pass_through_a_row_that_is_off():
    xs, xt, table, norm, (want, _, _) = case('odd')
    xs = xs.copy()
    xs[1, 0, 0, 0], xs[1, 1, 5, 46], xs[1, 2, 32, 46], xs[1, 0, 31, 32] = np.nan, np.inf, -np.inf, -0.0
    xs[1].view(np.int32)[2, 7, 9] = 0x7fc12345                          # a NaN with a payload
    got = run(xs, xt, table, norm).cpu().numpy()
    assert np.array_equal(got[1].view(np.int32), xs[1].view(np.int32))
    assert np.abs(got[[0, 2]] - want[[0, 2]]).max() <= 2.0 ** -20       # (NaN would fail this too)


def test_out_of_range_arguments_are_refused_before_any_launch():
    from regda_amd.aug import histogram
    xs, xt, table, norm, _ = case('odd')
    sd, ti = torch.from_numpy(xs).cuda(), torch.from_numpy(xt).cuda()
    td = torch.full(table.shape, -7, dtype=torch.int32, device='cuda')
    out = torch.full(xs.shape, -7.0, device='cuda')

    def bad(n, col, v):
        t = table.copy()
        t[n, col] = v
        return t
    for t in (bad(0, 0, 2), bad(0, 0, -1), bad(1, 1, 65537), bad(1, 1, -1), bad(0, 2, 2), bad(1, 0, 2)):
        with pytest.raises(ValueError):
            histogram.hist_style_write_table(td, t, 2, (33, 47))
    with pytest.raises(ValueError):                 # 17 images
        histogram.hist_style_write_table(torch.empty(17, 4, dtype=torch.int32, device='cuda'), np.tile(table[:1], (17, 1)), 2, (33, 47))
    with pytest.raises(ValueError):
        histogram.hist_style_write_table(td, table[:1], 2, (33, 47))
    with pytest.raises(ValueError):                 # in place
        histogram.hist_style(sd, ti, td, *norm, out=sd)
    with pytest.raises(ValueError):                 # the target as the result
        histogram.hist_style(sd[:2], ti, td[:2], *norm, out=ti)
    with pytest.raises(ValueError):                 # overlapping the source without starting where it starts
        histogram.hist_style(sd[:2], ti, td[:2], *norm, out=sd[1:])
    with pytest.raises(ValueError):                 # a view that is not contiguous
        histogram.hist_style(sd, ti, td, *norm, out=torch.empty(3, 3, 33, 94, device='cuda')[..., ::2])
    with pytest.raises(ValueError):                 # another shape
        histogram.hist_style(sd, ti, td, *norm, out=torch.empty(3, 3, 47, 33, device='cuda'))
    with pytest.raises(ValueError):
        histogram.hist_style(sd, ti, td, MEAN, (1.0, 0.0, 1.0), MEAN, STD, out=out)
    with pytest.raises(ValueError):
        histogram.hist_style(sd, ti, td.to(torch.int64), *norm, out=out)
    with pytest.raises(ValueError):                 # tiles of another size
        histogram.hist_style(sd, ti[..., :46], td, *norm, out=out)
    with pytest.raises(ValueError):
        histogram.hist_style(sd[:, :2], ti, td, *norm)
    with pytest.raises(ValueError):                 # hist of another shape, lut of another type
        histogram.hist_style(sd, ti, td, *norm, out=out, hist=torch.empty(3, 3, 256, dtype=torch.int32, device='cuda'))
    with pytest.raises(ValueError):
        histogram.hist_style(sd, ti, td, *norm, out=out, lut=torch.empty(3, 3, 256, device='cuda'))
    torch.cuda.synchronize()
    assert (td == -7).all() and (out == -7.0).all() and torch.equal(sd.cpu(), torch.from_numpy(xs))


def test_a_device_row_outside_the_served_range_copies_the_image_and_sets_the_flag():
    """a table that did not come through rgda_hist_style_write_table: the kernel cannot refuse, it copies and flags"""
    xs, xt, table, norm, _ = case('odd')
    sd, ti = torch.from_numpy(xs).cuda(), torch.from_numpy(xt).cuda()
    good = run(sd, ti, table, norm)
    for col, v in ((0, 2), (0, -1), (1, 65537), (1, -1), (2, 3), (2, -1)):     # partner, blend_q, the switch
        t = table.copy()
        t[0, col] = v
        flag = torch.zeros(1, dtype=torch.int32, device='cuda')
        lut = torch.empty(3, 3, 256, dtype=torch.float64, device='cuda')
        got = run(sd, ti, t, norm, device_table=torch.from_numpy(t).cuda(), flag=flag, lut=lut)
        assert flag.item() == 1, (col, v)
        assert torch.equal(bits(got[0]), bits(sd[0]))
        assert torch.equal(bits(got[1:]), bits(good[1:]))       # the other rows are served as before
        assert torch.equal(lut[0].cpu(), torch.arange(256.0, dtype=torch.float64).expand(3, 256))


def test_an_explicit_stream_is_used():
    from regda_amd import ops
    from regda_amd.aug import histogram
    xs, xt, table, norm, _ = case('noise')
    sd, ti = torch.from_numpy(xs).cuda(), torch.from_numpy(xt).cuda()
    want = run(sd, ti, table, norm)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with ops.use_stream(side):
        td = histogram.hist_style_write_table(torch.empty(2, 4, dtype=torch.int32, device='cuda'), table, 2, (64, 64))
        got = histogram.hist_style(sd, ti, td, *norm)
    side.synchronize()
    assert torch.equal(bits(got), bits(want))
