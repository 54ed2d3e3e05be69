"""GPU: rgda_fourier_style / rgda_fourier_style_write_table (ops.fourier_style, ops.fourier_style_write_table), every output
element against the fp64 restatement of the contract through numpy.fft (tests/fourier_ref.py), which is not the kernel's
algorithm.

Tolerance: the per-element bound fourier_ref derives from the fp64 run (its docstring counts the roundings and says why it
is six standard deviations of a rounding model and not a worst case); tests/test_fourier_cpu.py asserts, without a GPU, that
on these cases it stays below 0.05 grey levels, that |F_T| / |F_S| stays below 256 on every swapped bin and that a float32
numpy evaluation of the kernel's form lies inside it.  One wrong bin moves pixels by about a grey level.  The transform
is continuous, so no element is excluded.  A row that is off is compared bitwise.

Shapes, the smallest at which each route can go wrong:
  a0, a1  3 + 2 tiles of 40 x 72, b = 0, 3, 19: a non-square tile, no multiple of the 64 lanes or of 256; b = 19 swaps 39 of
          the 40 rows of the spectrum, the widest window that fits; one row off in each
  b0      2 + 2 tiles of 33 x 37, b = 2, 16: odd sizes, the element route (W % 4 != 0), 2b + 1 = H exactly, a last row
          group of one row
  c0      2 + 3 tiles of 64 x 64, b = 5, 31: every bin but Nyquist; the source and the target carry different
          normalisations; both rows take target 2, so targets 0 and 1 are the partner of none and are not transformed
  d0      1 + 1 tile of 132 x 136, b = 64: the cap; up to three terms per lane in both analysis passes, a last row group
          of four rows, 65 twiddle rows and 129 x 65 bins per plane
  e0      1 + 1 tile of 10 x 2100, b = 4: a row wider than 2048, where the eight staged rows of the row analysis pass 64 KB
          of LDS and the launch takes the route that raises the kernel's limit; 33 terms per lane, a last row group of two"""
import numpy as np
import pytest
import torch

import fourier_ref
from fourier_ref import MEAN, MEAN_T, STD, STD_T

pytestmark = pytest.mark.gpu

NORM = (MEAN, STD, MEAN, STD)
CASES = {       # source shape, target images, rows {partner, b, on, 0}, (mean_s, std_s, mean_t, std_t)
    'a0': ((3, 3, 40, 72), 2, [[1, 0, 1, 0], [0, 3, 0, 0], [0, 19, 1, 0]], NORM),
    'a1': ((3, 3, 40, 72), 2, [[0, 3, 1, 0], [1, 19, 1, 0], [1, 0, 0, 0]], NORM),
    'b0': ((2, 3, 33, 37), 2, [[1, 2, 1, 0], [0, 16, 1, 0]], NORM),
    'c0': ((2, 3, 64, 64), 3, [[2, 5, 1, 0], [2, 31, 1, 0]], (MEAN, STD, MEAN_T, STD_T)),
    'd0': ((1, 3, 132, 136), 1, [[0, 64, 1, 0]], NORM),
    'e0': ((1, 3, 10, 2100), 1, [[0, 4, 1, 0]], NORM),
}
_REF = {}


def tiles(rng, shape, mean, std):
    """seeded uniform noise times a per-pixel brightness field shared by the channels, normalised"""
    raw = rng.uniform(0.0, 255.0, shape) * rng.uniform(0.3, 1.0, (shape[0], 1, shape[2], shape[3]))
    return ((raw - np.asarray(mean)[:, None, None]) / np.asarray(std)[:, None, None]).astype(np.float32)


def case(name):
    """(xs f32, xt f32, table int32, norms, fp64 result, bound) of a case: made once, shared, never written.  The seeds are
    such that |F_T| / |F_S| <= 256 on every swapped bin (tests/test_fourier_cpu.py asserts it): among the 50 000 bins of
    the cap case about every other draw of white noise has a source bin that close to zero."""
    if name not in _REF:
        shape, m, rows, norm = CASES[name]
        rng = np.random.default_rng(400 + sorted(CASES).index(name))
        xs = tiles(rng, shape, norm[0], norm[1])
        xt = tiles(rng, (m,) + shape[1:], norm[2], norm[3])
        table = np.asarray(rows, np.int32)
        out, err = fourier_ref.fourier_ref(xs, xt, table, *norm, bound=True)
        _REF[name] = (xs, xt, table, norm, out, err)
    return _REF[name]


def run(xs, xt, table, norm, out=None, **kw):
    from regda_amd import ops
    sd = xs if torch.is_tensor(xs) else torch.from_numpy(xs).cuda()
    td_img = xt if torch.is_tensor(xt) else torch.from_numpy(xt).cuda()
    td = torch.empty(table.shape, dtype=torch.int32, device='cuda')
    ops.fourier_style_write_table(td, table, td_img.shape[0], sd.shape[-2:])
    res = ops.fourier_style(sd, td_img, td, *norm, out=out, **kw)
    torch.cuda.synchronize()
    assert torch.equal(td.cpu(), torch.from_numpy(table))
    return res


def compare(got, name):
    xs, _, table, norm, want, err = case(name)
    got = got.cpu().numpy()
    grey = np.asarray(norm[1], np.float32).astype(np.float64)[:, None, None]       # result units -> grey levels
    for n in range(xs.shape[0]):
        if not table[n, 2]:
            assert np.array_equal(got[n].view(np.int32), xs[n].view(np.int32)), 'image %d is not the input bit for bit' % n
            continue
        d = np.abs(got[n].astype(np.float64) - want[n])
        ratio = float((d / err[n]).max())
        print('%s image %d b %d: max |d| %.3e grey, max bound %.3e grey, max |d| / bound %.3f, change %.1f grey'
              % (name, n, table[n, 1], (d * grey).max(), (err[n] * grey).max(), ratio, (np.abs(want[n] - xs[n]) * grey).max()))
        assert (np.abs(want[n] - xs[n]) * grey).max() > 1.0         # a visible change
        assert (d <= err[n]).all(), 'image %d: |d| / bound up to %.3f' % (n, ratio)


@pytest.mark.parametrize('name', sorted(CASES))
def test_every_element_against_the_fp64_restatement(name):
    xs, xt, table, norm, _, _ = case(name)
    sd, td = torch.from_numpy(xs).cuda(), torch.from_numpy(xt).cuda()
    flag = torch.zeros(1, dtype=torch.int32, device='cuda')
    got = run(sd, td, table, norm, flag=flag)
    assert torch.equal(sd.cpu(), torch.from_numpy(xs)) and torch.equal(td.cpu(), torch.from_numpy(xt)), 'an input was written'
    compare(got, name)
    again = run(sd, td, table, norm, flag=flag)
    assert torch.equal(got.view(torch.int32), again.view(torch.int32)), 'two runs differ'
    assert flag.item() == 0


def test_a_given_workspace_and_out_and_a_misaligned_tensor_give_the_same_bits():
    from regda_amd import _lib
    xs, xt, table, norm, _, _ = case('c0')
    sd = torch.from_numpy(xs).cuda()
    want = run(sd, xt, table, norm)
    need = _lib.lib().size('rgda_fourier_style_workspace', 2, 3, 64, 64)
    ws = torch.full((need,), 0xAB, dtype=torch.uint8, device='cuda')        # any contents on entry
    out = torch.empty_like(sd)
    assert run(sd, xt, table, norm, out=out, ws=ws) is out and torch.equal(out.view(torch.int32), want.view(torch.int32))
    flat, oflat = (torch.empty(xs.size + 1, dtype=torch.float32, device='cuda') for _ in range(2))
    shifted = flat[1:].view(xs.shape)
    shifted.copy_(sd)
    got = run(shifted, xt, table, norm, out=oflat[1:].view(xs.shape))
    assert shifted.data_ptr() % 16 == 4 and torch.equal(got.view(torch.int32), want.view(torch.int32))


def test_nan_and_inf_pass_through_a_row_that_is_off():
    xs, xt, table, norm, _, _ = case('a0')
    xs = xs.copy()
    xs[1, 0, 0, 0], xs[1, 1, 5, 71], xs[1, 2, 39, 71], xs[1, 0, 31, 32] = np.nan, np.inf, -np.inf, -0.0
    xs[1].view(np.int32)[2, 7, 9] = 0x7fc12345                          # a NaN with a payload
    got = run(xs, xt, table, norm).cpu().numpy()
    assert np.array_equal(got[1].view(np.int32), xs[1].view(np.int32))
    assert np.isfinite(got[0]).all() and np.isfinite(got[2]).all()


def test_out_of_range_arguments_are_refused_before_any_launch():
    from regda_amd import ops
    xs, xt, table, norm, _, _ = case('b0')
    sd, td_img = torch.from_numpy(xs).cuda(), torch.from_numpy(xt).cuda()
    td = torch.full(table.shape, -7, dtype=torch.int32, device='cuda')
    out = torch.full(xs.shape, -7.0, device='cuda')

    def bad(n, col, v):
        t = table.copy()
        t[n, col] = v
        return t
    for t in (bad(0, 0, 2), bad(0, 0, -1), bad(1, 1, 17), bad(1, 1, -1), bad(0, 2, 2), bad(0, 1, 65)):
        with pytest.raises(ValueError):
            ops.fourier_style_write_table(td, t, 2, (33, 37))
    with pytest.raises(ValueError):                 # 2 * 16 + 1 does not fit a 32-pixel edge
        ops.fourier_style_write_table(td, table, 2, (32, 37))
    with pytest.raises(ValueError):                 # 17 images
        ops.fourier_style_write_table(torch.empty(17, 4, dtype=torch.int32, device='cuda'), np.tile(table[:1], (17, 1)), 2, (33, 37))
    with pytest.raises(ValueError):
        ops.fourier_style_write_table(td, table[:1], 2, (33, 37))
    with pytest.raises(ValueError):                 # in place
        ops.fourier_style(sd, td_img, td, *norm, out=sd)
    with pytest.raises(ValueError):                 # a view that is not contiguous
        ops.fourier_style(sd, td_img, td, *norm, out=torch.empty(2, 3, 33, 74, device='cuda')[..., ::2])
    with pytest.raises(ValueError):                 # another shape
        ops.fourier_style(sd, td_img, td, *norm, out=torch.empty(2, 3, 37, 33, device='cuda'))
    with pytest.raises(ValueError):
        ops.fourier_style(sd, td_img, td, MEAN, (1.0, 0.0, 1.0), MEAN, STD, out=out)
    with pytest.raises(ValueError):
        ops.fourier_style(sd, td_img, td.to(torch.int64), *norm, out=out)
    with pytest.raises(ValueError):                 # tiles of another size
        ops.fourier_style(sd, td_img[..., :36], td, *norm, out=out)
    with pytest.raises(ValueError):
        ops.fourier_style(sd[:, :2], td_img, td, *norm)
    torch.cuda.synchronize()
    assert (td == -7).all() and (out == -7.0).all() and torch.equal(sd.cpu(), torch.from_numpy(xs))


def test_a_device_row_outside_the_served_range_copies_the_image_and_sets_the_flag():
    """a table that did not come through rgda_fourier_style_write_table: the kernel cannot refuse, it copies and flags"""
    from regda_amd import ops
    xs, xt, table, norm, _, _ = case('b0')
    sd, td_img = torch.from_numpy(xs).cuda(), torch.from_numpy(xt).cuda()
    good = ops.fourier_style(sd, td_img, torch.from_numpy(table).cuda(), *norm)
    for col, v in ((0, 2), (1, 17), (1, -1), (2, 3)):      # partner, a b that does not fit 33 rows, a negative b, the switch
        t = table.copy()
        t[0, col] = v
        flag = torch.zeros(1, dtype=torch.int32, device='cuda')
        got = ops.fourier_style(sd, td_img, torch.from_numpy(t).cuda(), *norm, flag=flag)
        torch.cuda.synchronize()
        assert flag.item() == 1, (col, v)
        assert torch.equal(got[0].view(torch.int32), sd[0].view(torch.int32))
        assert torch.equal(got[1].view(torch.int32), good[1].view(torch.int32))        # the other row is served as before
