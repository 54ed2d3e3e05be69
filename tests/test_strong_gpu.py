"""GPU: rgda_strong_augment / rgda_strong_write_table (ops.strong_augment, ops.strong_write_table), every output element
against the fp64 restatement of the contract (tests/strong_ref.py).

Tolerance: the forward error bound strong_ref derives per element from the fp64 run -- K eps Mmax + |fc - 1| m_err,
scaled by 255 / std_c, with K = 6 + 15 j + (4 R + 4) b roundings on the longest dependency path (j, b: the jitter and
blur bits; R the blur radius: K = 6, 21, 4 R + 10, 4 R + 25; at R = 12: 58 and 73) and m_err = 9 eps Mg + 2^-25 from
the 2^-24 quantum of the image mean's integer sum.  strong_ref's docstring counts the roundings one by one.  The transform
is continuous (clamps, no selection), so no element is excluded.  An image with both bits clear is compared bitwise.

Shapes: 40 x 72 and 33 x 37 are no multiples of the 32 x 32 tile (33 x 37: partial quads, element stores, and R = 12
reaches past a third of the edge, so the reflection runs deep), 64 x 64 is whole tiles; 2 to 6 workgroups per image.
Factors sit at the ends of the default ranges and the tiles reach beyond 0..255, so each of the four clamps binds at both
ends on many elements (tests/test_strong_cpu.py asserts that of these cases)."""
import numpy as np
import pytest
import torch

import strong_ref

pytestmark = pytest.mark.gpu

TH = 2 * np.pi * 0.05
CLEAR = [1.3, 0.7, 1.3, 1.0, 2.0, 0, 0, 0]          # (values of switches that are off are not read)


def jit(fb, fc, fs, th):
    return [fb, fc, fs, th, 9.0, 1, 0, 0]


def blur(sigma):
    return [7.0, 7.0, 7.0, 7.0, sigma, 2, 0, 0]


def both(fb, fc, fs, th, sigma):
    return [fb, fc, fs, th, sigma, 3, 0, 0]


CASES = {
    'a0': ((4, 3, 40, 72), [CLEAR, jit(1.2, 1.2, 1.2, TH), blur(1.15), both(0.8, 1.2, 1.2, -TH, 4.0)]),
    'a1': ((4, 3, 40, 72), [both(1.2, 0.8, 1.2, -TH, 0.15), blur(4.0), jit(0.8, 1.2, 0.8, TH), CLEAR]),
    'b0': ((3, 3, 33, 37), [blur(4.0), both(1.2, 1.2, 0.8, TH, 4.0), CLEAR]),
    'b1': ((3, 3, 33, 37), [jit(1.2, 0.8, 1.2, -TH), both(0.8, 1.2, 1.2, TH, 0.15), blur(1.15)]),
    'c0': ((2, 3, 64, 64), [both(1.2, 1.2, 1.2, TH, 1.15), CLEAR]),
    'c1': ((2, 3, 64, 64), [jit(0.8, 1.2, 0.8, -TH), blur(4.0)]),
}
_REF = {}


def case(name):
    """(x f32, table f32, fp64 result, bound) of a case: made once, shared, never written"""
    if name not in _REF:
        shape, rows = CASES[name]
        rng = np.random.default_rng(sorted(CASES).index(name))
        raw = rng.uniform(-20.0, 275.0, shape)      # about 7 % of the values beyond each end of 0..255: the first clamp binds
        raw *= rng.uniform(0.3, 1.0, (shape[0], 1, shape[2], shape[3]))     # dark and bright pixels, coloured ones
        mean, std = np.asarray(strong_ref.MEAN)[:, None, None], np.asarray(strong_ref.STD)[:, None, None]
        x = ((raw - mean) / std).astype(np.float32)
        table = np.asarray(rows, np.float32)
        out, err = strong_ref.strong_ref(x, table, bound=True)
        _REF[name] = (x, table, out, err)
    return _REF[name]


def run(x, table, out=None, **kw):
    from regda_amd import ops
    xd = x if torch.is_tensor(x) else torch.from_numpy(x).cuda()
    td = torch.empty(table.shape, dtype=torch.float32, device='cuda')
    ops.strong_write_table(td, table, xd.shape[-2:])
    res = ops.strong_augment(xd, td, strong_ref.MEAN, strong_ref.STD, out=out, **kw)
    torch.cuda.synchronize()
    assert torch.equal(td.cpu(), torch.from_numpy(table))
    return res


def compare(got, name):
    x, table, want, err = case(name)
    got = got.cpu().numpy()
    for n in range(x.shape[0]):
        flags = int(table[n, 5])
        if not flags:
            assert np.array_equal(got[n].view(np.int32), x[n].view(np.int32)), 'image %d is not the input bit for bit' % n
            continue
        d = np.abs(got[n].astype(np.float64) - want[n])
        ratio = float((d / err[n]).max())
        print('%s image %d flags %d: max |d| %.3e, max bound %.3e, max |d| / bound %.3f'
              % (name, n, flags, d.max(), err[n].max(), ratio))
        assert err[n].max() < 2e-4 and np.abs(want[n] - x[n]).max() > 0.05      # a tight bound on a visible change
        assert (d <= err[n]).all(), 'image %d: |d| / bound up to %.3f' % (n, ratio)


@pytest.mark.parametrize('name', sorted(CASES))
def test_every_element_against_the_fp64_restatement(name):
    x, table, want, _ = case(name)
    xd = torch.from_numpy(x).cuda()
    got = run(xd, table)
    assert torch.equal(xd.cpu(), torch.from_numpy(x)), 'the input was written'
    compare(got, name)
    again = run(xd, table)
    assert torch.equal(got.view(torch.int32), again.view(torch.int32)), 'two runs differ'


def test_the_element_route_of_a_misaligned_tensor_gives_the_same_bits():
    x, table, _, _ = case('c0')
    xd = torch.from_numpy(x).cuda()
    want = run(xd, table)
    flat = torch.empty(x.size + 1, dtype=torch.float32, device='cuda')
    shifted = flat[1:].view(x.shape)
    shifted.copy_(xd)
    oflat = torch.empty(x.size + 1, dtype=torch.float32, device='cuda')
    got = run(shifted, table, out=oflat[1:].view(x.shape))
    assert shifted.data_ptr() % 16 == 4 and torch.equal(got.view(torch.int32), want.view(torch.int32))


def test_nan_and_inf_pass_through_an_image_with_both_bits_clear():
    x, table, _, _ = case('c0')
    x = x.copy()
    x[1, 0, 0, 0], x[1, 1, 5, 63], x[1, 2, 63, 63], x[1, 0, 31, 32] = np.nan, np.inf, -np.inf, -0.0
    x[1].view(np.int32)[2, 7, 9] = 0x7fc12345                          # a NaN with a payload
    got = run(x, table).cpu().numpy()
    assert np.array_equal(got[1].view(np.int32), x[1].view(np.int32))
    assert np.isfinite(got[0]).all()


def test_out_of_range_arguments_are_refused_before_any_launch():
    from regda_amd import ops
    x, table, _, _ = case('b0')
    xd = torch.from_numpy(x).cuda()
    td = torch.full(table.shape, -7.0, device='cuda')
    out = torch.full(x.shape, -7.0, device='cuda')

    def bad(n, col, v):
        t = table.copy()
        t[n, col] = v
        return t
    for t in (bad(0, 4, 4.5), bad(0, 4, 0.0), bad(1, 0, np.nan), bad(2, 5, 4.0)):
        with pytest.raises(ValueError):
            ops.strong_write_table(td, t, (33, 37))
    with pytest.raises(ValueError):                 # R = 12 does not fit a 12-pixel edge
        ops.strong_write_table(td, table, (12, 37))
    with pytest.raises(ValueError):                 # 17 images
        ops.strong_write_table(torch.empty(17, 8, device='cuda'), np.tile(table[:1], (17, 1)), (33, 37))
    with pytest.raises(ValueError):
        ops.strong_write_table(td, table[:2], (33, 37))
    with pytest.raises(ValueError):                 # in place
        ops.strong_augment(xd, td, strong_ref.MEAN, strong_ref.STD, out=xd)
    with pytest.raises(ValueError):
        ops.strong_augment(xd, td, strong_ref.MEAN, (1.0, 0.0, 1.0), out=out)
    with pytest.raises(ValueError):
        ops.strong_augment(xd, td.to(torch.float64), strong_ref.MEAN, strong_ref.STD, out=out)
    with pytest.raises(ValueError):
        ops.strong_augment(xd[:, :2], td, strong_ref.MEAN, strong_ref.STD)
    torch.cuda.synchronize()
    assert (td == -7.0).all() and (out == -7.0).all() and torch.equal(xd.cpu(), torch.from_numpy(x))


def test_a_device_row_outside_the_served_range_copies_the_image_and_sets_the_flag():
    """a table that did not come through rgda_strong_write_table: the kernel cannot refuse, it copies and flags"""
    from regda_amd import ops
    x, table, _, _ = case('c0')
    xd = torch.from_numpy(x).cuda()
    t = table.copy()
    t[0, 4] = 5.0               # sigma above 4 with both bits set
    flag = torch.zeros(1, dtype=torch.int32, device='cuda')
    got = ops.strong_augment(xd, torch.from_numpy(t).cuda(), strong_ref.MEAN, strong_ref.STD, flag=flag)
    torch.cuda.synchronize()
    assert flag.item() == 1 and torch.equal(got.view(torch.int32), xd.view(torch.int32))
    flag.zero_()
    ops.strong_augment(xd, torch.from_numpy(table).cuda(), strong_ref.MEAN, strong_ref.STD, flag=flag)
    assert flag.item() == 0
