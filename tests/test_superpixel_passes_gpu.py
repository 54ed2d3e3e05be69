"""GPU: every kernel of regda_amd/csrc/superpixel_kernels.hip, bit for bit against the numpy restatement of the
specification (tests/superpixel_ref.py), on the case table of tests/superpixel_cases.py -- each case is there for one
path of the kernels (a cell-block geometry, an unaligned staging row, a residue of the buffer rotation, a pass of the
root-scan loop, ...), and tests/test_superpixel_cases_cpu.py proves that it reaches it.  Then the workspace contract,
the paths of the ops.superpixels wrapper, and rgda_region_shrink at its window, shape and id limits.

Nothing here has a tolerance: the centres of the last Assign, the counts and the region maps are compared with
array_equal, in that order, so that a failure names the first stage that went wrong."""
import numpy as np
import pytest
import torch

import superpixel_cases as C
from regda_amd import ops

pytestmark = pytest.mark.gpu


def _need(n, h, w, S):
    return ops.lib().size('rgda_superpixels_workspace', n, h, w, S)


def _run(imgs, c, ws=None, out=None):
    """-> regs [N][H][W], count [N] as numpy, and the workspace's centres of the last Assign [N][K][5]."""
    t = imgs if torch.is_tensor(imgs) else torch.from_numpy(np.stack(imgs)).cuda()
    n, h, w, _ = t.shape
    if ws is None:
        ws = torch.empty(_need(n, h, w, c.S), dtype=torch.uint8, device='cuda')
    regs, count = ops.superpixels(t, c.S, c.m, c.iters, c.min_area, ws=ws, out=out)
    torch.cuda.synchronize()
    k = (h // c.S) * (w // c.S)
    centres = ws[:2 * n * k * 5 * 4].view(torch.int32).view(2, n, k, 5)[c.iters & 1]
    return regs.cpu().numpy(), count.cpu().numpy(), centres.cpu().numpy()


def _equal(got, name, images=None):
    """The stages in order: centres of the last Assign, count, regs."""
    regs, count, centres = got
    want = C.oracle(name)
    want = want if images is None else [want[i] for i in images]
    assert regs.dtype == np.int32 and count.dtype == np.int32 and len(regs) == len(count) == len(want)
    for i, o in enumerate(want):
        if centres is not None:
            assert np.array_equal(centres[i], o.centres), '%s image %d: centres of the last Assign differ' % (name, i)
        assert int(count[i]) == o.count, '%s image %d: count' % (name, i)
        assert np.array_equal(regs[i], o.regs), '%s image %d: regs' % (name, i)


@pytest.mark.parametrize('name', [c.name for c in C.CASES])
def test_case(name):
    _equal(_run(C.images(name), C.BY_NAME[name]), name)


@pytest.mark.parametrize('name', C.BATCH_CASES)
def test_batch_equals_single_calls(name):
    c = C.BY_NAME[name]
    regs, count, centres = _run(C.images(name), c)
    for i, img in enumerate(C.images(name)):
        r1, c1, t1 = _run([img], c)
        assert np.array_equal(centres[i], t1[0]) and count[i] == c1[0] and np.array_equal(regs[i], r1[0]), (name, i)
        _equal((r1, c1, t1), name, images=[i])


@pytest.mark.parametrize('name', ['batch3_s5', 'iters3', 'min_area_all'])
def test_workspace_full_of_ones(name):
    """The workspace is cleared inside the call where it has to be: 0xFF in every byte (-1 in every centre, sum, label,
    parent, area and chunk count) changes nothing."""
    c = C.BY_NAME[name]
    imgs = C.images(name)
    h, w, _ = imgs[0].shape
    ws = torch.full((_need(len(imgs), h, w, c.S),), 0xFF, dtype=torch.uint8, device='cuda')
    _equal(_run(imgs, c, ws=ws), name)


def test_workspace_reused_across_shapes():
    """One workspace tensor: a large shape, a smaller one (whose buffers lie where the first call's centres, sums and
    labels were), the large one again, and a run with fewer iterations after one with more."""
    big, small = C.BY_NAME['s48'], C.BY_NAME['batch3_s5']
    h, w, _ = C.images('s48')[0].shape
    ws = torch.empty(_need(1, h, w, big.S), dtype=torch.uint8, device='cuda')
    assert ws.numel() > _need(3, 35, 45, small.S)
    for name in ('s48', 'batch3_s5', 's48', 'iters7', 'iters2', 'iters1', 'min_area_1', 'min_area_all', 's5'):
        c = C.BY_NAME[name]
        imgs = C.images(name)
        assert ws.numel() >= _need(len(imgs), *imgs[0].shape[:2], c.S)
        _equal(_run(imgs, c, ws=ws), name)


def test_unusable_workspace_is_replaced():
    """A workspace one byte short, and one that starts 4 bytes off the 16-byte alignment, never reach the kernels: the
    wrapper takes a workspace of its own, the result is the same and the caller's bytes are untouched."""
    name = 's5'
    c = C.BY_NAME[name]
    img = torch.from_numpy(np.stack(C.images(name))).cuda()
    need = _need(1, 35, 45, c.S)
    short = torch.full((need - 1,), 0xAB, dtype=torch.uint8, device='cuda')
    regs, count = ops.superpixels(img, c.S, c.m, c.iters, c.min_area, ws=short)
    _equal((regs.cpu().numpy(), count.cpu().numpy(), None), name)
    assert bool((short == 0xAB).all())
    buf = torch.full((need + 32,), 0xAB, dtype=torch.uint8, device='cuda')
    off = (-buf.data_ptr()) % 16 + 4
    shifted = buf[off:off + need]
    assert shifted.data_ptr() % 16 == 4 and shifted.numel() == need
    regs, count = ops.superpixels(img, c.S, c.m, c.iters, c.min_area, ws=shifted)
    _equal((regs.cpu().numpy(), count.cpu().numpy(), None), name)
    assert bool((buf == 0xAB).all())


def test_out_is_written_in_place_and_returned():
    name = 'batch3_s5'
    c = C.BY_NAME[name]
    img = torch.from_numpy(np.stack(C.images(name))).cuda()
    regs = torch.full((3, 35, 45), -5, dtype=torch.int32, device='cuda')
    count = torch.full((3,), -5, dtype=torch.int32, device='cuda')
    r, n = ops.superpixels(img, c.S, c.m, c.iters, c.min_area, out=(regs, count))
    assert r is regs and n is count
    _equal((regs.cpu().numpy(), count.cpu().numpy(), None), name)
    # one of the two given: the other is allocated
    r2, n2 = ops.superpixels(img, c.S, c.m, c.iters, c.min_area, out=(None, count))
    assert n2 is count and r2 is not regs and torch.equal(r2, regs)


@pytest.mark.parametrize('name', ['s5', 'batch3_s5', 's33_m1'])
def test_image_view_at_an_odd_byte_offset(name):
    """A contiguous view that starts 1 .. 3 bytes into a larger uint8 buffer: the wrapper clones it (the kernel reads
    dwords from a 4-byte aligned base) and the result is that of the contiguous copy."""
    c = C.BY_NAME[name]
    imgs = np.stack(C.images(name))
    for off in (1, 2, 3):
        buf = torch.full((imgs.size + 8,), 0x5A, dtype=torch.uint8, device='cuda')
        start = (-buf.data_ptr()) % 4 + off
        view = buf[start:start + imgs.size].view(imgs.shape)
        view.copy_(torch.from_numpy(imgs))
        assert view.data_ptr() % 4 == off and view.is_contiguous()
        _equal(_run(view, c), name)
        assert bool((buf[:start] == 0x5A).all()) and bool((buf[start + imgs.size:] == 0x5A).all())
        assert np.array_equal(view.cpu().numpy(), imgs)


@pytest.mark.parametrize('name', ['iters6', 'batch2_s33', 'wide'])
def test_two_calls_are_bit_identical(name):
    c = C.BY_NAME[name]
    a, b = _run(C.images(name), c), _run(C.images(name), c)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))


# ---------------------------------------------------------------- region_shrink
@pytest.mark.parametrize('win', C.SHRINK_WINS)
def test_region_shrink(win):
    """Every shape of the table (1 x 1, one row, one column, one pixel past / short of a tile, a window larger than the
    image, a full tile grid, a batch at a non-tile shape) at every fill; ids and fills include negatives and both int32
    limits; [H][W] and [N][H][W] inputs; the input is left as it was."""
    for shape in C.SHRINK_SHAPES:
        regs = C.shrink_map(shape)
        src = torch.from_numpy(regs.copy()).cuda()
        for fill in C.shrink_fills(regs):
            out = ops.region_shrink(src, win, fill)
            assert out.dtype == torch.int32 and out.data_ptr() != src.data_ptr()
            assert np.array_equal(out.cpu().numpy(), C.shrink_oracle(shape, win, fill)), (shape, win, fill)
            assert np.array_equal(src.cpu().numpy(), regs), (shape, win, fill)
            if win == 0:
                assert torch.equal(out, src)
        if shape[0] == 1:
            out = ops.region_shrink(src[0], win, -7)
            assert out.dim() == 2 and np.array_equal(out.cpu().numpy(), C.shrink_oracle(shape, win, -7)[0])
