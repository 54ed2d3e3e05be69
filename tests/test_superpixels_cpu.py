"""CPU: region maps without SAM (rgda_superpixels, rgda_region_shrink, regda_amd.gast.superpixels) -- the numpy
restatement of edge_shrinking against the reference's own loop (tests/golden/edge_shrink.npz), the argument errors of the
three entry points, the workspace query, and the invariants of the specification's restatement on its own outputs."""
import ctypes

import numpy as np
import pytest

import superpixel_ref as R
from regda_amd import _lib


def test_numpy_shrink_equals_the_reference_golden(gold):
    g = gold('edge_shrink.npz')
    fill = int(g['fill'])
    assert fill == R.reference_fill(48, 48, 16) == 9
    for name in ('grid', 'thin', 'blocky'):
        assert g[name].shape == (48, 48) and g[name].dtype == np.int32
        for win in (1, 3):
            want = g['%s_win%d' % (name, win)]
            assert (want != g[name]).any() and (want == g[name]).any(), (name, win)     # the case shrinks something, not all
            assert np.array_equal(R.shrink(g[name], win, fill), want), (name, win)


def _addr():
    buf = ctypes.create_string_buffer(64)
    f = ctypes.addressof(buf)           # 16-byte aligned host address: never dereferenced, the checks fail first
    return buf, f + (-f) % 16


def test_superpixels_argument_errors_without_a_gpu():
    L = _lib.lib()
    buf, f = _addr()
    names = ['img', 'N', 'H', 'W', 'S', 'm', 'iters', 'min_area', 'regs_out', 'count_out', 'ws', 'ws_bytes', 'stream']
    big = 1 << 40
    good = dict(img=f, N=2, H=64, W=96, S=16, m=10, iters=3, min_area=64, regs_out=f, count_out=f, ws=f, ws_bytes=big,
                stream=None)

    def call(**kw):
        a = dict(good, **kw)
        L.call('rgda_superpixels', *[(a[k] or None) if k in ('img', 'regs_out', 'count_out', 'ws') else a[k]
                                     for k in names])
    for kw in (dict(img=0), dict(regs_out=0), dict(count_out=0), dict(ws=0),                  # null pointers
               dict(H=65), dict(W=100), dict(S=3), dict(S=65, H=65, W=65), dict(m=65), dict(m=0),
               dict(iters=0), dict(min_area=0), dict(N=0), dict(H=0), dict(img=f + 1), dict(ws=f + 4),
               dict(H=16400, S=8), dict(N=65536)):
        with pytest.raises(ValueError):
            call(**kw)
    with pytest.raises(ValueError, match='not supported'):
        call(S=3, H=63, W=96)
    with pytest.raises(ValueError, match='not supported'):
        call(m=65)
    need = L.size('rgda_superpixels_workspace', 2, 64, 96, 16)
    assert need > 0
    with pytest.raises(_lib.RgdaError, match='workspace'):
        call(ws_bytes=need - 1)
    with pytest.raises(_lib.RgdaError, match='workspace'):
        call(ws_bytes=0)
    del buf


def test_region_shrink_argument_errors_without_a_gpu():
    L = _lib.lib()
    buf, f = _addr()
    for args in ((None, 1, 48, 48, 3, 0, f + 16, None), (f, 1, 48, 48, 3, 0, None, None), (f, 1, 48, 48, 3, 0, f, None),
                 (f, 0, 48, 48, 3, 0, f + 16, None), (f, 1, 0, 48, 3, 0, f + 16, None), (f, 1, 48, 48, -1, 0, f + 16, None),
                 (f + 2, 1, 48, 48, 3, 0, f + 16, None)):
        with pytest.raises(ValueError):
            L.call('rgda_region_shrink', *args)
    with pytest.raises(ValueError, match='not supported'):
        L.call('rgda_region_shrink', f, 1, 48, 48, 9, 0, f + 16, None)
    del buf


def test_workspace_query():
    """0 for a shape the generator does not serve; strictly monotone in N; it holds what the layout says it holds."""
    L = _lib.lib()
    q = lambda *a: L.size('rgda_superpixels_workspace', *a)
    for bad in ((0, 64, 64, 16), (1, 64, 64, 3), (1, 64, 64, 65), (1, 60, 64, 16), (1, 64, 60, 16), (1, 16400, 64, 8),
                (1, 0, 64, 16), (65536, 64, 64, 16)):
        assert q(*bad) == 0, bad
    sizes = [q(n, 64, 96, 8) for n in range(1, 9)]
    assert all(b > a for a, b in zip(sizes, sizes[1:])), sizes
    # centres[2][N][K][5], sums[3][N][K][6], three int32 maps, one count per 1024-pixel chunk
    n, h, w, s = 3, 64, 96, 8
    k = (h // s) * (w // s)
    floor = 4 * (n * k * (2 * 5 + 3 * 6) + 3 * n * h * w + n * -(-h * w // 1024))
    assert floor <= q(n, h, w, s) <= floor + 6 * 16
    assert q(8, 512, 512, 16) < 32 << 20


def _flood(labels):
    """Independent of superpixel_ref.components: the 4-connected components of equal labels by a stack flood fill, in
    raster order -> (component index per pixel, [first pixel], [area])."""
    H, W = labels.shape
    comp = -np.ones((H, W), np.int64)
    first, area = [], []
    for y0 in range(H):
        for x0 in range(W):
            if comp[y0, x0] >= 0:
                continue
            c, l, stack, a = len(first), labels[y0, x0], [(y0, x0)], 0
            comp[y0, x0] = c
            while stack:
                y, x = stack.pop()
                a += 1
                for yy, xx in ((y - 1, x), (y + 1, x), (y, x - 1), (y, x + 1)):
                    if 0 <= yy < H and 0 <= xx < W and comp[yy, xx] < 0 and labels[yy, xx] == l:
                        comp[yy, xx] = c
                        stack.append((yy, xx))
            first.append(y0 * W + x0)
            area.append(a)
    return comp, np.array(first), np.array(area)


@pytest.mark.parametrize('case', ['noise', 'diagonal', 'scene'])
def test_restatement_invariants(case):
    """On the restatement's own outputs: ids dense 1..R, every kept region one 4-connected component of equal labels with
    area >= min_area, region 0 exactly the pixels of the dropped components, count == regs.max(), numbering in root order."""
    img, S, min_area, iters = dict(noise=(R.blurred_noise(64, 96, 1), 8, 16, 10), diagonal=(R.diagonal_image(), 16, 64, 5),
                                   scene=(R.rectangle_scene(96, 64, 3, count=12), 16, 40, 4))[case]
    labels, _ = R.slic_labels(img, S, 10, iters)
    regs, count = R.superpixels(img, S, 10, iters, min_area)
    assert regs.dtype == np.int32 and regs.shape == img.shape[:2]
    comp, first, area = _flood(labels)
    assert np.array_equal(first[comp], R.components(labels))                 # min-index roots
    kept = area >= min_area
    assert count == int(kept.sum()) == int(regs.max())
    assert np.array_equal(np.unique(regs[regs > 0]), np.arange(1, count + 1))
    assert np.array_equal(regs == 0, ~kept[comp])
    want = np.zeros(len(first), np.int64)
    want[kept] = np.arange(1, count + 1)                                    # raster order of first pixels = root order
    assert np.array_equal(regs, want[comp])
    if case == 'noise':
        assert (~kept).sum() >= 1 and count >= 8


def test_constant_image_follows_the_tie_rule():
    """A constant image leaves the position term alone.  Update rounds half up, so the first centres sit at 8 g + 4 and
    the pixel rows / columns 8 g + 8 are at equal distance from the cells g and g + 1: the smaller k takes them."""
    img = np.full((32, 32, 3), 77, np.uint8)
    labels, centres = R.slic_labels(img, 8, 10, 1)
    assert np.array_equal(centres[:, :2].reshape(4, 4, 2)[:, :, 0], np.repeat(np.arange(4) * 8 + 4, 4).reshape(4, 4))
    cell = np.maximum(np.arange(32) - 1, 0) // 8
    assert np.array_equal(labels, cell[:, None] * 4 + cell[None, :])


def test_python_surface_without_a_gpu():
    from regda_amd import ops
    from regda_amd.gast.superpixels import SuperPixelsSLIC
    from regda_amd.utils.prefetch import DevicePrefetcher
    gen = SuperPixelsSLIC()
    assert (gen.region_size, gen.compactness, gen.iterate_num, gen.min_area) == (16, 10, 10, 64)
    assert gen.max_regions(512, 512) == 512 * 512 // 64 + 1 == ops.superpixels_max_regions(512, 512, 64)
    assert SuperPixelsSLIC(8, min_area=16).max_regions(64, 96) == 64 * 96 // 16 + 1
    with pytest.raises(ValueError, match='augment'):
        DevicePrefetcher([{}], regions=gen)
