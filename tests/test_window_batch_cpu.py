"""Batched sliding-window inference without a GPU: the window list against pre_slide's loop arithmetic, and the
argument checks of rgda_window_gather / _scatter / _finish (they return RGDA_ERR_ARG before any launch)."""
from math import ceil

import pytest

from regda_amd import _lib
from regda_amd.utils.tools import batched_slide_supported, check_window_batch, window_list

ERR_ARG = -1


def literal_windows(H, W, tile_size):
    """tools.py:61-97's two loops, copied as written."""
    stride = ceil(tile_size[0] * (1 - 1 / 2))
    tile_rows = int(ceil((H - tile_size[0]) / stride) + 1)
    tile_cols = int(ceil((W - tile_size[1]) / stride) + 1)
    out = []
    for row in range(tile_rows):
        for col in range(tile_cols):
            x1, y1 = int(col * stride), int(row * stride)
            x2, y2 = min(x1 + tile_size[1], W), min(y1 + tile_size[0], H)
            x1, y1 = max(int(x2 - tile_size[1]), 0), max(int(y2 - tile_size[0]), 0)
            out.append((y1, x1, y2 - y1, x2 - x1))
    return out


SIZES = [1, 7, 12, 16, 17, 40, 255, 256, 257, 300, 511, 512, 513, 700, 768, 769, 1024, 1025, 1100, 1500, 2000, 6000]
TILES = [(512, 512), (16, 16), (256, 512), (512, 256), (17, 9)]


@pytest.mark.parametrize('tile', TILES)
def test_window_list_is_pre_slides_loop(tile):
    for H in SIZES:
        for W in SIZES:
            assert window_list(H, W, tile) == literal_windows(H, W, tile), (H, W, tile)


def test_window_list_edges():
    assert window_list(512, 512) == [(0, 0, 512, 512)]                          # H = W = tile: the image itself
    assert window_list(513, 512) == [(0, 0, 512, 512), (1, 0, 512, 512)]        # just above: the edge window shifted back
    w = window_list(1100, 700)
    assert len(w) == 4 * 2 and w[-1] == (588, 188, 512, 512)
    assert all(h == 512 and ww == 512 for _, _, h, ww in window_list(1024, 1024)) and len(window_list(1024, 1024)) == 9
    assert len(window_list(6000, 6000)) == 23 * 23
    assert window_list(40, 24) == []                                             # no window: pre_slide's NaN result
    assert window_list(300, 300) == [(0, 0, 300, 300)]                           # smaller than the tile: one padded window


def test_batched_route_scope():
    assert batched_slide_supported((1, 3, 512, 512)) and batched_slide_supported((1100, 700))
    assert not batched_slide_supported((511, 512)) and not batched_slide_supported((512, 300))
    assert batched_slide_supported((600, 600), (512, 256)) and not batched_slide_supported((600, 600), (512, 256), tta=True)
    assert check_window_batch(16, tta=True) == 16
    for bad in (0, -1, 2.5, 1024):
        with pytest.raises(ValueError):
            check_window_batch(bad, tta=True)


@pytest.fixture(scope='module')
def L():
    try:
        return _lib.lib()
    except ImportError as e:
        pytest.skip(str(e))


P = 0x1000      # a non-null pointer that is never dereferenced: every call below is refused before any launch


def test_window_gather_refuses_bad_arguments(L):
    g = L.raw('rgda_window_gather')
    ok = dict(f32=P, u8=None, lut=None, win=P, K=2, V=1, n=1, C=3, H=600, W=600, Th=512, Tw=512, out=P)

    def call(**kw):
        a = dict(ok, **kw)
        return g(a['f32'], a['u8'], a['lut'], a['win'], a['K'], a['V'], a['n'], a['C'], a['H'], a['W'], a['Th'], a['Tw'],
                 a['out'], None, None)
    for bad in (dict(f32=None), dict(u8=P), dict(f32=None, u8=P), dict(f32=None, u8=P, lut=P, C=4), dict(win=None),
                dict(out=None), dict(K=0), dict(n=0), dict(C=0), dict(H=511), dict(W=100), dict(Th=0), dict(V=2),
                dict(V=8, Tw=256), dict(V=0)):
        assert call(**bad) == ERR_ARG, bad


def test_window_scatter_refuses_bad_arguments(L):
    s = L.raw('rgda_window_scatter')
    ok = dict(pred=P, win=P, K=2, V=1, n=2, C=6, H=600, W=600, Th=512, Tw=512, row0=0, rows=600, full=P, count=P)

    def call(**kw):
        a = dict(ok, **kw)
        return s(a['pred'], a['win'], a['K'], a['V'], a['n'], a['C'], a['H'], a['W'], a['Th'], a['Tw'], a['row0'],
                 a['rows'], a['full'], a['count'], None, None)
    for bad in (dict(pred=None), dict(win=None), dict(full=None), dict(count=None), dict(K=0), dict(K=1025),
                dict(V=4), dict(V=8, Th=256), dict(n=0), dict(C=0), dict(H=500), dict(row0=-1), dict(rows=0),
                dict(row0=700, rows=501), dict(rows=1201)):
        assert call(**bad) == ERR_ARG, bad


def test_window_finish_refuses_bad_arguments(L):
    f = L.raw('rgda_window_finish')
    ok = dict(full=P, count=P, n=1, C=6, H=8, W=8, u8=None, i64=None, yt=None, cm=None, flag=None)

    def call(**kw):
        a = dict(ok, **kw)
        return f(a['full'], a['count'], a['n'], a['C'], a['H'], a['W'], a['u8'], a['i64'], a['yt'], a['cm'], a['flag'], None)
    for bad in (dict(full=None), dict(count=None), dict(n=0), dict(C=0), dict(H=0), dict(W=0), dict(u8=P, C=257),
                dict(yt=P), dict(cm=P), dict(yt=P, cm=P), dict(yt=P, cm=P, flag=P, C=65)):
        assert call(**bad) == ERR_ARG, bad
