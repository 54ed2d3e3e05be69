"""Mint tests/golden/edge_shrink.npz from the reference's OWN edge_shrinking (regda/gast/superpixels.py:129-152), the one
part of its superpixel route that is its own code.  The module's third-party imports (cv2, skimage.io, tqdm) are not
installed; they are replaced by empty stub modules, and `iio.imsave` -- the only call of theirs that edge_shrinking
makes -- by a no-op.  The superpixel generators themselves (cv2.ximgproc LSC, skimage SLIC) are NOT pinned: no golden
can come from them.

Run in the build container only (needs the reference checkout):  python tests/golden/make_superpixel_goldens.py
Data only: three int32 maps of 48 x 48 and the reference's outputs for win_size 1 and 3 (region_size 16, so its fill
value int(h / 16 * w / 16) = 9):
  grid   : the 16-pixel grid map, ids 0..8
  thin   : a one-pixel-wide region, a region touching all four borders, and two blocks
  blocky : seeded random ids on a 6-pixel block raster, offset so the blocks are cut by the borders"""
import importlib.util
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = '/root/reference'


def _load_reference():
    cv2 = types.ModuleType('cv2')
    skimage = types.ModuleType('skimage')
    iio = types.ModuleType('skimage.io')
    iio.imsave = lambda *a, **k: None
    skimage.io = iio
    tqdm = types.ModuleType('tqdm')
    tqdm.tqdm = lambda it, *a, **k: it
    sys.modules.update({'cv2': cv2, 'skimage': skimage, 'skimage.io': iio, 'tqdm': tqdm})
    spec = importlib.util.spec_from_file_location('ref_superpixels', os.path.join(REF, 'regda', 'gast', 'superpixels.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def inputs():
    H = W = 48
    yy, xx = np.mgrid[0:H, 0:W]
    grid = ((yy // 16) * 3 + xx // 16).astype(np.int32)
    thin = np.full((H, W), 1, np.int32)              # region 1: the frame, touches every border
    thin[4:44, 4:44] = 2
    thin[10:30, 20] = 3                              # one pixel wide
    thin[32:40, 8:24] = 4
    thin[6:20, 30:42] = 5
    rng = np.random.default_rng(20261017)
    ids = rng.integers(0, 12, (10, 10)).astype(np.int32)
    blocky = ids[(yy + 3) // 6, (xx + 2) // 6]
    return dict(grid=grid, thin=thin, blocky=blocky)


def main():
    ref = _load_reference()
    out = {}
    for name, m in inputs().items():
        out[name] = m
        for win in (1, 3):
            r = ref.edge_shrinking('unused', 'unused.png', 'png', m.copy(), win_size=win)
            assert r.shape == m.shape
            out['%s_win%d' % (name, win)] = r.astype(np.int32)
    out['fill'] = np.int32(int(48 / 16 * 48 / 16))
    path = os.path.join(HERE, 'edge_shrink.npz')
    np.savez_compressed(path, **out)
    print('wrote %s (%d bytes)' % (path, os.path.getsize(path)))


if __name__ == '__main__':
    main()
