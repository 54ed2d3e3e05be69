"""CPU: the case tables of tests/teacher_cases.py reach every path they name, the restatement of the host-side decisions
still matches teacher_kernels.hip, the references agree with the project's oracles (oracle.teacher, oracle.evalpath,
tests/golden/tta.npz, F.interpolate on the CPU), and every resize case has its entry in tests/golden/head_tolerances.json."""
import json
import os
import re

import numpy as np
import torch
import torch.nn.functional as F

import teacher_cases as T
from oracle import evalpath
from oracle import teacher as oteach

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = open(os.path.join(ROOT, 'regda_amd', 'csrc', 'teacher_kernels.hip')).read()
TOL = json.load(open(os.path.join(ROOT, 'tests', 'golden', 'head_tolerances.json')))


def test_every_named_path_is_reached():
    reached = T.paths_reached()
    print('\n'.join('%-24s %s' % (p, ', '.join(str(n) for n in reached.get(p, []))) for p in T.REQUIRED))
    missing = [p for p in T.REQUIRED if not reached.get(p)]
    assert not missing, missing
    for prefix, cases in (('crop:', T.CROP_CASES), ('acc:', T.ACC_CASES), ('conf:', T.CONF_CASES)):
        for c in cases:
            got = {p[len(prefix):] for p, names in reached.items() if p.startswith(prefix) and c.name in names}
            assert set(c.paths) <= got, (c.name, set(c.paths) - got)
    # the sizes that make a grid-stride loop take a second trip, and only just
    assert T.trips(int(np.prod(T.DIHEDRAL_BIG))) == 2 and T.trips(int(np.prod(T.NORM_BIG))) == 2
    assert T.trips(T.CONFUSION_GRID_CAP * T.THREADS + 77, T.CONFUSION_GRID_CAP) == 2
    assert all(T.trips(int(np.prod(s))) == 1 for s in T.DIHEDRAL_SHAPES + T.NORM_SHAPES)
    assert int(np.prod(T.DIHEDRAL_BIG)) < 1 << 24                # index_image stays exact


def test_restatement_matches_the_source():
    m = re.search(r'static inline int grid_for\(long long total\) \{ long long g = \(total \+ 255\) / 256; '
                  r'return \(int\)\(g > (\d+) \? (\d+) : \(g < 1 \? 1 : g\)\); \}', SRC)
    assert m and int(m.group(1)) == int(m.group(2)) == T.GRID_CAP and T.THREADS == 256
    assert re.search(r'int grid = \(int\)\(\(total \+ 255\) / 256 > 65535 \? 65535 : \(total \+ 255\) / 256\);', SRC)
    assert int(re.search(r'if \(grid > (\d+)\) grid = \1;', SRC).group(1)) == T.CONFUSION_GRID_CAP
    assert int(re.search(r'n < 0 \|\| C <= 0 \|\| C > (\d+)\) return RGDA_ERR_ARG;', SRC).group(1)) == T.CONFUSION_MAX_CLASSES
    assert re.search(r'if \(n == 0\) return RGDA_OK;', SRC)
    assert re.search(r'const int Ho = \(k & 1\) \? Ws : Hs, Wo = \(k & 1\) \? Hs : Ws;', SRC)
    assert T.dihedral_shape(2, 3, 5, 9, 1) == (2, 3, 9, 5) and T.dihedral_shape(2, 3, 5, 9, 2) == (2, 3, 5, 9)
    assert re.search(r'full\[i\] = __fdiv_rn\(full\[i\], count\[n \* HW \+ p\]\);', SRC)
    assert re.search(r'#pragma clang fp contract\(off\)', SRC)
    assert re.search(r'if \(v > best\) \{ best = v; arg = c; \}', SRC)
    assert (T.grid_for(0), T.grid_for(1), T.grid_for(257), T.grid_for(1 << 30)) == (1, 1, 2, T.GRID_CAP)
    assert T.confusion_status(5, 65) == T.ERR_ARG and T.confusion_status(0, 64) == T.OK


def test_dihedral_reference_is_the_oracles_views():
    x = torch.from_numpy(T.index_image((2, 3, 5, 9)))
    for f, k, ff in T.VIEWS:
        want = oteach.augment(x, bool(f), k) if ff else oteach.deaugment(x, bool(f), -k % 4)
        got = T.dihedral_ref(x.numpy(), f, k, ff)
        assert got.shape == T.dihedral_shape(2, 3, 5, 9, k) and np.array_equal(got, want.numpy()), (f, k, ff)
    # de-augmenting undoes augmenting, and the two orders differ wherever both a flip and an odd rotation are asked for
    for f, k in oteach.tta_views():
        back = T.dihedral_ref(T.dihedral_ref(x.numpy(), f, k, 1), f, -k % 4, 0)
        assert np.array_equal(back, x.numpy())
        same = np.array_equal(T.dihedral_ref(x.numpy(), f, k, 1), T.dihedral_ref(x.numpy(), f, k, 0))
        assert same == (not (f and k & 1)), (f, k)
    assert len(set(T.VIEWS)) == 16
    src, old = T.dihedral_acc_inputs(T.DIHEDRAL_SHAPES[-1], (1, 1, 0))
    ref, bound = T.dihedral_acc_ref(src, old, (1, 1, 0), T.DIHEDRAL_SCALE)
    f32 = old + np.float32(T.DIHEDRAL_SCALE) * T.dihedral_ref(src, 1, 1, 0)           # numpy's own fp32: within the bound
    assert (np.abs(f32 - ref) <= bound).all() and bound.max() < 1e-6


def test_window_references_compose_to_the_oracles_pre_slide(gold):
    """crop -> model -> accumulate over oracle.teacher.windows, then normalise: the sliding-window result of
    oracle.teacher.pre_slide, bit for bit (a pointwise model, so the tiles' zero padding stays out of the result)."""
    g = gold('tta.npz')
    model = lambda t: t * 2.0 + 1.0
    for i, tile in ((0, (8, 8)), (1, (16, 16)), (2, (8, 12))):
        img = g[f'img{i}']
        N, C, H, W = img.shape
        want = oteach.pre_slide(model, torch.from_numpy(img), num_classes=C, tile_size=tile).numpy()
        full, count = np.zeros((N, C, H, W), np.float32), np.zeros((N, 1, H, W), np.float32)
        for (y1, y2, x1, x2) in oteach.windows(H, W, tile):
            c = T.CropCase('w', img.shape, y1, x1, y2 - y1, x2 - x1, tile[0], tile[1], ())
            pred = model(T.crop_ref(img, c))
            a = T.AccCase('w', img.shape, tile, [(y1, x1, y2 - y1, x2 - x1)], ())
            full, count = T.acc_ref([pred], full, count, a)
        assert count.max() > 1 and np.array_equal(T.norm_ref(full, count), want)
    for c in T.CROP_CASES:                                       # the crop with its padding is the oracle's, where it pads rows only
        full = T.index_image(c.shape)
        win = torch.from_numpy(full[:, :, c.y1:c.y1 + c.h, c.x1:c.x1 + c.w])
        want = F.pad(win, (0, c.Tw - c.w, 0, c.Th - c.h))
        assert np.array_equal(T.crop_ref(full, c), want.numpy())
    for c in T.ACC_CASES:
        tiles, full, count = T.acc_inputs(c)
        f2, c2 = T.acc_ref(tiles, full, count, c)
        assert np.isfinite(f2).all() and np.isnan(tiles[0]).any() == ('nan_padding' in c.paths)
        touched = np.zeros(count.shape, bool)
        for (y1, x1, h, w) in c.windows:
            touched[:, :, y1:y1 + h, x1:x1 + w] = True
        assert np.array_equal(c2[~touched], count[~touched]) and (c2[touched] >= count[touched] + 1).all()
        assert np.array_equal(f2[np.broadcast_to(~touched, f2.shape)], full[np.broadcast_to(~touched, f2.shape)])
        assert count.any() and full.all()
    full, count = T.norm_inputs(T.NORM_SHAPES[1])
    out = T.norm_ref(full, count)
    assert np.isnan(out).any() and np.isinf(out).any() and np.isfinite(out).any()


def test_resize_and_pad_references(gold):
    g = gold('tta.npz')
    cls = torch.from_numpy(g['probs1_tta1'])
    np.testing.assert_allclose(T.resize_ref(cls, (64, 48)).squeeze(0).numpy(), g['resized'], rtol=0, atol=1e-6)
    for shape, size in T.RESIZE_CASES:
        x = T.resize_inputs(shape, size)
        ref = T.resize_ref(x, size)
        f64 = F.interpolate(x.double(), size, mode='bilinear', align_corners=True)
        # torch's fp64 path forms the source coordinate in fp64, the reference in fp32 like the kernel: an ulp of it apart
        assert tuple(ref.shape[2:]) == size and float((ref - f64).abs().max()) <= 2e-5, (shape, size)
        e = TOL['resize'][T.resize_name(shape, size)]
        assert e['bound'] > 0 and e['floor'] == (e['deviation'] == 0.0)
        if not e['floor']:
            assert e['bound'] == TOL['margin'] * e['deviation']
    x = T.index_image(T.PAD_SHAPE)
    for top, bottom in T.PAD_CASES:
        out = T.pad_ref(x, top, bottom)
        assert out.shape == T.PAD_SHAPE[:2] + (T.PAD_SHAPE[2] + top + bottom, T.PAD_SHAPE[3])
        if top >= 0 and bottom >= 0:                             # pad_image's own call: (rows_missing, cols_missing)
            target = (T.PAD_SHAPE[2] + top, T.PAD_SHAPE[3] + bottom)
            assert np.array_equal(out, oteach.pad_image(torch.from_numpy(x), target).numpy())
        lo, hi = max(-top, 0), T.PAD_SHAPE[2] - max(-bottom, 0)
        assert np.array_equal(out[:, :, max(top, 0):max(top, 0) + hi - lo], x[:, :, lo:hi])


def test_argmax_and_confusion_references():
    for name, x in T.argmax_cases():
        assert np.array_equal(T.argmax_ref(x), torch.from_numpy(x).argmax(1).numpy()), name
        assert np.array_equal(T.argmax_ref(x), np.argmax(x, 1)), name
    ties = dict(T.argmax_cases())['ties']
    r = T.argmax_ref(ties)
    assert (r[0, 0] == 0).all() and (r[0, 1] == 3).all() and (r[0, 2] == 0).all()
    for c in T.CONF_CASES:
        yt, yp = T.conf_inputs(c)
        cm, flag = T.conf_ref(yt, yp, c.C, 0)
        assert cm.sum() <= c.n and flag == int(c.special == 'bad')
        if not flag:
            ok = yt >= 0
            assert np.array_equal(cm, evalpath.confusion_matrix(yt[ok], np.clip(yp[ok], 0, c.C - 1), c.C))
            assert cm.sum() == ok.sum()
        else:
            assert cm.sum() == (yt >= 0).sum() - 3               # label C, prediction -1, prediction C: not counted
        if c.special == 'negative':
            assert (yp[yt < 0] == c.C).any()                     # an out-of-range prediction under a skipped truth
    assert T.conf_ref(*T.conf_inputs(T.CONF_CASES[1]), 64, 0)[0].astype(bool).sum() > 64
