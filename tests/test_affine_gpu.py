"""GPU: rgda_augment_affine against its numpy restatement (tests/affine_ref.py) -- image, labels and regions bit for bit,
the soft planes within the rounding of their f32 sum -- at odd shapes, on both store routes and both staging routes,
against rgda_augment_tiles for the dihedral rows, with invalid rows, and through DevicePrefetcher."""
import random

import numpy as np
import pytest
import torch

import affine_ref
from regda_amd import ops
from regda_amd.aug import augmentation as A

pytestmark = pytest.mark.gpu

MEAN = (123.675, 116.28, 103.53)
STD = (58.395, 57.12, 57.375)
HI, WI = 70, 83
SIZES = [(40, 36), (33, 33)]        # partial tiles with 16-byte stores; the scalar route
SOFT_RTOL = 7 * 2.0 ** -24          # four products and three sums of non-negative terms in f32
# AFF_IMG_DW of regda_amd/csrc/augment_kernels.hip: the kernel's LDS budget for a tile's staged uint8 window, in dwords.
# _tile_fits below restates the kernel's window arithmetic (its `rd` row stride included) to know which route a tile
# takes: keep both in step with the kernel, or the route test may run one route only while still passing.
IMG_BUDGET_DW = 8192


def _raw(n, h, w, c, seed):
    g = torch.Generator().manual_seed(seed)
    return dict(img=torch.randint(0, 256, (n, h, w, 3), generator=g, dtype=torch.uint8),
                label=torch.randint(0, 256, (n, h, w), generator=g, dtype=torch.uint8),
                soft=torch.rand(n, c, h, w, generator=g) + 0.01,
                regs=torch.randint(1, 1 << 20, (n, h, w), generator=g, dtype=torch.int32))


def _rows(ho, wo):
    """15 rows, five launches of three: (name, row, scaled).  The scaled rows are placed so that part of the output
    falls outside the input."""
    rows = [('identity', affine_ref.dihedral_row(10, 20, 0, ho, wo), False)]
    rows += [('d%d' % d, affine_ref.dihedral_row(5 + d, 7 + 2 * d, d, ho, wo), False) for d in range(8)]
    rows += [('s0.5 t30', affine_ref.make_row(HI / 2, WI / 2, affine_ref.rot(0.5, 30.0), (9, 200, 77)), True),
             ('s2 t-45', affine_ref.make_row(3.25, 80.7, affine_ref.rot(2.0, -45.0)), True),
             ('s4', affine_ref.make_row(68.5, 2.3, affine_ref.rot(4.0, 0.0), (255, 0, 128)), True),
             ('s0.25 t77', affine_ref.make_row(31.9, 40.2, affine_ref.rot(0.25, 77.0), (1, 2, 3)), True),
             ('corner 0', affine_ref.make_row(0, 0, affine_ref.rot(1.0, 15.0)), True),
             ('corner hw', affine_ref.make_row(HI, WI, affine_ref.rot(1.3, -20.0), (255, 255, 255)), True)]
    return rows


@pytest.fixture(scope='module')
def tables():
    return A.Normalize(MEAN, STD, clamp=True).table(), A.label_table(-1, 7, -1)


@pytest.fixture(scope='module')
def raw():
    return _raw(3, HI, WI, 16, seed=5)


@pytest.fixture(scope='module')
def expected(raw, tables):
    """{size: [per launch: the restatement of rows 3k .. 3k+2 on the three samples]} with all 16 soft planes."""
    lut, llut = tables
    out = {}
    for size in SIZES:
        rows = _rows(*size)
        out[size] = [affine_ref.augment(raw['img'].numpy(), np.array([r for _, r, _ in rows[k:k + 3]]), size, lut.numpy(),
                                        label=raw['label'].numpy(), label_lut=llut.numpy(), ignore_label=-1,
                                        soft=raw['soft'].numpy(), regs=raw['regs'].numpy())
                     for k in range(0, len(rows), 3)]
    return out


def _bits(t):
    return t.view(np.uint32) if isinstance(t, np.ndarray) else t.cpu().numpy().view(np.uint32)


def _compare(got, want, n, c, tag):
    """Sample n of the launch's outputs against the restatement's (its first c soft planes)."""
    assert np.array_equal(_bits(got['image'][n]), _bits(want['image'][n])), (tag, 'image')
    assert np.array_equal(got['label'][n].cpu().numpy(), want['label'][n]), (tag, 'label')
    assert np.array_equal(got['regs'][n].cpu().numpy(), want['regs'][n]), (tag, 'regs')
    s, ref = got['soft'][n].cpu().numpy(), want['soft'][n][:c]
    err = np.abs(s.astype(np.float64) - ref)
    assert (err <= SOFT_RTOL * np.abs(ref)).all(), (tag, 'soft', float((err / np.maximum(np.abs(ref), 1e-30)).max()))
    exact = np.broadcast_to(want['exact'][n], s.shape)
    assert np.array_equal(_bits(s[exact]), _bits(ref.astype(np.float32)[exact])), (tag, 'soft on pixel centres')
    assert (s[:, ~want['inframe'][n] & want['exact'][n]] == 0).all()


@pytest.mark.parametrize('c', [7, 16])
@pytest.mark.parametrize('size', SIZES)
def test_odd_shapes_match_the_restatement(raw, tables, expected, size, c):
    """N = 3, 70 x 83 -> 40 x 36 and 33 x 33, all four planes: identity, the eight dihedral elements, s = 0.5 / 30 deg,
    s = 2 / -45 deg, s = 4, s = 0.25, a centre on each extreme corner.  Every scaled row has pixels inside and outside the
    input."""
    lut, llut = (t.cuda() for t in tables)
    dev = {k: v.cuda() for k, v in raw.items()}
    soft = dev['soft'][:, :c].contiguous()
    rows = _rows(*size)
    flag = torch.zeros(1, dtype=torch.int32, device='cuda')
    for k in range(0, len(rows), 3):
        want = expected[size][k // 3]
        prm = torch.tensor([r for _, r, _ in rows[k:k + 3]], dtype=torch.int32)
        got = ops.augment_affine(dev['img'], prm, lut, size, label=dev['label'], label_lut=llut, ignore_label=-1,
                                 soft=soft, regs=dev['regs'], flag=flag)
        assert got['image'].shape == (3, 3) + size and got['label'].dtype == torch.int64
        assert got['soft'].shape == (3, c) + size and got['regs'].shape == (3, 1) + size
        for n, (name, _, scaled) in enumerate(rows[k:k + 3]):
            inframe = want['inframe'][n]
            assert inframe.any() and (not scaled or not inframe.all()), name
            assert (want['exact'][n].all()) == (not scaled), name
            _compare(got, want, n, c, (name, size, c))
    assert flag.item() == 0


def test_staging_budget_is_the_kernels():
    """IMG_BUDGET_DW above is the kernel's AFF_IMG_DW, read from the source."""
    import os
    import re
    src = open(os.path.join(os.path.dirname(ops.__file__), 'csrc', 'augment_kernels.hip')).read()
    assert int(re.search(r'constexpr int AFF_IMG_DW = (\d+);', src).group(1)) == IMG_BUDGET_DW


def _tile_fits(row, size, hi, wi):
    """Per 32 x 32 output tile: does the bounding box of its image taps, clipped to the input, fit the staging budget."""
    Y, X = affine_ref.coords(row, *size)
    y, x = (Y - 32768) >> 16, (X - 32768) >> 16
    fits = []
    for i0 in range(0, size[0], 32):
        for j0 in range(0, size[1], 32):
            ty, tx = y[i0:i0 + 32, j0:j0 + 32], x[i0:i0 + 32, j0:j0 + 32]
            wr = min(ty.max() + 1, hi - 1) - max(ty.min(), 0) + 1
            wc = min(tx.max() + 1, wi - 1) - max(tx.min(), 0) + 1
            if wr > 0 and wc > 0:
                fits.append(bool(wr * ((3 * wc + 6) // 4) <= IMG_BUDGET_DW))
    return fits


def test_larger_output_runs_the_staged_and_the_direct_route(tables):
    """128 x 128 -> 96 x 96 (nine tiles per sample): s = 2 / 45 deg and s = 1.1 / 10 deg have small footprints (staged in
    LDS); at s = 0.25 / 45 deg and s = 0.3 a central tile's footprint is the whole 48 KB image (read directly) while
    corner tiles still fit.  All compare with the one restatement."""
    lut, llut = tables
    raw = _raw(4, 128, 128, 3, seed=8)
    size = (96, 96)
    rows = [affine_ref.make_row(64, 64, affine_ref.rot(2.0, 45.0), (10, 20, 30)),
            affine_ref.make_row(60.3, 70.9, affine_ref.rot(0.25, 45.0), (200, 100, 0)),
            affine_ref.make_row(64, 64, affine_ref.rot(1.1, 10.0)),
            affine_ref.make_row(64, 64, affine_ref.rot(0.3, 0.0))]
    fits = [_tile_fits(r, size, 128, 128) for r in rows]
    assert all(fits[0]) and all(fits[2]) and not all(fits[1]) and any(fits[1]) and not all(fits[3])
    want = affine_ref.augment(raw['img'].numpy(), np.array(rows), size, lut.numpy(), label=raw['label'].numpy(),
                              label_lut=llut.numpy(), ignore_label=-1, soft=raw['soft'].numpy(), regs=raw['regs'].numpy())
    got = ops.augment_affine(raw['img'].cuda(), torch.tensor(rows, dtype=torch.int32), lut.cuda(), size,
                             label=raw['label'].cuda(), label_lut=llut.cuda(), ignore_label=-1, soft=raw['soft'].cuda(),
                             regs=raw['regs'].cuda())
    for n in range(4):
        _compare(got, want, n, 3, n)


def test_dihedral_and_quarter_turn_rows_equal_augment_tiles(raw, tables):
    """The eight dihedral rows and RandomScaleRotate's exact quarter turns at 33 x 33, the four untransposed elements at
    40 x 36: all four outputs torch.equal with rgda_augment_tiles for the matching (y0, x0, d)."""
    lut, llut = (t.cuda() for t in tables)
    dev = {k: v.cuda() for k, v in raw.items()}
    soft = dev['soft'][:, :7].contiguous()
    turns = {90.0: 3, -90.0: 5, 180.0: 6}                       # RandomScaleRotate's matrix at theta -> d
    for size, cases in (((33, 33), [(d, None) for d in range(8)] + [(d, th) for th, d in turns.items()] + [(0, None)]),
                        ((40, 36), [(0, None), (2, None), (4, None), (6, None), (6, 180.0), (0, 0.0)])):
        ho, wo = size
        for k in range(0, len(cases), 3):
            tile_rows, aff_rows = [], []
            for n, (d, theta) in enumerate(cases[k:k + 3]):
                y0, x0 = 3 + 2 * n + d, 11 + n + 3 * d
                tile_rows.append([y0, x0, d, 0])
                m = A.matrix(d) if theta is None else A.rotation(1.0, theta)
                aff_rows.append(A.affine_row(y0, x0, m, (0, 0), ho, wo, HI, WI))
                if theta is not None:
                    assert aff_rows[-1] == affine_ref.dihedral_row(y0, x0, d, ho, wo)
            a = ops.augment_tiles(dev['img'], torch.tensor(tile_rows, dtype=torch.int32), lut, size, label=dev['label'],
                                  label_lut=llut, soft=soft, regs=dev['regs'])
            b = ops.augment_affine(dev['img'], torch.tensor(aff_rows, dtype=torch.int32), lut, size, label=dev['label'],
                                   label_lut=llut, ignore_label=-1, soft=soft, regs=dev['regs'])
            for name in ('image', 'label', 'soft', 'regs'):
                assert a[name].dtype == b[name].dtype and torch.equal(a[name], b[name]), (size, cases[k:k + 3], name)


@pytest.mark.parametrize('bad', [(1, 2, 131073), (1, 4, -131073), (0, 7, 1), (2, 6, 1 << 24), (2, 0, HI * 65536 + 1)])
def test_invalid_rows_are_skipped_and_flagged(raw, tables, bad):
    """A device-side row the check rejects: its outputs keep their sentinel, the flag is 1, its neighbours are written."""
    n_bad, col, val = bad
    lut, llut = (t.cuda() for t in tables)
    dev = {k: v.cuda() for k, v in raw.items()}
    soft = dev['soft'][:, :7].contiguous()
    size = (40, 36)
    rows = [affine_ref.make_row(30, 40, affine_ref.rot(0.7, 20.0)) for _ in range(3)]
    rows[n_bad][col] = val
    assert not affine_ref.row_valid(rows[n_bad], HI, WI)
    want = affine_ref.augment(raw['img'].numpy(), np.array(rows), size, tables[0].numpy(), label=raw['label'].numpy(),
                              label_lut=tables[1].numpy(), ignore_label=-1, soft=raw['soft'].numpy(),
                              regs=raw['regs'].numpy())
    out = dict(image=torch.full((3, 3) + size, -7.0, device='cuda'),
               label=torch.full((3,) + size, -77, dtype=torch.int64, device='cuda'),
               soft=torch.full((3, 7) + size, -7.0, device='cuda'),
               regs=torch.full((3, 1) + size, -77, dtype=torch.int64, device='cuda'))
    flag = torch.zeros(1, dtype=torch.int32, device='cuda')
    got = ops.augment_affine(dev['img'], torch.tensor(rows, dtype=torch.int32).cuda(), lut, size, label=dev['label'],
                             label_lut=llut, ignore_label=-1, soft=soft, regs=dev['regs'], out=out, flag=flag)
    assert flag.item() == 1
    for n in range(3):
        if n == n_bad:
            assert want['image'][n] is None
            assert (got['image'][n] == -7).all() and (got['soft'][n] == -7).all()
            assert (got['label'][n] == -77).all() and (got['regs'][n] == -77).all()
        else:
            _compare(got, want, n, 7, (bad, n))
    with pytest.raises(ValueError):                             # the same table from the host is refused before the launch
        ops.augment_affine(dev['img'], torch.tensor(rows, dtype=torch.int32), lut, size)


def _pipe(seed, warp):
    ts = [A.RandomCrop((48, 40)), A.RandomHorizontalFlip(1.0), A.RandomVerticalFlip(0.0)]
    if warp is not None:
        ts.append(A.RandomScaleRotate(scale=(0.5, 2.0), degrees=40, prob=warp, fill=(5, 6, 7)))
    return A.Compose(ts + [A.Normalize(MEAN, STD, clamp=True)], rng=random.Random(seed),
                     generator=torch.Generator().manual_seed(seed), offset=-1, num_class=7)


def test_prefetcher_delivers_the_pipelines_batches():
    """A two-batch DevicePrefetcher with RandomScaleRotate hands out what pipeline.batch gives for the same seed, stage by
    stage; with prob = 0 it hands out, bit for bit, what the pipeline without the transform delivers (the flips here do
    not depend on their draw, the crops come from the torch generator)."""
    from regda_amd.utils.prefetch import DevicePrefetcher
    host = []
    for i in range(2):
        r = _raw(3, HI, WI, 7, seed=30 + i)
        host.append(dict(images_t=r['img'], label_t=r['label'], soft_t=r['soft'], regs_t=r['regs']))
    roles = dict(image='images_t', mask='label_t', soft='soft_t', mask_sup='regs_t')
    names = dict(image='images_t', mask='label_t', soft='soft_t', mask_sup='regs_t')

    def delivered(pipe, k=5):
        pf = DevicePrefetcher(host, depth=2, augment=[(pipe, roles)])
        out = []
        for _ in range(k):
            b = pf.next()
            torch.cuda.synchronize()
            out.append({key: v.clone() for key, v in b.items()})
            pf.release()
        return out

    got, ref = delivered(_pipe(3, 0.7)), _pipe(3, 0.7)
    assert ref.param_cols == 8
    warped = 0
    for i in range(5):
        b = host[i % 2]
        prm = ref.params(3, HI, WI)
        warped += int((prm[:, 2:6].abs().sort(1).values != torch.tensor([0, 0, 32768, 32768])).any(1).sum())
        want = ref.batch(b['images_t'], mask=b['label_t'], soft=b['soft_t'], mask_sup=b['regs_t'], params=prm)
        for role, key in names.items():
            assert got[i][key].dtype == want[role].dtype and torch.equal(got[i][key], want[role]), (i, key)
        assert (got[i]['label_t'] == -1).any()
    assert 0 < warped < 15
    off, plain = delivered(_pipe(3, 0.0)), delivered(_pipe(3, None))
    for i in range(5):
        for key in names.values():
            assert torch.equal(off[i][key], plain[i][key]), (i, key)
