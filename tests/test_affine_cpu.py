"""CPU: random scale and rotation of raw tiles (rgda_augment_affine) -- the numpy restatement (tests/affine_ref.py)
against the dihedral restatement and an independent fp64 bilinear, the draws of RandomScaleRotate / ShiftScaleRotate,
the host-side row check and the pipelines' refusals."""
import random

import numpy as np
import pytest
import torch
from scipy import ndimage

import affine_ref
import aug_ref
from regda_amd import aug, ops
from regda_amd.aug import albu, augmentation as A

MEAN = (123.675, 116.28, 103.53)
STD = (58.395, 57.12, 57.375)


def _raw(n, h, w, c=5, seed=0):
    g = torch.Generator().manual_seed(seed)
    return dict(img=torch.randint(0, 256, (n, h, w, 3), generator=g, dtype=torch.uint8),
                label=torch.randint(0, 256, (n, h, w), generator=g, dtype=torch.uint8),
                soft=torch.rand(n, c, h, w, generator=g),
                regs=torch.randint(0, 1 << 20, (n, h, w), generator=g, dtype=torch.int32))


class CountingRandom(random.Random):
    """random.Random that counts its primitive draws (uniform and friends go through random())."""
    draws = 0

    def random(self):
        self.draws += 1
        return super().random()


def test_dihedral_rows_equal_the_dihedral_restatement():
    """For each of the eight d, the affine restatement of the matching row gives aug_ref's image, label, soft planes
    and regions bit for bit, and every weight is on a pixel centre."""
    raw = _raw(1, 29, 34, seed=3)
    lut = A.Normalize(MEAN, STD, clamp=True).table()
    llut = A.label_table(-1, 7, -1)
    ho = wo = 19
    for d in range(8):
        y0, x0 = 3 + d, 9 - d
        want = aug_ref.augment(raw['img'], torch.tensor([[y0, x0, d, 0]], dtype=torch.int32), (ho, wo), lut,
                               label=raw['label'], label_lut=llut, soft=raw['soft'], regs=raw['regs'])
        prm = np.array([affine_ref.dihedral_row(y0, x0, d, ho, wo)])
        got = affine_ref.augment(raw['img'].numpy(), prm, (ho, wo), lut.numpy(), label=raw['label'].numpy(),
                                 label_lut=llut.numpy(), soft=raw['soft'].numpy(), regs=raw['regs'].numpy())
        assert got['exact'][0].all() and got['inframe'][0].all(), d
        assert np.array_equal(got['image'][0].view(np.uint32), want['image'][0].numpy().view(np.uint32)), d
        assert np.array_equal(got['label'][0], want['label'][0].numpy()), d
        assert np.array_equal(got['regs'][0], want['regs'][0].numpy()), d
        assert np.array_equal(got['soft'][0], want['soft'][0].numpy().astype(np.float64)), d


@pytest.mark.parametrize('s,theta,size', [(1.0, 0.0, (20, 24)), (0.5, 30.0, (40, 36)), (2.0, -45.0, (33, 33)),
                                          (0.8, 90.0, (21, 30)), (4.0, 10.0, (24, 24)), (0.25, 77.0, (16, 16))])
def test_image_agrees_with_an_independent_fp64_bilinear(s, theta, size):
    """scipy's order-1 map_coordinates at the same Q16 coordinates (the input padded by one pixel of the fill colour,
    so that the border band interpolates towards it as the contract says).  Truncating fx, fy to 8 bits moves the value
    by less than 255/256 each and the two roundings add 0.5 each: the integers differ by at most 2.  A wrong
    orientation or centre convention moves a random image by tens of grey levels."""
    raw = _raw(1, 37, 45, seed=11)
    img = raw['img'][0].numpy()
    fill = (7, 130, 255)
    row = affine_ref.make_row(17.5, 24.0, affine_ref.rot(s, theta), fill)
    ident = np.broadcast_to(np.arange(256, dtype=np.float32), (3, 256))
    got = affine_ref.warp_one(row, size, img, ident)
    Y, X = affine_ref.coords(row, *size)
    yy, xx = (Y - 32768) / 65536.0, (X - 32768) / 65536.0
    for ch in range(3):
        pad = np.pad(img[:, :, ch].astype(np.float64), 1, constant_values=fill[ch])
        want = ndimage.map_coordinates(pad, [yy + 1, xx + 1], order=1, mode='constant', cval=fill[ch])
        diff = np.abs(got['byte'][ch].astype(np.int64) - np.rint(want).astype(np.int64))
        assert diff.max() <= 2, (ch, diff.max())
    assert np.array_equal(got['image'], got['byte'].astype(np.float32))
    if s < 1:
        assert got['inframe'].any() and not got['inframe'].all()


def test_orientation_and_centre():
    """A quarter turn by RandomScaleRotate's matrix is the dihedral element 3 (rows from reversed columns), and the
    centre convention puts an even crop's centre between pixels: the identity row of a 4 x 4 crop at (2, 3) reads
    pixel (2 + i, 3 + j)."""
    m = A.rotation(1.0, 90.0)
    assert [int(round(v * 32768)) for v in m.ravel()] == [0, -32768, 32768, 0]
    assert A.code(np.rint(m).astype(int)) == 3
    img = np.arange(10 * 12 * 3, dtype=np.int64).reshape(10, 12, 3).astype(np.uint8)
    ident = np.broadcast_to(np.arange(256, dtype=np.float32), (3, 256))
    got = affine_ref.warp_one(A.affine_row(2, 3, A.IDENTITY, (0, 0), 4, 4, 10, 12), (4, 4), img, ident)
    assert np.array_equal(got['byte'], img[2:6, 3:7].transpose(2, 0, 1))
    assert A.affine_row(2, 3, A.IDENTITY, (0, 0), 4, 4, 10, 12) == affine_ref.dihedral_row(2, 3, 0, 4, 4)


def _srr(scale, degrees, prob, rng, gen, fill=(0, 0, 0), first=False):
    w = A.RandomScaleRotate(scale=scale, degrees=degrees, prob=prob, fill=fill)
    flips = [A.RandomHorizontalFlip(0.5), A.RandomVerticalFlip(0.5), A.RandomRotate90(0.5)]
    return A.Compose([A.RandomCrop((32, 32))] + ([w] + flips if first else flips + [w]) +
                     [A.Normalize(MEAN, STD, clamp=True)], rng=rng, generator=gen)


@pytest.mark.parametrize('prob', [0.0, 0.5, 1.0])
def test_three_draws_per_sample_whatever_the_coin_says(prob):
    rng = CountingRandom(5)
    p = _srr((0.5, 2.0), 30, prob, rng, torch.Generator().manual_seed(5))
    assert p.param_cols == 8
    t = p.params(7, 48, 40)
    assert rng.draws == 7 * (3 + 3) and tuple(t.shape) == (7, 8) and t.dtype == torch.int32
    rng = CountingRandom(5)
    q = albu.Compose([albu.RandomCrop(32, 32), albu.ShiftScaleRotate(p=prob)], rng=rng)
    q.params(7, 48, 40)
    assert rng.draws == 7 * (2 + 5)


def test_draws_respect_their_bounds_and_repeat_with_the_seed():
    lo, hi, deg = 0.5, 2.0, 25.0
    tabs = [_srr((lo, hi), deg, 1.0, random.Random(9), torch.Generator().manual_seed(9), fill=(1, 2, 3),
                 first=True).params(200, 48, 40) for _ in range(2)]
    assert torch.equal(tabs[0], tabs[1])
    t = tabs[0].numpy().astype(np.float64)
    ops.check_affine_params(tabs[0], 48, 40)
    m = t[:, 2:6].reshape(-1, 2, 2) / 32768
    # every row is (1/s) R(theta) times a signed permutation: |det| = 1/s^2, and the turn of its first column modulo a
    # quarter turn is within the bound
    sc = 1 / np.sqrt(np.abs(np.linalg.det(m)))
    assert (sc > lo - 1e-3).all() and (sc < hi + 1e-3).all() and sc.std() > 0.1
    ang = np.rad2deg(np.arctan2(m[:, 1, 0], m[:, 0, 0]))
    off = np.abs((ang + 45) % 90 - 45)
    assert (off < deg + 1e-2).all() and off.std() > 1
    assert (t[:, 6] == (1 | 2 << 8 | 3 << 16)).all() and (t[:, 7] == 0).all()
    # the crop centre: an integer origin plus half the 32 x 32 output
    assert ((t[:, 0] / 65536 - 16) % 1 == 0).all() and (t[:, 0] / 65536 - 16 <= 48 - 32).all() and (t[:, 0] >= 16 * 65536).all()
    # albumentations' class: scale inside 1 +- limit, a shift inside the limit of the output size
    q = albu.Compose([albu.RandomCrop(32, 32), albu.ShiftScaleRotate(0.1, 0.2, 30, p=1.0)], rng=random.Random(3))
    t = q.params(200, 64, 64).numpy().astype(np.float64)
    ops.check_affine_params(q.params(10, 64, 64), 64, 64)
    sc = 1 / np.sqrt(np.abs(np.linalg.det(t[:, 2:6].reshape(-1, 2, 2) / 32768)))
    assert (sc > 0.8 - 1e-3).all() and (sc < 1.2 + 1e-3).all()
    frac = (t[:, :2] / 65536) % 1
    assert (np.minimum(frac, 1 - frac) > 1e-6).any()            # shifted off the pixel grid


def test_shift_scale_rotate_pair_limits():
    """A (lo, hi) limit: shift and rotate pairs are the range, a scale pair is a pair of offsets from 1."""
    w = albu.ShiftScaleRotate(shift_limit=(0.0, 0.1), scale_limit=(-0.5, 1.0), rotate_limit=(10, 30), p=1.0)
    assert w.shift == (0.0, 0.1) and w.scale == (0.5, 2.0) and w.rotate == (10, 30)
    assert albu.ShiftScaleRotate(scale_limit=0.25).scale == (0.75, 1.25)
    with pytest.raises(ValueError):
        albu.ShiftScaleRotate(scale_limit=(-0.8, 0.0))          # 1 - 0.8 is outside [1/4, 4]
    with pytest.raises(ValueError):
        albu.ShiftScaleRotate(scale_limit=(0.0, 3.5))           # 1 + 3.5 is outside [1/4, 4]
    rng = random.Random(7)
    sc, ang, sh = [], [], []
    for _ in range(300):
        m, b = w.draw(rng, 32, 40)
        sc.append(1 / np.sqrt(abs(np.linalg.det(m))))
        # m = rotation(s, -angle): the angle back from its first column
        ang.append(-np.rad2deg(np.arctan2(m[1, 0], m[0, 0])))
        sh.append(-np.linalg.solve(m, b) / np.array([32, 40]))  # (dy, dx) as fractions of the output
    sc, ang, sh = np.array(sc), np.array(ang), np.array(sh)
    assert sc.min() >= 0.5 and sc.max() <= 2.0 and sc.min() < 0.6 and sc.max() > 1.8
    assert ang.min() >= 10 - 1e-9 and ang.max() <= 30 + 1e-9 and ang.max() - ang.min() > 15
    assert sh.min() >= -1e-12 and sh.max() <= 0.1 + 1e-12 and sh.max() > 0.08


def test_unit_scale_and_a_failed_coin_give_dihedral_rows():
    """scale=(1, 1), degrees=0 (coin always fires) and prob=0 both yield the exact rows of rgda_augment_tiles'
    (y0, x0, d): the same crop and element a pipeline without the transform draws from the same seeds (the transform
    sits last, so the earlier draws are the same)."""
    plain = A.Compose([A.RandomCrop((32, 32)), A.RandomHorizontalFlip(0.5), A.RandomVerticalFlip(0.5),
                       A.RandomRotate90(0.5), A.Normalize(MEAN, STD, clamp=True)], rng=random.Random(4),
                      generator=torch.Generator().manual_seed(4))
    assert plain.param_cols == 4
    want = [affine_ref.dihedral_row(int(y0), int(x0), int(d), 32, 32) for y0, x0, d, _ in plain.params(40, 48, 40).tolist()]
    assert len(set(tuple(r[2:6]) for r in want)) == 8
    for scale, deg, prob in (((1, 1), 0, 1.0), ((0.5, 2.0), 45, 0.0)):
        p = _srr(scale, deg, prob, random.Random(4), torch.Generator().manual_seed(4))
        for r in p.params(40, 48, 40).tolist():
            assert sorted(abs(v) for v in r[2:6]) == [0, 0, 32768, 32768] and r[0] % 65536 == 0 and r[1] % 65536 == 0

    # the same rows as the plain pipeline's, once its rng skips the transform's three draws after each sample's three
    class Skipping(random.Random):
        k = 0

        def random(self):
            self.k += 1
            v = super().random()
            if self.k % 3 == 0:
                for _ in range(3):
                    super().random()
            return v
    plain2 = A.Compose(plain.transforms, rng=Skipping(4), generator=torch.Generator().manual_seed(4))
    want2 = [affine_ref.dihedral_row(int(y0), int(x0), int(d), 32, 32) for y0, x0, d, _ in plain2.params(40, 48, 40).tolist()]
    got = _srr((0.5, 2.0), 45, 0.0, random.Random(4), torch.Generator().manual_seed(4)).params(40, 48, 40).tolist()
    assert got == want2


def test_check_affine_params():
    good = torch.tensor([affine_ref.make_row(10, 12, affine_ref.rot(0.25, 45), (255, 255, 255)),
                         affine_ref.make_row(0, 40, affine_ref.rot(4, 0))], dtype=torch.int32)
    ops.check_affine_params(good, 48, 40)
    for col, val in ((2, 131073), (5, -131073), (0, -1), (0, 48 * 65536 + 1), (1, 40 * 65536 + 1), (6, 1 << 24), (6, -1),
                     (7, 1)):
        bad = good.clone()
        bad[1, col] = val
        assert not affine_ref.row_valid(bad[1].tolist(), 48, 40)
        with pytest.raises(ValueError):
            ops.check_affine_params(bad, 48, 40)
    with pytest.raises(ValueError):
        ops.check_affine_params(torch.zeros(2, 4, dtype=torch.int32), 48, 40)
    assert all(affine_ref.row_valid(r, 48, 40) for r in good.tolist())


def test_abi_argument_errors_without_a_gpu():
    """rgda_augment_affine validates its arguments before any launch (in the style of tests/test_abi.py)."""
    import ctypes
    from regda_amd import _lib
    L = _lib.lib()
    buf = ctypes.create_string_buffer(64)
    f = ctypes.addressof(buf)           # 16-byte aligned host address: never dereferenced, the checks fail first
    f = f + (-f) % 16
    names = ['img', 'label', 'soft', 'regs', 'params', 'N', 'Hi', 'Wi', 'C', 'Ho', 'Wo', 'lut', 'label_lut',
             'ignore_label', 'img_out', 'label_out', 'soft_out', 'regs_out', 'flag', 'stream']
    ints = ('N', 'Hi', 'Wi', 'C', 'Ho', 'Wo', 'ignore_label')
    good = (f, 0, 0, 0, f, 2, 48, 40, 0, 64, 64, f, 0, -1, f, 0, 0, 0, 0, None)
    assert len(L.protos['rgda_augment_affine'][1]) == len(names) == 20

    def call(**kw):
        a = dict(zip(names, good))
        a.update(kw)
        L.call('rgda_augment_affine', *[a[k] if k in ints else a[k] or None for k in names])
    for kw in (dict(img=0), dict(N=0), dict(Hi=0), dict(Wo=0), dict(params=0), dict(lut=0), dict(img_out=0),
               dict(img=f + 1), dict(params=f + 2), dict(label=f), dict(label=f, label_lut=f),
               dict(soft=f, C=0, soft_out=f), dict(soft=f, C=6), dict(soft=f + 2, C=6, soft_out=f), dict(regs=f)):
        with pytest.raises(ValueError, match='status -1'):
            call(**kw)
    for kw in (dict(Hi=16385), dict(Wi=16385), dict(Ho=8193), dict(Wo=8193), dict(soft=f, C=17, soft_out=f),
               dict(N=65536)):
        with pytest.raises(ValueError, match='not supported'):
            call(**kw)


def test_refusals():
    w = A.RandomScaleRotate
    for kw in (dict(scale=(0.2, 1)), dict(scale=(1, 4.5)), dict(scale=(2, 1)), dict(degrees=-1), dict(degrees=181),
               dict(fill=(0, 0)), dict(fill=(0, 0, 256))):
        with pytest.raises(ValueError):
            w(**kw)
    with pytest.raises(ValueError, match='at most one'):
        A.Compose([A.RandomCrop((8, 8)), w(), A.RandomHorizontalFlip(0.5), w()])
    with pytest.raises(ValueError, match='RandomCrop must come first'):
        A.Compose([w(), A.RandomCrop((8, 8))])
    with pytest.raises(ValueError, match='Normalize must come last'):
        A.Compose([A.Normalize(MEAN, STD), w()])
    assert A.Compose([A.RandomCrop((8, 8)), w(), A.RandomHorizontalFlip(0.5)]).param_cols == 8
    assert A.Compose([w(), A.Normalize(MEAN, STD)]).param_cols == 8
    with pytest.raises(ValueError, match='border_mode'):
        albu.ShiftScaleRotate(border_mode=4)
    with pytest.raises(ValueError):
        albu.ShiftScaleRotate(scale_limit=0.8)
    with pytest.raises(ValueError, match='at most one'):
        albu.Compose([albu.ShiftScaleRotate(), albu.ShiftScaleRotate()])
    with pytest.raises(ValueError, match='RandomCrop must come first'):
        albu.Compose([albu.ShiftScaleRotate(), albu.RandomCrop(8, 8)])


def test_from_config_accepts_both_names():
    mag = aug.from_config(dict(transforms=[('RandomCrop', (16, 16)), ('RandomHorizontalFlip', 0.5),
                                           ('RandomScaleRotate', dict(scale=(0.5, 2.0), degrees=15, prob=0.5)),
                                           ('Normalize', dict(mean=MEAN, std=STD, clamp=True))]), rng=random.Random(0))
    assert isinstance(mag, A.Compose) and mag.param_cols == 8 and mag.affine.degrees == 15
    assert tuple(mag.params(3, 24, 24).shape) == (3, 8)
    al = aug.from_config(dict(transforms=[('RandomCrop', (16, 16)),
                                          ('ShiftScaleRotate', dict(shift_limit=0.05, scale_limit=0.5, rotate_limit=20, p=0.7)),
                                          ('Normalize', dict(mean=MEAN, std=STD, max_pixel_value=1)), ('ToTensor',)]),
                         rng=random.Random(0))
    assert isinstance(al, albu.Compose) and al.param_cols == 8 and al.affine.p == 0.7
    with pytest.raises(ValueError):
        aug.from_config(dict(transforms=[('RandomCrop', (16, 16)), ('RandomScaleRotate', dict(scale=(0.1, 1)))]))
    with pytest.raises(ValueError, match='unknown'):
        aug.from_config(dict(transforms=[('RandomCrop', (16, 16)), ('RandomScale', 0.5)]))
    # a pipeline without the transform keeps today's table
    plain = aug.from_config(dict(transforms=[('RandomCrop', (16, 16)), ('RandomHorizontalFlip', 0.5)]), rng=random.Random(0))
    assert plain.param_cols == 4 and tuple(plain.params(3, 24, 24).shape) == (3, 4)
