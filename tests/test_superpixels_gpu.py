"""GPU: rgda_superpixels and rgda_region_shrink bit for bit against the numpy restatement of their specification
(tests/superpixel_ref.py) and the reference's own edge_shrinking (tests/golden/edge_shrink.npz); SuperPixelsSLIC in front
of Homogenizer; DevicePrefetcher(augment=..., regions=...)."""
import functools
import random

import numpy as np
import pytest
import torch

import aug_ref
import superpixel_ref as R
from regda_amd import ops
from regda_amd.aug import augmentation as A
from regda_amd.gast.superpixels import SuperPixelsSLIC, edge_shrinking

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _image(name):
    return dict(diagonal=lambda: R.diagonal_image(64, 64), constant=lambda: np.full((32, 32, 3), 77, np.uint8),
                noise=lambda: R.blurred_noise(64, 96, 1), noise64=lambda: R.blurred_noise(64, 64, 2),
                scene64=lambda: R.rectangle_scene(64, 64, 4, count=10), scene512=lambda: R.rectangle_scene(512, 512, 5),
                noise80a=lambda: R.blurred_noise(80, 80, 6), noise80b=lambda: R.rectangle_scene(80, 80, 7, count=12))[name]()


@functools.lru_cache(maxsize=None)
def _oracle(name, S, m, iters, min_area):
    """(regs, count, centres of the last Assign) of the restatement, computed once per case."""
    img = _image(name)
    labels, centres = R.slic_labels(img, S, m, iters)
    regs, count = R.number(R.components(labels), min_area)
    return regs, count, centres


def _gpu(imgs, S, m, iters, min_area):
    """-> regs, count as numpy, and the workspace's centres of the last Assign [N][K][5]."""
    t = torch.from_numpy(np.stack(imgs)).cuda()
    n, h, w, _ = t.shape
    ws = torch.empty(ops.lib().size('rgda_superpixels_workspace', n, h, w, S), dtype=torch.uint8, device='cuda')
    regs, count = ops.superpixels(t, S, m, iters, min_area, ws=ws)
    torch.cuda.synchronize()
    k = (h // S) * (w // S)
    centres = ws[:2 * n * k * 5 * 4].view(torch.int32).view(2, n, k, 5)[iters & 1]
    return regs.cpu().numpy(), count.cpu().numpy(), centres.cpu().numpy()


def _check(name, S, m, iters, min_area):
    want, cnt, ctr = _oracle(name, S, m, iters, min_area)
    regs, count, centres = _gpu([_image(name)], S, m, iters, min_area)
    assert regs.dtype == np.int32 and count.dtype == np.int32
    assert np.array_equal(centres[0], ctr), 'centres of the last Assign differ'
    assert int(count[0]) == cnt
    assert np.array_equal(regs[0], want)
    return regs[0], cnt


@pytest.mark.parametrize('iters', [1, 5])
def test_diagonal_edge_on_a_4x4_grid(iters):
    """64 x 64, S = 16: most cells have fewer than 9 neighbours; two flat colours split by the diagonal."""
    regs, cnt = _check('diagonal', 16, 10, iters, 64)
    assert cnt >= 4


@pytest.mark.parametrize('iters', [1, 4])
def test_constant_image_ties(iters):
    """Every colour term ties: the position term and the lowest-k rule decide.  One might expect the grid
    itself; the specification gives the grid moved by one pixel instead, because Update rounds half up: the first centres sit
    at 8 g + 4, so rows / columns 8 g + 8 are equally far from cells g and g + 1 and go to the smaller k
    (tests/test_superpixels_cpu.py: test_constant_image_follows_the_tie_rule derives it).  Asserted here: bit-exact
    against the restatement, and for one iteration that closed form -- 16 regions numbered in cell order."""
    regs, cnt = _check('constant', 8, 10, iters, 16)
    assert cnt == 16
    if iters == 1:
        cell = np.maximum(np.arange(32) - 1, 0) // 8
        assert np.array_equal(regs, cell[:, None] * 4 + cell[None, :] + 1)


def test_fragmenting_noise_non_square():
    """64 x 96, S = 8, min_area = 16: the labels fragment, so components are dropped and kept."""
    labels, _ = R.slic_labels(_image('noise'), 8, 10, 10)
    area = np.bincount(R.components(labels).reshape(-1))
    area = area[area > 0]
    assert (area < 16).sum() >= 1 and (area >= 16).sum() >= 8          # on the numpy result: the input is not degenerate
    regs, cnt = _check('noise', 8, 10, 10, 16)
    assert (regs == 0).any() and cnt >= 8


def test_batch_of_three_equals_three_single_calls():
    names = ('diagonal', 'noise64', 'scene64')
    regs, count, centres = _gpu([_image(k) for k in names], 16, 10, 4, 20)
    for i, k in enumerate(names):
        r1, c1, t1 = _gpu([_image(k)], 16, 10, 4, 20)
        assert np.array_equal(regs[i], r1[0]) and count[i] == c1[0] and np.array_equal(centres[i], t1[0]), k
        want, cnt, ctr = _oracle(k, 16, 10, 4, 20)
        assert np.array_equal(regs[i], want) and count[i] == cnt and np.array_equal(centres[i], ctr), k
    assert len({int(c) for c in count}) > 1                             # the three images do differ


def test_real_tile_512():
    """One 512 x 512 tile, S = 16, 10 iterations: a few dozen rectangles plus mild noise."""
    gen = SuperPixelsSLIC(16, 10, 10)
    regs, cnt = _check('scene512', 16, 10, 10, gen.min_area)
    assert 0 < cnt < gen.max_regions(512, 512) and regs.max() == cnt


@pytest.mark.parametrize('win', [1, 3])
def test_region_shrink_equals_the_reference_golden(gold, win):
    g = gold('edge_shrink.npz')
    names = ('grid', 'thin', 'blocky')
    batch = torch.from_numpy(np.stack([g[k] for k in names])).cuda()
    for fill in (int(g['fill']), 0):
        out = ops.region_shrink(batch, win, fill).cpu().numpy()
        for i, k in enumerate(names):
            want = g['%s_win%d' % (k, win)]
            if fill == 0:       # the restatement, which equals the golden at the reference's fill (CPU test)
                want = R.shrink(g[k], win, 0)
            assert np.array_equal(out[i], want), (k, win, fill)
    # the module-level mirror: fill=None is the reference's cnt_sup, and a numpy map comes back as numpy
    out = edge_shrinking(g['thin'], win_size=win, region_size=16)
    assert isinstance(out, np.ndarray) and np.array_equal(out, g['thin_win%d' % win])
    # a map that is no multiple of the kernel's tile, and wider than one tile
    m = np.random.default_rng(3).integers(0, 3, (9, 11)).astype(np.int32)[np.arange(70)[:, None] // 8, np.arange(45)[None] // 5]
    assert np.array_equal(ops.region_shrink(torch.from_numpy(m).cuda(), win, -7).cpu().numpy(), R.shrink(m, win, -7))


def test_generator_in_front_of_lrh():
    """SuperPixelsSLIC -> Homogenizer(max_regions=gen.max_regions) equals ops.lrh on the restatement's map; two calls on
    the same input are identical."""
    from regda_amd.utils.local_region_homog import Homogenizer
    gen = SuperPixelsSLIC(8, 10, 10, min_area=16)
    img = _image('noise')
    H, W = img.shape[:2]
    number, label = gen.get_super_pixels(img)
    want, cnt, _ = _oracle('noise', 8, 10, 10, 16)
    assert number == cnt and isinstance(label, np.ndarray) and np.array_equal(label, want)
    t = torch.from_numpy(img).cuda()
    number2, label2 = gen.get_super_pixels(t)
    assert number2 == cnt and torch.is_tensor(label2) and np.array_equal(label2.cpu().numpy(), want)
    regs, count = gen(t[None])
    regs_b, count_b = gen(t[None])
    assert torch.equal(regs, regs_b) and torch.equal(count, count_b)
    hard = torch.from_numpy(np.random.default_rng(5).integers(-1, 6, (1, H, W))).cuda()
    # blocks of one class so that some regions do pass the percentage
    hard[0, :32] = hard[0, :32].clamp(max=0)
    lrh = Homogenizer(percent=0.5, class_num=6, ignore_label=-1, max_regions=gen.max_regions(H, W))
    got = lrh(hard, regs.long())
    ref = ops.lrh(hard, torch.from_numpy(want).cuda().long()[None], 0.5, 6, -1, gen.max_regions(H, W))
    assert torch.equal(got, ref)
    assert not torch.equal(got, hard)                                   # LRH did change labels on these regions


def test_prefetcher_generates_the_region_maps():
    """A raw 2-image target batch without `mask_sup`: the delivered region map is the restatement's map pushed through
    the augmentation's geometry with the same parameters.  A batch that carries `mask_sup` is delivered as before."""
    from regda_amd.utils.prefetch import DevicePrefetcher
    MEAN, STD = (123.675, 116.28, 103.53), (58.395, 57.12, 57.375)

    def pipe(seed):
        return A.Compose([A.RandomCrop((64, 64)), A.RandomHorizontalFlip(0.5), A.RandomVerticalFlip(0.5),
                          A.RandomRotate90(0.5), A.Normalize(MEAN, STD, clamp=True)], rng=random.Random(seed),
                         generator=torch.Generator().manual_seed(seed + 1))
    names = ('noise80a', 'noise80b')
    imgs = torch.from_numpy(np.stack([_image(k) for k in names]))
    soft = torch.softmax(torch.randn(2, 6, 80, 80, generator=torch.Generator().manual_seed(1)), 1)
    oracle = torch.from_numpy(np.stack([_oracle(k, 8, 10, 5, 16)[0] for k in names]))
    gen = SuperPixelsSLIC(8, 10, 5, min_area=16)
    roles = dict(image='images_t', soft='soft_t', mask_sup='regs_t')
    for host in (dict(images_t=imgs, soft_t=soft), dict(images_t=imgs, soft_t=soft, regs_t=None)):
        pf = DevicePrefetcher([host], depth=2, augment=[(pipe(31), roles)], regions=gen)
        ref = pipe(31)
        for i in range(3):
            b = pf.next()
            torch.cuda.synchronize()
            want = aug_ref.augment(imgs, ref.params(2, 80, 80), (64, 64), ref.table(), soft=soft, regs=oracle)
            assert b['regs_t'].dtype == torch.int64 and tuple(b['regs_t'].shape) == (2, 1, 64, 64)
            assert torch.equal(b['regs_t'].cpu(), want['regs']), i
            assert torch.equal(b['images_t'].cpu(), want['image']) and torch.equal(b['soft_t'].cpu(), want['soft'])
            pf.release()
    # a batch that brings its own map: delivered unchanged (through the same geometry), with and without `regions`
    own = torch.from_numpy(np.random.default_rng(9).integers(0, 40, (2, 80, 80)).astype(np.int32))
    host = dict(images_t=imgs, soft_t=soft, regs_t=own)
    got = []
    for regions in (gen, None):
        pf = DevicePrefetcher([host], depth=2, augment=[(pipe(33), roles)], regions=regions)
        b = pf.next()
        torch.cuda.synchronize()
        got.append(b['regs_t'].cpu().clone())
    ref = pipe(33)
    want = aug_ref.augment(imgs, ref.params(2, 80, 80), (64, 64), ref.table(), soft=soft, regs=own)
    assert torch.equal(got[0], want['regs']) and torch.equal(got[1], want['regs'])
