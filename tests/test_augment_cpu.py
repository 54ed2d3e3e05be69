"""CPU: the training augmentation of raw tiles (regda_amd.aug, rgda_augment_tiles) -- samplers, tables, the dihedral
codes, the CPU restatement against the reference's own transforms (tests/golden/augment.npz), from_config and the
ABI's argument errors."""
import importlib
import random

import numpy as np
import pytest
import torch

import aug_ref
from regda_amd import aug
from regda_amd.aug import albu, augmentation as A

MEAN = (123.675, 116.28, 103.53)
STD = (58.395, 57.12, 57.375)


def mag(size, rng=None, generator=None, clamp=True):
    return A.Compose([A.RandomCrop(size), A.RandomHorizontalFlip(0.5), A.RandomVerticalFlip(0.5), A.RandomRotate90(0.5),
                      A.Normalize(MEAN, STD, clamp=clamp)], rng=rng, generator=generator)


def test_restatement_matches_the_reference_golden(gold):
    """aug_ref with the golden's (y0, x0, d) and the mag table gives the reference's outputs bit for bit: image (after
    normalise + clamp), soft label and region map of every seed, and the 512 -> 512 case."""
    g = gold('augment.npz')
    lut = mag((32, 32)).table()
    img = torch.from_numpy(g['small_img'])[None]
    soft = torch.from_numpy(g['small_soft'])[None]
    regs = torch.from_numpy(g['small_regs'])[None]
    assert len(set(int(d) for d in g['params'][:, 2])) == 8
    for k, p in enumerate(g['params']):
        prm = torch.tensor([[p[0], p[1], p[2], 0]], dtype=torch.int32)
        r = aug_ref.augment(img, prm, (32, 32), lut, soft=soft, regs=regs)
        assert torch.equal(r['image'][0], torch.from_numpy(g['small_image_out'][k])), k
        assert torch.equal(r['soft'][0], torch.from_numpy(g['small_mask_out'][k])), k
        assert torch.equal(r['regs'][0], torch.from_numpy(g['small_sup_out'][k])), k
    big = torch.from_numpy(g['full_img'])[None]
    r = aug_ref.augment(big, torch.tensor([[0, 0, 0, 0]], dtype=torch.int32), (512, 512), mag((512, 512)).table())
    # the golden's seed drew some element for the full tile: find it among the 8 (the crop is fixed)
    outs = [aug_ref.augment(big, torch.tensor([[0, 0, d, 0]], dtype=torch.int32), (512, 512), mag((512, 512)).table())
            for d in range(8)]
    assert any(torch.equal(o['image'][0], torch.from_numpy(g['full_image_out'])) for o in outs)
    assert r['image'].shape == (1, 3, 512, 512)


@pytest.mark.parametrize('explicit', [False, True])
def test_mag_sampler_draws_the_reference_parameters_and_stream(gold, explicit):
    """Seeded like the golden, the mag sampler gives the same (y0, x0, d) and leaves both generators where the
    reference left them (same number of draws) -- with the global generators and with explicit ones."""
    g = gold('augment.npz')
    for k, s in enumerate(g['seeds']):
        s = int(s)
        if explicit:
            rng, gen = random.Random(s), torch.Generator().manual_seed(s)
            p = mag((32, 32), rng, gen).sample(48, 40)
            nxt = (rng.random(), torch.rand(1, generator=gen).item())
        else:
            random.seed(s)
            torch.manual_seed(s)
            p = mag((32, 32)).sample(48, 40)
            nxt = (random.random(), torch.rand(1).item())
        assert tuple(p) == tuple(int(v) for v in g['params'][k]), s
        assert nxt[0] == g['small_next_py'][k] and np.float32(nxt[1]) == g['small_next_torch'][k], s
    # 512 -> 512: no crop draw; the three flip / rotation draws only
    s = int(g['full_seed'])
    rng, gen = random.Random(s), torch.Generator().manual_seed(s)
    y0, x0, d = mag((512, 512), rng, gen).sample(512, 512)
    assert (y0, x0) == (0, 0)
    assert rng.random() == g['full_next_py'] and np.float32(torch.rand(1, generator=gen).item()) == g['full_next_torch']
    r = aug_ref.augment(torch.from_numpy(g['full_img'])[None], torch.tensor([[0, 0, d, 0]], dtype=torch.int32),
                        (512, 512), mag((512, 512)).table())
    assert torch.equal(r['image'][0], torch.from_numpy(g['full_image_out']))


def test_dihedral_codes_equal_the_flip_and_rot90_chains():
    """The 8 codes on a non-symmetric square, against torch's own ops; and the composition of the two pipelines'
    elements (include/rgda_hip.h)."""
    x = torch.arange(25).view(5, 5) * 3 + torch.arange(5)[:, None] ** 2
    H = lambda t: t.flip(-1)
    V = lambda t: t.flip(-2)
    R = lambda t: torch.rot90(t, 1, [-2, -1])
    chains = {0: x, 4: H(x), 2: V(x), 5: R(x), 6: R(R(x)), 3: R(R(R(x))), 1: x.t(), 7: V(H(x)).t()}
    for d, want in chains.items():
        assert torch.equal(aug_ref.apply_d(x, d), want), d
        assert A.code(A.matrix(d)) == d
    assert len({tuple(aug_ref.apply_d(x, d).flatten().tolist()) for d in range(8)}) == 8
    assert torch.equal(R(x), torch.from_numpy(np.rot90(x.numpy()).copy()))         # torch.rot90 == np.rot90 on HW
    # mag: H then V then R, each optional
    for h in (0, 1):
        for v in (0, 1):
            for r in (0, 1):
                m, y = A.IDENTITY, x
                for on, mm, f in ((h, A.HFLIP, H), (v, A.VFLIP, V), (r, A.ROT90, R)):
                    if on:
                        m, y = m @ mm, f(y)
                assert torch.equal(aug_ref.apply_d(x, A.code(m)), y)
                assert A.code(m) == ((1 | v << 1 | (1 - h) << 2) if r else (v << 1 | h << 2))
    for k in range(4):
        assert torch.equal(aug_ref.apply_d(x, A.code(np.linalg.matrix_power(A.ROT90, k))),
                           torch.from_numpy(np.rot90(x.numpy(), k).copy()))


def test_albumentations_sampler_distribution():
    """~60k seeded draws of the source pipeline: crop origins uniform, the OneOf branch with p = 0.75 and its children
    (H, V, R^k) with equal weight, k uniform -- every frequency within 5 sigma of its binomial expectation."""
    p = aug.from_config(importlib.import_module('configs.ToPotsdam').SOURCE_DATA_CONFIG, rng=random.Random(7))
    n = 60000
    draws = [p.sample(520, 516) for _ in range(n)]
    d = np.array([x[2] for x in draws])
    # not applied (1/4), H (code 4), V (code 2) or R^k (k = 0..3: codes 0, 5, 6, 3), each 3/4 * 1/3
    want = {0: 0.25 + 0.0625, 4: 0.25, 2: 0.25, 5: 0.0625, 6: 0.0625, 3: 0.0625}
    for code in range(8):
        q = want.get(code, 0.0)
        c = int((d == code).sum())
        assert abs(c - n * q) <= 5 * np.sqrt(n * q * (1 - q)) + 1e-9, (code, c, n * q)
    y0 = np.array([x[0] for x in draws])
    x0 = np.array([x[1] for x in draws])
    for arr, span in ((y0, 9), (x0, 5)):
        assert arr.min() == 0 and arr.max() == span - 1
        for v in range(span):
            c = int((arr == v).sum())
            assert abs(c - n / span) <= 5 * np.sqrt(n / span * (1 - 1 / span)), (v, c)


def test_tables():
    """mag: torch `(v - mean) / std` for all 256 values, clamped at 1; albumentations 1.3.0's restated normalize; the
    label table applies the offset and the ignore rule of basedata.py:83-88."""
    v = torch.arange(256, dtype=torch.float32)
    for clamp in (False, True):
        t = A.Normalize(MEAN, STD, clamp=clamp).table()
        for c in range(3):
            want = (v - torch.tensor(MEAN[c], dtype=torch.float32)) / torch.tensor(STD[c], dtype=torch.float32)
            if clamp:
                want = want.clamp(max=1.0)
            assert torch.equal(t[c], want)
    assert A.Normalize(MEAN, STD, clamp=True).table().max() == 1.0
    a = albu.Normalize(MEAN, STD, max_pixel_value=1).table()
    den = np.reciprocal(np.array(STD, np.float32))
    for c in range(3):
        want = (np.arange(256, dtype=np.float32) - np.float32(MEAN[c])) * den[c]
        assert np.array_equal(a[c].numpy(), want)
    for offset in (0, -1):
        lt = A.label_table(offset, 6, -1)
        raw = torch.arange(256) + offset
        raw[raw >= 6] = -1
        assert lt.dtype == torch.int32 and torch.equal(lt.long(), raw)
    assert A.label_table(-1, 6, -1)[0] == -1 and A.label_table(0, 6, 255)[200] == 255


def test_from_config():
    """The configs' declarative lists build the right pipelines; unknown names raise ValueError."""
    for target in ('2potsdam', '2vaihingen'):
        cfg = importlib.import_module('configs.st.regda.' + target)
        p = aug.from_config(cfg.TARGET_DATA_CONFIG)
        assert isinstance(p, A.Compose) and p.crop == (512, 512) and p.norm.clamp
        assert [type(t).__name__ for t in p.transforms] == ['RandomCrop', 'RandomHorizontalFlip', 'RandomVerticalFlip',
                                                            'RandomRotate90', 'Normalize']
        assert torch.equal(p.table(), A.Normalize(cfg.MEAN, cfg.STD, clamp=True).table())
    for ds in ('ToPotsdam', 'ToVaihingen'):
        cfg = importlib.import_module('configs.' + ds)
        s = aug.from_config(cfg.SOURCE_DATA_CONFIG)
        assert isinstance(s, albu.Compose) and s.crop == (512, 512)
        norm = next(t[1] for t in cfg.SOURCE_DATA_CONFIG['transforms'] if t[0] == 'Normalize')
        assert torch.equal(s.table(), albu.Normalize(**norm).table())
        for name in ('EVAL_DATA_CONFIG', 'PSEUDO_DATA_CONFIG', 'TEST_DATA_CONFIG'):
            e = aug.from_config(getattr(cfg, name))
            assert e.crop is None and e.out_size(300, 200) == (300, 200)
            assert all(e.sample(300, 200) == (0, 0, 0) for _ in range(20))
    with pytest.raises(ValueError):
        aug.from_config(dict(transforms=[('RandomCrop', (8, 8)), ('ColorJitter', 0.5)]))
    with pytest.raises(ValueError):
        aug.from_config(dict(transforms=[('OneOf', ('HorizontalFlip', 'Transpose'), 0.5), ('ToTensor',)]))
    with pytest.raises(ValueError):
        aug.from_config(dict(transforms=[('Blur', 3), ('ToTensor',)]))


def test_host_parameter_check():
    from regda_amd import ops
    ok = torch.tensor([[0, 0, 7, 0], [16, 8, 1, 0]], dtype=torch.int32)
    ops.check_augment_params(ok, 48, 40, 32, 32)
    for bad in ([[17, 0, 0, 0]], [[0, 9, 0, 0]], [[-1, 0, 0, 0]], [[0, 0, 8, 0]], [[0, 0, -1, 0]]):
        with pytest.raises(ValueError):
            ops.check_augment_params(torch.tensor(bad, dtype=torch.int32), 48, 40, 32, 32)
    with pytest.raises(ValueError):                 # transposing element, non-square output
        ops.check_augment_params(torch.tensor([[0, 0, 3, 0]], dtype=torch.int32), 48, 40, 32, 24)
    with pytest.raises(ValueError):                 # a rotation drawn for a non-square crop
        p = A.Compose([A.RandomCrop((8, 6)), A.RandomRotate90(1.0)])
        ops.check_augment_params(p.params(1, 16, 16), 16, 16, 8, 6)
    with pytest.raises(ValueError):
        A.Compose([A.RandomHorizontalFlip(0.5), A.RandomCrop((8, 8))])


def test_abi_argument_errors_without_a_gpu():
    """rgda_augment_tiles validates its arguments before any launch (in the style of tests/test_abi.py)."""
    import ctypes
    from regda_amd import _lib
    L = _lib.lib()
    buf = ctypes.create_string_buffer(64)
    f = ctypes.addressof(buf)           # 16-byte aligned host address: never dereferenced, the checks fail first
    f = f + (-f) % 16
    good = (f, 0, 0, 0, f, 2, 48, 40, 0, 32, 32, f, 0, f, 0, 0, 0, 0, None)

    def call(**kw):
        names = ['img', 'label', 'soft', 'regs', 'params', 'N', 'Hi', 'Wi', 'C', 'Ho', 'Wo', 'lut', 'label_lut',
                 'img_out', 'label_out', 'soft_out', 'regs_out', 'flag', 'stream']
        a = dict(zip(names, good))
        a.update(kw)
        L.call('rgda_augment_tiles', *[a[k] or None if k not in ('N', 'Hi', 'Wi', 'C', 'Ho', 'Wo') else a[k]
                                       for k in names])
    for kw in (dict(img=0), dict(N=0), dict(Ho=49), dict(Wo=41), dict(params=0), dict(lut=0), dict(img_out=0),
               dict(img=f + 1), dict(label=f), dict(label=f, label_lut=f), dict(soft=f, C=0, soft_out=f),
               dict(soft=f, C=6), dict(regs=f)):
        with pytest.raises(ValueError):
            call(**kw)
    with pytest.raises(ValueError, match='not supported'):      # more soft channels than a tile's LDS holds
        call(soft=f, C=9, soft_out=f)
