"""GPU: rgda_augment_tiles against the reference's own transforms (tests/golden/augment.npz) and the CPU restatement
(tests/aug_ref.py) bit for bit, and DevicePrefetcher(augment=...) against CPU-prepared batches staged the current way,
down to two SSL steps."""
import importlib
import random

import numpy as np
import pytest
import torch

import aug_ref
from oracle import model as omodel
from regda_amd import aug
from regda_amd.aug import albu, augmentation as A

pytestmark = pytest.mark.gpu

MEAN = (123.675, 116.28, 103.53)
STD = (58.395, 57.12, 57.375)


def mag(size, rng=None, generator=None, **kw):
    return A.Compose([A.RandomCrop(size), A.RandomHorizontalFlip(0.5), A.RandomVerticalFlip(0.5), A.RandomRotate90(0.5),
                      A.Normalize(MEAN, STD, clamp=True)], rng=rng, generator=generator, **kw)


def source(size, rng=None, **kw):
    return albu.Compose([albu.RandomCrop(*size), albu.OneOf([albu.HorizontalFlip(True), albu.VerticalFlip(True),
                                                             albu.RandomRotate90(True)], p=0.75),
                         albu.Normalize(MEAN, STD, max_pixel_value=1), albu.ToTensor()], rng=rng, **kw)


def test_kernel_reproduces_the_reference_golden(gold):
    """Per tile through Compose (seeded as the golden: same draws) and as one Compose.batch launch with the golden's
    parameters: image, soft label and region map bit for bit; the 512 -> 512 case too."""
    g = gold('augment.npz')
    img = torch.from_numpy(g['small_img'])
    soft = torch.from_numpy(g['small_soft'])
    regs = torch.from_numpy(g['small_regs'])
    for k, s in enumerate(g['seeds']):
        s = int(s)
        r = mag((32, 32), random.Random(s), torch.Generator().manual_seed(s))(img, mask=soft, mask_sup=regs)
        assert torch.equal(r['image'].cpu(), torch.from_numpy(g['small_image_out'][k])), s
        assert torch.equal(r['mask'].cpu(), torch.from_numpy(g['small_mask_out'][k])), s
        assert r['mask_sup'].dtype == torch.int64 and torch.equal(r['mask_sup'].cpu(), torch.from_numpy(g['small_sup_out'][k]))
    n = len(g['seeds'])
    prm = torch.zeros(n, 4, dtype=torch.int32)
    prm[:, :3] = torch.from_numpy(g['params'])
    r = mag((32, 32)).batch(img[None].expand(n, -1, -1, -1), soft=soft[None].expand(n, -1, -1, -1),
                            mask_sup=regs[None].expand(n, -1, -1), params=prm)
    assert torch.equal(r['image'].cpu(), torch.from_numpy(g['small_image_out']))
    assert torch.equal(r['soft'].cpu(), torch.from_numpy(g['small_mask_out']))
    assert torch.equal(r['mask_sup'].cpu(), torch.from_numpy(g['small_sup_out']))
    s = int(g['full_seed'])
    r = mag((512, 512), random.Random(s), torch.Generator().manual_seed(s))(torch.from_numpy(g['full_img']))
    assert torch.equal(r['image'].cpu(), torch.from_numpy(g['full_image_out']))


def _raw(n, h, w, c=6, seed=0):
    g = torch.Generator().manual_seed(seed)
    return dict(img=torch.randint(0, 256, (n, h, w, 3), generator=g, dtype=torch.uint8),
                label=torch.randint(0, 256, (n, h, w), generator=g, dtype=torch.uint8),
                soft=torch.rand(n, c, h, w, generator=g),
                regs=torch.randint(0, 1 << 20, (n, h, w), generator=g, dtype=torch.int32))


@pytest.mark.parametrize('hw', [512, 1024])
def test_full_size_matches_the_restatement(hw):
    """8 x hw^2 -> 512 crops, each of the 8 elements forced in turn plus drawn ones, both tables, with and without the
    label / soft / region inputs: torch.equal with aug_ref."""
    from regda_amd import ops
    n = 8
    raw = _raw(n, hw, hw, seed=hw)
    dev = {k: v.cuda() for k, v in raw.items()}
    rng = random.Random(hw)
    for pipe in (mag((512, 512), rng, torch.Generator().manual_seed(hw)), source((512, 512), rng, offset=-1)):
        lut, llut = pipe.device_tables('cuda')
        for force in list(range(8)) + [None]:
            prm = pipe.params(n, hw, hw)
            if force is not None:
                prm[:, 2] = force
            want = aug_ref.augment(raw['img'], prm, (512, 512), pipe.table(), raw['label'], pipe.label_table(),
                                   raw['soft'], raw['regs'])
            got = ops.augment_tiles(dev['img'], prm, lut, (512, 512), dev['label'], llut, dev['soft'], dev['regs'])
            for k in ('image', 'label', 'soft', 'regs'):
                assert torch.equal(got[k].cpu(), want[k]), (type(pipe).__module__, force, k)
        # null pointers: each optional input left out alone, then all of them
        prm = pipe.params(n, hw, hw)
        want = aug_ref.augment(raw['img'], prm, (512, 512), pipe.table(), raw['label'], pipe.label_table(), raw['soft'],
                               raw['regs'])
        for drop in ('label', 'soft', 'regs', 'all'):
            kw = dict(label=dev['label'], label_lut=llut, soft=dev['soft'], regs=dev['regs'])
            for k in (('label', 'soft', 'regs') if drop == 'all' else (drop,)):
                kw[k] = None
            got = ops.augment_tiles(dev['img'], prm, lut, (512, 512), **kw)
            assert torch.equal(got['image'].cpu(), want['image'])
            for k in ('label', 'soft', 'regs'):
                assert (got[k] is None) if kw[k] is None else torch.equal(got[k].cpu(), want[k]), (drop, k)


def test_odd_shapes_and_device_side_parameter_check():
    """Tiles that do not fill the 32 x 32 grid (scalar stores), a 4-byte-unaligned HWC row stride, a non-square crop;
    device-side params that leave the input set the flag and leave the sample unwritten."""
    from regda_amd import ops
    raw = _raw(3, 45, 37, c=3, seed=5)
    dev = {k: v.cuda() for k, v in raw.items()}
    for ho, wo, ds in ((27, 27, range(8)), (20, 30, (0, 2, 4, 6)), (45, 36, (0, 6))):
        pipe = A.Compose([A.RandomCrop((ho, wo)), A.Normalize(MEAN, STD)], generator=torch.Generator().manual_seed(ho))
        lut, llut = pipe.device_tables('cuda')
        for d in ds:
            prm = pipe.params(3, 45, 37)
            prm[:, 2] = d
            want = aug_ref.augment(raw['img'], prm, (ho, wo), pipe.table(), raw['label'], pipe.label_table(),
                                   raw['soft'], raw['regs'])
            got = ops.augment_tiles(dev['img'], prm, lut, (ho, wo), dev['label'], llut, dev['soft'], dev['regs'])
            for k in ('image', 'label', 'soft', 'regs'):
                assert torch.equal(got[k].cpu(), want[k]), (ho, wo, d, k)
    flag = torch.zeros(1, dtype=torch.int32, device='cuda')
    bad = torch.tensor([[0, 0, 0, 0], [19, 0, 0, 0], [0, 0, 9, 0]], dtype=torch.int32, device='cuda')
    out = {'image': torch.full((3, 3, 27, 27), 7.0, device='cuda')}
    lut, _ = A.Compose([A.Normalize(MEAN, STD)]).device_tables('cuda')
    ops.augment_tiles(dev['img'], bad, lut, (27, 27), out=out, flag=flag)
    assert flag.item() == 1
    assert (out['image'][1:] == 7.0).all() and not (out['image'][0] == 7.0).all()


@pytest.mark.parametrize('offset', [0, -1])
def test_labels_map_to_ignore(offset):
    """Every byte 0..255 as a label with n_classes = 6: byte + offset, >= 6 -> ignore_label (basedata.py:83-88)."""
    lab = torch.arange(256, dtype=torch.uint8).view(1, 16, 16).expand(2, 16, 16).contiguous()
    img = torch.zeros(2, 16, 16, 3, dtype=torch.uint8)
    pipe = A.Compose([A.Normalize(MEAN, STD)], offset=offset, num_class=6, ignore_label=-1)
    r = pipe.batch(img, mask=lab)
    v = torch.arange(256) + offset
    want = torch.where(v >= 6, torch.full_like(v, -1), v).view(16, 16)
    assert r['mask'].dtype == torch.int64 and torch.equal(r['mask'].cpu(), want.expand(2, 16, 16))


def _build(rt='resnet17t'):
    from regda_amd.models.Encoder import Deeplabv2
    m = Deeplabv2(dict(backbone=dict(resnet_type=rt, output_stride=16, pretrained=False), multi_layer=True,
                       cascade=False, use_ppm=True, ppm=dict(num_classes=6, use_aux=False, fc_dim=2048),
                       inchannels=2048, num_classes=6, is_ins_norm=True))
    m.load_state_dict(omodel.init_state_dict(rt, 6, seed=3), strict=True)
    m.set_drop_masks(torch.ones(2, 512), torch.ones(2, 512))
    return m


def _raw_batches(k, n=2, hw=80):
    out = []
    for i in range(k):
        r = _raw(n, hw, hw, seed=100 + i)
        r['label'] = (r['label'] % 7).to(torch.uint8)          # 0..5 and 6 (-> ignore)
        r['regs'] = r['regs'] % 40
        out.append(dict(images_s=r['img'], label_s=r['label'], images_t=_raw(n, hw, hw, seed=200 + i)['img'],
                        soft_t=torch.softmax(3 * r['soft'], 1), regs_t=r['regs']))
    return out


def _pipes(seed):
    return (source((64, 64), random.Random(seed)),
            mag((64, 64), random.Random(seed + 1), torch.Generator().manual_seed(seed + 2)))


def _prepared(raw, k, seed):
    """The CPU-prepared batches of the first k stages: the same pipelines with the same seeds, drawing source then
    target per batch, as the prefetcher does."""
    ps, pt = _pipes(seed)
    out = []
    for i in range(k):
        b = raw[i % len(raw)]
        n, h, w, _ = b['images_s'].shape
        s = aug_ref.augment(b['images_s'], ps.params(n, h, w), (64, 64), ps.table(), b['label_s'], ps.label_table())
        t = aug_ref.augment(b['images_t'], pt.params(n, h, w), (64, 64), pt.table(), soft=b['soft_t'],
                            regs=b['regs_t'])
        out.append(dict(images_s=s['image'], label_s=s['label'], images_t=t['image'], soft_t=t['soft'],
                        regs_t=t['regs']))
    return out


def _augment_arg(seed):
    ps, pt = _pipes(seed)
    return [(ps, dict(image='images_s', mask='label_s')),
            (pt, dict(image='images_t', soft='soft_t', mask_sup='regs_t'))]


def test_prefetcher_depth2_delivers_the_cpu_prepared_batches():
    from regda_amd.utils.prefetch import DevicePrefetcher
    raw = _raw_batches(3)
    want = _prepared(raw, 7, seed=11)
    pf = DevicePrefetcher(raw, depth=2, augment=_augment_arg(11))
    assert pf.bytes_per_batch == sum(v.numel() * v.element_size() for v in raw[0].values())
    for i in range(7):
        b = pf.next()
        torch.cuda.synchronize()
        for k, v in want[i].items():
            assert b[k].dtype == v.dtype and torch.equal(b[k].cpu(), v), (i, k)
        pf.release()


def test_prefetcher_into_static_inputs_gives_bit_identical_steps():
    """Two recorded SSL steps fed (a) CPU-prepared batches staged the current way and (b) raw batches augmented by the
    prefetcher straight into the step's static inputs: the same tensors, bit-identical losses and prototypes."""
    from regda_amd.ssl import SSLStep
    from regda_amd.utils.prefetch import DevicePrefetcher
    raw = _raw_batches(2)
    prep = _prepared(raw, 3, seed=21)
    results = []
    for path in ('prepared', 'augment'):
        st = SSLStep(_build(), torch.zeros(6, 2048))
        g0 = {k: v.cuda() for k, v in prep[0].items()}
        st.step(g0['images_s'], g0['label_s'], g0['images_t'], g0['soft_t'], g0['regs_t'], 1e-3)
        st.record_plan(g0['images_s'], g0['label_s'], g0['images_t'], g0['soft_t'], g0['regs_t'])
        if path == 'prepared':
            pf = DevicePrefetcher(prep[1:] + prep[:1], into=st.static_inputs())
        else:
            # the first stage's draws were used by the eager + recorded steps above: draw and drop them
            aug_arg = _augment_arg(21)
            for pipe, roles in aug_arg:
                pipe.params(2, 80, 80)
            pf = DevicePrefetcher(raw[1:] + raw[:1], into=st.static_inputs(), augment=aug_arg)
        losses = []
        for i in range(2):
            b = pf.next()
            out = st.step(b['images_s'], b['label_s'], b['images_t'], b['soft_t'], b['regs_t'], 1e-3)
            torch.cuda.synchronize()
            for k, v in prep[1 + i].items():
                assert torch.equal(b[k].cpu(), v), (path, i, k)
            pf.release(st.inputs_consumed())
            losses.append([x.cpu() for x in out])
        torch.cuda.synchronize()
        results.append((losses, st.prototypes.cpu().clone()))
    (la, pa), (lb, pb) = results
    for a, b in zip(la, lb):
        for x, y in zip(a, b):
            assert torch.equal(x, y)
    assert torch.equal(pa, pb)


def test_normalise_only_pipeline_feeds_pre_slide():
    """EVAL_DATA_CONFIG (normalise only) on raw tiles feeds pre_slide the same input as the CPU-normalised image."""
    from regda_amd.utils.tools import pre_slide
    cfg = importlib.import_module('configs.ToPotsdam')
    pipe = aug.from_config(cfg.EVAL_DATA_CONFIG)
    img = _raw(1, 96, 80, seed=9)['img']
    r = pipe(img[0])
    norm = next(t[1] for t in cfg.EVAL_DATA_CONFIG['transforms'] if t[0] == 'Normalize')
    mean = np.array(norm['mean'], np.float32) * np.float32(norm['max_pixel_value'])
    den = np.reciprocal(np.array(norm['std'], np.float32) * np.float32(norm['max_pixel_value']))
    cpu = (img[0].numpy().astype(np.float32) - mean) * den          # albumentations 1.3.0 normalize, HWC
    cpu = torch.from_numpy(np.ascontiguousarray(cpu.transpose(2, 0, 1)))[None]
    assert torch.equal(r['image'][None].cpu(), cpu)

    def model(x):               # any deterministic map of the tile
        return torch.cat([x, x * x], 1)[:, :5].contiguous()
    got = pre_slide(model, r['image'][None], num_classes=5, tile_size=(64, 64))
    want = pre_slide(model, cpu.cuda(), num_classes=5, tile_size=(64, 64))
    assert torch.equal(got, want)
