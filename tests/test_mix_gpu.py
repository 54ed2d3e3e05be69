"""GPU: rgda_domain_mix (ops.domain_mix, regda_amd.utils.classmix / cutmix, DevicePrefetcher(mix=...)) bit for bit against
the reference's own functions (tests/golden/mix.npz) and the numpy restatement (tests/mix_ref.py), down to an SSL step
on a mixed batch.  Every comparison goes through an integer view, so the NaN payloads of untouched pixels count."""
import itertools
import random

import numpy as np
import pytest
import torch

import mix_ref
from mix_ref import bits_equal, golden_cases

pytestmark = pytest.mark.gpu


def rand_inputs(rng, n, h, w, C, label_s=None):
    """Random-bit f32 images and soft planes (NaNs and infinities included), labels in [-1, C), region ids > 0."""
    bits = lambda *s: rng.integers(0, 1 << 32, s, dtype=np.uint32).view(np.float32)
    if label_s is None:
        label_s = rng.integers(-1, C, (n, h, w)).astype(np.int64)
    return dict(img_s=bits(n, 3, h, w), label_s=label_s, img_t=bits(n, 3, h, w),
                label_t=rng.integers(-1, C, (n, h, w)).astype(np.int64), soft_t=bits(n, C, h, w),
                regs_t=rng.integers(1, 1000, (n, 1, h, w)).astype(np.int64))


def dev(a, offset=False):
    """numpy -> device tensor; offset: a contiguous view that starts one element into its buffer (4 or 8 bytes: not
    16-byte aligned) with a guard element on either side."""
    if a is None:
        return None
    t = torch.from_numpy(np.ascontiguousarray(a))
    if not offset:
        return t.cuda()
    buf = torch.zeros(t.numel() + 2, dtype=t.dtype, device='cuda')
    v = buf[1:-1].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 != 0 and v.is_contiguous()
    return v


def check(inp, C, use=('label_t', 'soft_t', 'regs_t'), offset=False, ignore_label=-1, **pred):
    """ops.domain_mix on the device against mix_ref: every target tensor, the sources and the flag."""
    from regda_amd import ops
    t = {k: dev(v if k in ('img_s', 'label_s', 'img_t') or k in use else None, offset) for k, v in inp.items()}
    flag = torch.zeros(1, dtype=torch.int32, device='cuda')
    out = ops.domain_mix(t['img_s'], t['label_s'], t['img_t'], label_t=t['label_t'], soft_t=t['soft_t'], regs_t=t['regs_t'],
                         ignore_label=ignore_label, class_num=C, flag=flag, **pred)
    torch.cuda.synchronize()
    assert out[0] is t['img_t'] and out[1] is t['label_t'] and out[2] is t['soft_t'] and out[3] is t['regs_t']
    opt = {k: (inp[k] if k in use else None) for k in ('label_t', 'soft_t', 'regs_t')}
    img, lab, soft, regs, rflag, cond = mix_ref.domain_mix(inp['img_s'], inp['label_s'], inp['img_t'], C=C,
                                                           ignore_label=ignore_label, **opt, **pred)
    for name, want in (('img_t', img), ('label_t', lab), ('soft_t', soft), ('regs_t', regs), ('img_s', inp['img_s']),
                       ('label_s', inp['label_s'])):
        if want is None:
            assert t[name] is None
        else:
            assert bits_equal(t[name].cpu().numpy(), want), (name, pred)
    assert int(flag.item()) == rflag
    return cond, rflag


def test_goldens_through_ops_and_both_wrappers(gold):
    from regda_amd import ops
    from regda_amd.utils.classmix import classmix
    from regda_amd.utils.cutmix import cutmix
    g = gold('mix.npz')
    ig = int(g['ignore_label'])
    for C, kind, k, (img_s, lab_s, img_t, lab_t), pred, want_img, want_lab in golden_cases(g):
        d = [torch.from_numpy(a).cuda() for a in (img_s, lab_s, img_t, lab_t)]
        it, lt = d[2].clone(), d[3].clone()
        ops.domain_mix(d[0], d[1], it, label_t=lt, ignore_label=ig, class_num=C, check=True, **pred)
        assert bits_equal(it.cpu().numpy(), want_img) and bits_equal(lt.cpu().numpy(), want_lab), (C, kind, k)
        if kind == 'class':
            torch.manual_seed(int(g['class_seeds'][k]))         # the wrapper draws the reference's classes itself
            ds, ts, dt, tt = classmix(d[0], d[1][:, None], d[2], d[3][:, None], ratio=float(g['ratio']), class_num=C, ignore_label=ig)
            assert ts.shape == tt.shape == lab_s.shape and ts.dtype == tt.dtype == torch.int64
            # the unmixed targets_s: the reference returns it with C written over ignore_label (tools.py:413)
            ref_s = g['c%d_class_lab_s_out' % C][k]
            assert np.array_equal(np.where(lab_s == ig, C, lab_s), ref_s) and bits_equal(ts.cpu().numpy(), lab_s)
            ds2, _, dt2, tt2 = classmix(d[0], d[1], d[2], d[3], class_num=C, ignore_label=ig, class_ids=pred['classes'])
            assert bits_equal(dt2.cpu().numpy(), want_img) and bits_equal(tt2.cpu().numpy(), want_lab)
        else:
            np.random.seed(int(g['box_seeds'][k]))
            ds, ts, dt, tt = cutmix(d[0], d[1], d[2], d[3], alpha=1.0)
            assert bits_equal(ts.cpu().numpy(), lab_s)
            _, _, dt2, tt2 = cutmix(d[0], d[1], d[2], d[3], box=pred['box'])
            assert bits_equal(dt2.cpu().numpy(), want_img) and bits_equal(tt2.cpu().numpy(), want_lab)
        assert bits_equal(dt.cpu().numpy(), want_img) and bits_equal(tt.cpu().numpy(), want_lab), (C, kind, k)
        assert bits_equal(ds.cpu().numpy(), img_s)
        for a, b in zip(d, (img_s, lab_s, img_t, lab_t)):      # the wrappers work on clones
            assert bits_equal(a.cpu().numpy(), b)


def quad_labels(rng, n, h, w, C):
    """Source labels for the 16-byte path: 8-pixel runs of one class (whole quads pasted or not), then single pixels
    redrawn in every 5th row (partly pasted quads)."""
    lab = np.repeat(rng.integers(-1, C, (n, h, w // 8)), 8, axis=2).astype(np.int64)
    lab[:, ::5, 1::3] = rng.integers(-1, C, lab[:, ::5, 1::3].shape)
    return lab


def quad_kinds(cond):
    q = cond.reshape(cond.shape[0], cond.shape[1], -1, 4).sum(-1)
    return {'full': int((q == 4).sum()), 'part': int(((q > 0) & (q < 4)).sum()), 'none': int((q == 0).sum())}


def test_scalar_path_with_ragged_edges():
    rng = np.random.default_rng(1)
    inp = rand_inputs(rng, 3, 19, 23, 6)
    cond, _ = check(inp, 6, classes=[0, 3, 4])
    assert cond.any() and not cond.all() and cond[:, :, -1].any() and cond[:, :, 20:].any()
    for box in ((3, 17, 5, 22), (0, 19, 21, 23), (18, 19, 0, 23), (2, 9, 3, 4)):
        check(inp, 6, box=box)


@pytest.mark.parametrize('offset', [False, True], ids=['aligned', 'offset-by-one-element'])
def test_vector_path_full_partial_and_untouched_quads(offset):
    """2 x 32 x 64: W % 4 == 0, so aligned tensors take the 16-byte path and the same tensors one element into their
    buffers fall to the element path; both must give the restatement's bits."""
    rng = np.random.default_rng(2)
    inp = rand_inputs(rng, 2, 32, 64, 6, quad_labels(rng, 2, 32, 64, 6))
    cond, _ = check(inp, 6, offset=offset, classes=[1, 2, 5])
    kinds = quad_kinds(cond)
    assert min(kinds.values()) > 20, kinds
    for box in ((4, 28, 8, 40), (4, 28, 6, 41), (0, 32, 0, 64), (31, 32, 61, 64)):      # quad-aligned, ragged, full, corner
        check(inp, 6, offset=offset, box=box)
    check(inp, 6, offset=offset, use=(), classes=[0])


def test_sixteen_classes_with_soft_planes():
    rng = np.random.default_rng(3)
    inp = rand_inputs(rng, 2, 32, 64, 16, quad_labels(rng, 2, 32, 64, 16))
    cond, _ = check(inp, 16, classes=[0, 3, 7, 8, 11, 12, 15, 14])
    assert min(quad_kinds(cond).values()) > 20
    check(inp, 16, box=(5, 20, 7, 33))
    inp = rand_inputs(rng, 2, 9, 10, 16)
    check(inp, 16, classes=[15, 1, 2, 9])


def test_more_quads_than_one_grid_pass():
    """8 x 512 x 512 is 2048 workgroups of quads, the grid's cap: 9 images make every thread walk a second quad."""
    rng = np.random.default_rng(4)
    n, h, w = 9, 512, 512
    lab = quad_labels(rng, n, h, w, 6)
    inp = dict(img_s=rng.integers(0, 1 << 32, (n, 3, h, w), dtype=np.uint32).view(np.float32), label_s=lab,
               img_t=np.zeros((n, 3, h, w), np.float32), label_t=np.full((n, h, w), -1, np.int64), soft_t=None, regs_t=None)
    cond, _ = check(inp, 6, use=('label_t',), classes=[0, 4])
    assert cond[8].any() and cond[0].any()


def test_edge_cases_in_both_modes():
    rng = np.random.default_rng(5)
    C, (n, h, w) = 6, (2, 16, 24)
    inp = rand_inputs(rng, n, h, w, C, quad_labels(rng, n, h, w, C))
    assert (inp['label_s'] == -1).any()
    # source pixels carrying ignore_label: never pasted by class, pasted with all-zero soft planes by box
    cond, _ = check(inp, C, classes=range(C))                      # all classes chosen
    assert np.array_equal(cond, inp['label_s'] != -1)
    check(inp, C, box=(0, h, 0, w))                                # the full box
    for box in ((0, 5, 3, 9), (11, h, 3, 9), (3, 9, 0, 5), (3, 9, 19, w), (0, 1, 0, 1), (h - 1, h, w - 1, w)):
        cond, _ = check(inp, C, box=box)
        assert cond.sum() == n * (box[1] - box[0]) * (box[3] - box[2])
    # another ignore label: -1 is then out of range
    inp255 = dict(inp, label_s=np.where(inp['label_s'] == -1, 255, inp['label_s']))
    assert check(inp255, C, ignore_label=255, classes=[0, 1])[1] == 0
    assert check(inp, C, ignore_label=255, classes=[0, 1])[1] == 1
    # an out-of-range label sets the flag; class mode pastes nothing there, box mode pastes it with all-zero soft planes
    bad = dict(inp, label_s=inp['label_s'].copy())
    bad['label_s'][0, 3, 4:7] = (C, 40, -5)
    bad['label_s'][1, 15, 23] = 1 << 40
    cond, flag = check(bad, C, classes=range(C))
    assert flag == 1 and not cond[0, 3, 4:7].any() and not cond[1, 15, 23]
    assert check(bad, C, box=(2, 5, 2, 9))[1] == 1
    assert check(bad, C, box=(8, 12, 2, 9))[1] == 0                # box mode reads the labels inside the box only
    # an empty class set and an empty box: bit-identical targets and no launch (a launch would raise the flag here)
    for pred in (dict(classes=[]), dict(box=(3, 3, 0, w)), dict(box=(0, h, 7, 7)), dict(box=(h, h, w, w))):
        cond, flag = check(bad, C, **pred)
        assert not cond.any() and flag == 0
    # each optional target present and absent
    for r in range(4):
        for use in itertools.combinations(('label_t', 'soft_t', 'regs_t'), r):
            check(inp, C, use=use, classes=[2, 3])
            check(inp, C, use=use, box=(1, 14, 2, 21))


def test_python_surface_errors_and_check():
    from regda_amd import ops
    rng = np.random.default_rng(6)
    inp = rand_inputs(rng, 1, 8, 8, 6)
    t = {k: dev(v) for k, v in inp.items()}
    a = (t['img_s'], t['label_s'], t['img_t'])
    for kw in (dict(), dict(classes=[0], box=(0, 1, 0, 1)), dict(classes=[6], class_num=6), dict(box=(0, 9, 0, 1)),
               dict(box=(3, 2, 0, 1)), dict(classes=[0], class_num=33), dict(classes=[0], class_num=6, soft_t=t['soft_t'][:, :5]),
               dict(classes=[0], label_t=t['label_t'].int()), dict(classes=[0], regs_t=t['regs_t'][:, :, :4]),
               dict(classes=[0], soft_t=t['soft_t'].transpose(2, 3))):
        with pytest.raises(ValueError):
            ops.domain_mix(*a, **kw)
    for bad in ((t['img_s'].half(), t['label_s'], t['img_t']), (t['img_s'], t['label_s'].int(), t['img_t']),
                (t['img_s'], t['label_s'], t['img_t'].double()), (t['img_s'][:, :, :4], t['label_s'], t['img_t'])):
        with pytest.raises(ValueError):
            ops.domain_mix(*bad, classes=[0])
    assert bits_equal(t['img_t'].cpu().numpy(), inp['img_t'])      # nothing above wrote
    t['label_s'][0, 0, 0] = 17
    with pytest.raises(ValueError, match='neither'):
        ops.domain_mix(*a, classes=[0], class_num=6, check=True)
    ops.domain_mix(*a, classes=[0], class_num=32, check=True)      # 17 is a class of a 32-class problem
    # (N,1,H,W) maps are accepted as they are
    ops.domain_mix(t['img_s'], t['label_s'][:, None], t['img_t'], label_t=t['label_t'][:, None], regs_t=t['regs_t'], box=(0, 4, 0, 4))
    torch.cuda.synchronize()
    assert int(t['regs_t'][0, 0, :4, :4].abs().sum()) == 0 and int(t['regs_t'][0, 0, 4:, 4:].min()) > 0


# ---------------------------------------------------------------------------------------------------- prefetcher
MEAN = (123.675, 116.28, 103.53)
STD = (58.395, 57.12, 57.375)
ROLES_S = dict(image='images_s', mask='label_s')
ROLES_T = dict(image='images_t', soft='soft_t', mask_sup='regs_t')


def _slot_ref(b, drawn, C):
    """mix_ref applied to the slot tensors of an unmixed prefetcher."""
    out = {k: v.cpu().numpy() for k, v in b.items()}
    if drawn is not None:
        img, _, soft, regs, flag, cond = mix_ref.domain_mix(out['images_s'], out['label_s'], out['images_t'], soft_t=out['soft_t'],
                                                            regs_t=out['regs_t'], C=C, **{drawn[0]: drawn[1]})
        assert flag == 0
        out.update(images_t=img, soft_t=soft, regs_t=regs)
    return out


def _compare_prefetchers(make, kind, steps=6):
    from regda_amd.aug.mix import DomainMix
    plain = make(None)
    mixed = make((DomainMix(kind, 6, prob=0.75, seed=9), ROLES_S, ROLES_T))
    twin = DomainMix(kind, 6, prob=0.75, seed=9)
    mixes = skips = 0
    for i in range(steps):
        b0, b1 = plain.next(), mixed.next()
        torch.cuda.synchronize()
        h, w = b0['images_t'].shape[2:]
        drawn = twin.draw(h, w)
        skips += drawn is None
        want = _slot_ref(b0, drawn, 6)
        for k, v in want.items():
            assert bits_equal(b1[k].cpu().numpy(), v), (kind, i, k, drawn)
        if drawn is not None and not bits_equal(want['images_t'], b0['images_t'].cpu().numpy()):
            mixes += 1
        plain.release()
        mixed.release()
    assert mixes > 0 and skips > 0 and int(mixed.mix_flag.item()) == 0       # prob = 0.75: some batches are left alone
    return mixes


@pytest.mark.parametrize('kind', ['class', 'box'])
def test_prefetcher_mix_without_augment(kind):
    from regda_amd.synthetic import make_batch
    from regda_amd.utils.prefetch import DevicePrefetcher
    host = [make_batch(b=2, size=64, seed=s, device='cpu') for s in (41, 42, 43)]
    _compare_prefetchers(lambda mix: DevicePrefetcher(host, depth=2, mix=mix), kind)


@pytest.mark.parametrize('kind', ['class', 'box'])
def test_prefetcher_mix_with_augment(kind):
    from regda_amd.aug import albu, augmentation as A
    from regda_amd.utils.prefetch import DevicePrefetcher
    g = torch.Generator().manual_seed(50)
    raw = []
    for i in range(3):
        raw.append(dict(images_s=torch.randint(0, 256, (2, 80, 80, 3), generator=g, dtype=torch.uint8),
                        label_s=torch.randint(0, 7, (2, 80, 80), generator=g, dtype=torch.uint8),    # 6 -> ignore
                        images_t=torch.randint(0, 256, (2, 80, 80, 3), generator=g, dtype=torch.uint8),
                        soft_t=torch.softmax(3 * torch.rand(2, 6, 80, 80, generator=g), 1),
                        regs_t=torch.randint(1, 40, (2, 80, 80), generator=g, dtype=torch.int32)))

    def make(mix, seed=11):
        ps = albu.Compose([albu.RandomCrop(64, 64), albu.OneOf([albu.HorizontalFlip(True), albu.VerticalFlip(True),
                                                                albu.RandomRotate90(True)], p=0.75),
                           albu.Normalize(MEAN, STD, max_pixel_value=1), albu.ToTensor()], rng=random.Random(seed))
        pt = A.Compose([A.RandomCrop((64, 64)), A.RandomHorizontalFlip(0.5), A.RandomVerticalFlip(0.5), A.RandomRotate90(0.5),
                        A.Normalize(MEAN, STD, clamp=True)], rng=random.Random(seed + 1),
                       generator=torch.Generator().manual_seed(seed + 2))
        return DevicePrefetcher(raw, depth=2, augment=[(ps, ROLES_S), (pt, ROLES_T)], mix=mix)
    _compare_prefetchers(make, kind)


def test_prefetcher_mix_refusals():
    from regda_amd.aug.mix import DomainMix
    from regda_amd.synthetic import make_batch
    from regda_amd.utils.prefetch import DevicePrefetcher
    host = [make_batch(b=2, size=64, seed=44, device='cpu')]
    dm = DomainMix('class', 6, seed=0)
    with pytest.raises(ValueError, match='supervision'):           # the online-teacher batch: no target labels to mix
        DevicePrefetcher(host, mix=(dm, ROLES_S, dict(image='images_t', mask_sup='regs_t')))
    small = dict(host[0], images_t=host[0]['images_t'][:, :, :32, :32].contiguous(),
                 soft_t=host[0]['soft_t'][:, :, :32, :32].contiguous(), regs_t=host[0]['regs_t'][:, :, :32, :32].contiguous())
    with pytest.raises(ValueError, match='pixel by pixel'):        # source and target slots of different shapes
        DevicePrefetcher([small], mix=(dm, ROLES_S, ROLES_T))
    with pytest.raises(ValueError, match='pixel by pixel'):        # soft planes of another class count
        DevicePrefetcher(host, mix=(DomainMix('class', 7, seed=0), ROLES_S, ROLES_T))
    with pytest.raises(ValueError):
        DevicePrefetcher(host, mix=(dm, dict(image='images_s'), ROLES_T))
    with pytest.raises(ValueError):
        DevicePrefetcher(host, mix=(dm, ROLES_S, dict(ROLES_T, soft='nope')))


# ---------------------------------------------------------------------------------------------------- step
def test_ssl_step_on_a_class_mixed_batch():
    """SSLStep(refine_label=False, sam_refine=True) on a class-mixed batch with offline soft labels: a pasted one-hot
    pixel survives pseudo_selection (1 > max(0.8 * 1, 0.6)) and sits in region 0, which LRH leaves alone, so the step's
    hard labels equal the source labels at every pasted pixel; the losses are finite; a second step from the same
    state on the same inputs is bit-identical."""
    from oracle import model as omodel
    from regda_amd import ops
    from regda_amd.models.Encoder import Deeplabv2
    from regda_amd.ssl import SSLStep
    from regda_amd.synthetic import make_batch
    rt = 'resnet17t'
    sd = omodel.init_state_dict(rt, 6, seed=3)
    b = make_batch(b=2, size=64, seed=7)
    present = sorted(set(b['label_s'].flatten().tolist()) - {-1})
    classes = present[: max(1, len(present) // 2)]
    src = {k: v.clone() for k, v in b.items()}
    runs = []
    for _ in range(2):
        m = Deeplabv2(dict(backbone=dict(resnet_type=rt, output_stride=16, pretrained=False), multi_layer=True,
                           cascade=False, use_ppm=True, ppm=dict(num_classes=6, use_aux=False, fc_dim=2048),
                           inchannels=2048, num_classes=6, is_ins_norm=True))
        m.load_state_dict(sd, strict=True)
        m.set_drop_masks(torch.ones(2, 512), torch.ones(2, 512))
        st = SSLStep(m, torch.randn(6, 2048, generator=torch.Generator().manual_seed(0)), refine_label=False, sam_refine=True)
        t = {k: v.clone() for k, v in src.items()}
        ops.domain_mix(t['images_s'], t['label_s'], t['images_t'], soft_t=t['soft_t'], regs_t=t['regs_t'], classes=classes, check=True)
        ls, lt, gn = st.step(t['images_s'], t['label_s'], t['images_t'], t['soft_t'], t['regs_t'], lr=1e-3)
        torch.cuda.synchronize()
        runs.append(dict(ls=ls.clone(), lt=lt.clone(), gn=gn.clone(), hard=st.last_hard.clone(), img=t['images_t'], soft=t['soft_t']))
    cond = torch.isin(src['label_s'], torch.tensor(classes, device='cuda'))
    assert cond.any() and not cond.all()
    r = runs[0]
    assert torch.equal(r['hard'][cond], src['label_s'][cond])
    assert not torch.equal(r['img'], src['images_t']) and torch.equal(torch.where(cond[:, None], src['soft_t'], r['soft']), src['soft_t'])
    assert all(bool(torch.isfinite(r[k]).all()) for k in ('ls', 'lt', 'gn')) and st.lrh_flag() == 0
    for k, v in r.items():
        assert bits_equal(v.cpu().numpy(), runs[1][k].cpu().numpy()), k
