"""GPU: batched sliding-window inference (rgda_window_gather / _scatter / _finish, pre_slide(window_batch=K), evaluate,
gener_target_pseudo and predict_scene) against the per-window path, bit for bit."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

VIEWS = [(f, k) for f in (False, True) for k in (0, 1, 2, 3)]


@pytest.fixture(scope='module')
def ops():
    from regda_amd import ops
    return ops


class Stub:
    """A batch-invariant stand-in for the network: elementwise torch ops only, so every output pixel depends on its own
    sample (and input pixel) alone and is the same at any batch size."""
    def __init__(self, num_classes=6, seed=0):
        g = torch.Generator().manual_seed(seed)
        self.num_classes = num_classes
        self.idx = torch.arange(num_classes) % 3
        self.w = (torch.randn(num_classes, generator=g) * 2).cuda().view(1, -1, 1, 1)
        self.b = torch.randn(num_classes, generator=g).cuda().view(1, -1, 1, 1)
        self.calls = []

    def eval(self):
        return self

    def __call__(self, x):
        self.calls.append(tuple(x.shape))
        return torch.sigmoid(x[:, self.idx] * self.w + self.b)


def table(rows):
    return torch.tensor(rows, dtype=torch.int32).cuda()


def windows_of(n, H, W, tile):
    from regda_amd.utils.tools import window_list
    return [(i, y1, x1) for i in range(n) for (y1, x1, _, _) in window_list(H, W, tile)]


# --------------------------------------------------------------------------------------------------------- kernels
@pytest.mark.parametrize('views', [1, 8])
def test_gather_equals_crop_then_view(ops, views):
    g = torch.Generator().manual_seed(1)
    n, c, H, W, T = 2, 3, 70, 53, 32
    img = torch.randn(n, c, H, W, generator=g).cuda()
    rows = windows_of(n, H, W, (T, T))
    for K in (1, 3, len(rows)):
        wins = table(rows[:K])
        out = ops.window_gather(img, wins, (T, T), views)
        assert tuple(out.shape) == (K * views, c, T, T)
        for w, (i, y1, x1) in enumerate(rows[:K]):
            tile = ops.window_crop(img[i:i + 1].contiguous(), y1, x1, T, T, T, T)
            for v in range(views):
                f, k = VIEWS[v]
                ref = ops.dihedral(tile, f, k, True) if views == 8 else tile
                assert torch.equal(out[w * views + v:w * views + v + 1], ref), (K, w, v)


def test_gather_uint8_equals_eval_normalise_then_crop(ops):
    from regda_amd import aug
    from configs import ToPotsdam
    pipe = aug.from_config(ToPotsdam.EVAL_DATA_CONFIG)
    lut = pipe.table().cuda()
    rng = np.random.default_rng(2)
    n, H, W, T = 2, 45, 61, 24
    raw = torch.from_numpy(rng.integers(0, 256, (n, H, W, 3), dtype=np.uint8)).cuda()
    norm = torch.stack([pipe(raw[i].clone())['image'] for i in range(n)])     # (the launch wants a 4-byte aligned image)
    rows = windows_of(n, H, W, (T, T))
    for views in (1, 8):
        out = ops.window_gather(raw, table(rows), (T, T), views, lut=lut)
        ref = ops.window_gather(norm.contiguous(), table(rows), (T, T), views)
        assert torch.equal(out, ref), views
        i, y1, x1 = rows[-1]
        assert torch.equal(out[(len(rows) - 1) * views], norm[i, :, y1:y1 + T, x1:x1 + T])


def sequential(ops, pred, rows, views, full, count, T):
    """The per-window path: tta_predict's de-augmented mean (views = 8), then window_accumulate, window by window."""
    for w, (i, y1, x1) in enumerate(rows):
        if views == 1:
            t = pred[w:w + 1].contiguous()
        else:
            t = None
            for v, (f, k) in enumerate(VIEWS):
                t = ops.dihedral(pred[w * 8 + v:w * 8 + v + 1].contiguous(), f, (4 - k) % 4, False, dst=t, scale=1.0 / 8,
                                 accumulate=t is not None)
        fi, ci = full[i:i + 1].contiguous(), count[i:i + 1].contiguous()
        ops.window_accumulate(t, fi, ci, y1, x1, T, T)
        full[i:i + 1], count[i:i + 1] = fi, ci


@pytest.mark.parametrize('views', [1, 8])
def test_scatter_equals_sequential_accumulate(ops, views):
    g = torch.Generator().manual_seed(3)
    n, C, H, W, T = 2, 7, 75, 50, 32
    rows = windows_of(n, H, W, (T, T))
    pred = torch.softmax(torch.randn(len(rows) * views, C, T, T, generator=g) * 3, 1).cuda()
    full_ref, count_ref = torch.zeros(n, C, H, W, device='cuda'), torch.zeros(n, 1, H, W, device='cuda')
    sequential(ops, pred, rows, views, full_ref, count_ref, T)
    for K in (1, 2, 5, len(rows), len(rows) + 3):
        full, count = torch.zeros_like(full_ref), torch.zeros_like(count_ref)
        for s in range(0, len(rows), K):
            chunk = rows[s:s + K]
            r0 = min(i * H + y for i, y, _ in chunk)
            r1 = max(i * H + y + T for i, y, _ in chunk)
            ops.window_scatter(pred[s * views:(s + len(chunk)) * views], table(chunk), full, count, (r0, r1 - r0), views)
        assert torch.equal(full, full_ref) and torch.equal(count, count_ref), K


def test_scatter_flags_a_bad_row_and_skips_it(ops):
    full, count = torch.zeros(1, 6, 40, 40, device='cuda'), torch.zeros(1, 1, 40, 40, device='cuda')
    flag = torch.zeros(1, dtype=torch.int32, device='cuda')
    pred = torch.ones(2, 6, 32, 32, device='cuda')
    ops.window_scatter(pred, table([(0, 0, 0), (0, 9, 0)]), full, count, (0, 40), 1, flag=flag)
    assert int(flag) == 1 and float(count.max()) == 1 and float(count.sum()) == 32 * 32
    out = ops.window_gather(torch.ones(1, 3, 40, 40, device='cuda'), table([(1, 0, 0)]), (32, 32), flag=flag)
    assert float(out.abs().sum()) == 0


def test_finish_equals_normalise_argmax_confusion(ops):
    g = torch.Generator().manual_seed(4)
    n, C, H, W = 2, 9, 37, 41
    full = torch.rand(n, C, H, W, generator=g).cuda() * 3
    full[0, :, 3, 3] = 1.5                                       # a tie: the first maximum wins
    count = torch.randint(1, 5, (n, 1, H, W), generator=g).float().cuda()
    count[1, 0, 7, 7] = 0                                        # no window: NaN probabilities, label 0
    y_true = torch.randint(-1, C, (n, H, W), generator=g).cuda()
    ref = full.clone()
    ops.window_normalise(ref, count)
    lab_ref = ops.argmax_nchw(ref)
    cm_ref = torch.zeros(C, C, dtype=torch.int64, device='cuda')
    flag_ref = torch.zeros(1, dtype=torch.int32, device='cuda')
    ops.confusion_accumulate(y_true, lab_ref, cm_ref, flag_ref)
    got = full.clone()
    cm = torch.zeros(C, C, dtype=torch.int64, device='cuda')
    flag = torch.zeros(1, dtype=torch.int32, device='cuda')
    u8 = torch.empty(n, H, W, dtype=torch.uint8, device='cuda')
    ops.window_finish(got, count, labels=u8, y_true=y_true, cm=cm, flag=flag)
    assert torch.equal(got.view(torch.int32), ref.view(torch.int32))       # bits, NaN included
    assert torch.equal(u8.long(), lab_ref) and torch.equal(cm, cm_ref) and int(flag) == 0
    i64 = torch.empty(n, H, W, dtype=torch.int64, device='cuda')
    ops.window_finish(full.clone(), count, labels=i64)
    assert torch.equal(i64, lab_ref)
    ops.window_finish(full.clone(), count, y_true=torch.full_like(y_true, C), cm=cm, flag=flag)
    assert int(flag) == 1 and torch.equal(cm, cm_ref)            # a label >= C: flagged, not counted


# --------------------------------------------------------------------------------------------------------- pre_slide
@pytest.mark.parametrize('shape', [(1, 512, 512), (1, 1024, 1024), (2, 1100, 700), (1, 300, 400), (1, 40, 24)])
@pytest.mark.parametrize('tta', [False, True])
def test_pre_slide_batched_equals_per_window(shape, tta):
    from regda_amd.utils.tools import pre_slide
    n, H, W = shape
    if tta and n > 1:
        n = 1                                                    # tta_predict (the per-window path) takes one image
    img = torch.randn(n, 3, H, W, generator=torch.Generator().manual_seed(H + W)).cuda()
    m = Stub(6)
    ref = pre_slide(m, img, num_classes=6, tta=tta)
    for K in (1, 3, 16):
        m.calls.clear()
        got = pre_slide(m, img, num_classes=6, tta=tta, window_batch=K)
        assert torch.equal(got.view(torch.int32), ref.view(torch.int32)), (shape, tta, K)
        if H >= 512 and W >= 512:
            assert max(c[0] for c in m.calls) <= K * (8 if tta else 1)


def test_tta_goldens_through_the_batched_path(gold):
    from regda_amd.utils.tools import pre_slide
    from test_teacher_gpu import fake_model
    g = gold('tta.npz')
    model = fake_model(g)
    for i in range(3):
        img, tile = torch.from_numpy(g[f'img{i}']).cuda(), tuple(int(v) for v in g[f'tile{i}'])
        for tta in (0, 1):
            got = pre_slide(model, img, num_classes=5, tile_size=tile, tta=bool(tta), window_batch=4)
            np.testing.assert_allclose(got.cpu().numpy(), g[f'probs{i}_tta{tta}'], rtol=0, atol=2e-6)


# --------------------------------------------------------------------------------------------------------- scenes
def test_predict_scene_equals_host_normalised_pre_slide():
    from configs import ToPotsdam
    from regda_amd import ops
    from regda_amd.utils.infer import predict_scene, scene_table
    from regda_amd.utils.tools import pre_slide
    rng = np.random.default_rng(5)
    scene = rng.integers(0, 256, (2000, 1500, 3), dtype=np.uint8)
    lut = scene_table(ToPotsdam)
    x = lut[torch.arange(3).view(3, 1, 1), torch.from_numpy(scene).permute(2, 0, 1).long()][None]     # on the host
    m = Stub(6, seed=1)
    for tta in (False, True):
        probs = pre_slide(m, x.cuda(), num_classes=6, tta=tta)
        want = ops.argmax_nchw(probs)[0].to(torch.uint8)
        lab, got = predict_scene(m, scene, ToPotsdam, 6, tta=tta, window_batch=8, return_probs=True)
        assert lab.dtype == torch.uint8 and tuple(lab.shape) == (2000, 1500)
        assert torch.equal(lab, want) and torch.equal(got, probs), tta
        assert max(c[0] for c in m.calls[-4:]) <= 8 * (8 if tta else 1)
    small = scene[:300, :200]
    assert torch.equal(predict_scene(m, torch.from_numpy(small).cuda(), ToPotsdam, 6),
                       ops.argmax_nchw(pre_slide(m, x[:, :, :300, :200].contiguous().cuda(), num_classes=6))[0].to(torch.uint8))


# --------------------------------------------------------------------------------------------------------- the network
def build(rt, ncls, seed):
    from regda_amd.models.Encoder import Deeplabv2
    torch.manual_seed(seed)
    m = Deeplabv2(dict(backbone=dict(resnet_type=rt, output_stride=16, pretrained=False), multi_layer=True,
                       cascade=False, use_ppm=True, ppm=dict(num_classes=ncls, use_aux=False, fc_dim=2048),
                       inchannels=2048, num_classes=ncls, is_ins_norm=True))
    with torch.no_grad():                       # confident random classifiers (bench.py does the same)
        for head in ('layer5', 'layer6'):
            m.convs[f'{head}.conv_last.4'].w.mul_(40.0)
    m.sync_weights()
    m.eval()
    return m


@pytest.fixture(scope='module', params=[('resnet50', 7), ('resnet101', 6)], ids=['r50c7', 'r101c6'])
def net(request):
    rt, ncls = request.param
    return build(rt, ncls, seed=11), ncls


def same_batches_reference(m, img, ncls, tile, tta, K):
    """pre_slide(window_batch=K) spelled out with the per-window kernels: the same K-window forward batches (crops +
    dihedral views stacked in table order), then tta_predict's de-augmented mean and window_accumulate window by window.
    The network sees exactly the batches the batched route gives it, so the two must agree bit for bit."""
    from regda_amd import ops
    n, _, H, W = img.shape
    rows = windows_of(n, H, W, tile)
    views = 8 if tta else 1
    full, count = torch.zeros(n, ncls, H, W, device='cuda'), torch.zeros(n, 1, H, W, device='cuda')
    for s in range(0, len(rows), K):
        chunk = rows[s:s + K]
        parts = []
        for i, y1, x1 in chunk:
            t = ops.window_crop(img[i:i + 1].contiguous(), y1, x1, tile[0], tile[1], tile[0], tile[1])
            parts += [ops.dihedral(t, f, k, True) for f, k in VIEWS] if tta else [t]
        pred = m(torch.cat(parts))
        sequential(ops, pred, chunk, views, full, count, tile[0])
    ops.window_normalise(full, count)
    return full


def test_deeplab_pre_slide_batched_equals_same_batches(net):
    """The real network through the batched route: bit for bit the per-window kernels over the same forward batches.
    Against the batch-1 per-window path the network itself is not batch invariant (the eval forward
    of a sample changes with the batch it sits in); that difference is reported, and bounded loosely here."""
    from regda_amd.utils.tools import pre_slide
    m, ncls = net
    g = torch.Generator().manual_seed(6)
    for H, W, tta in ((512, 512, True), (1024, 768, False)):
        img = torch.randn(1, 3, H, W, generator=g).cuda()
        got = pre_slide(m, img, num_classes=ncls, tta=tta, window_batch=4)
        assert torch.equal(got, same_batches_reference(m, img, ncls, (512, 512), tta, 4)), (H, W, tta)
        ref = pre_slide(m, img, num_classes=ncls, tta=tta)
        assert torch.isfinite(got).all() and torch.allclose(got.sum(1), torch.ones_like(got.sum(1)), atol=1e-4)
        assert (got.argmax(1) != ref.argmax(1)).float().mean().item() < 0.25


def test_deeplab_evaluate_batched_equals_its_groups(net):
    """evaluate(window_batch=K): the table and mIoU of the confusion matrix that argmax + rgda_confusion_accumulate
    build from pre_slide(window_batch=K) over the same groups of items."""
    from regda_amd import ops
    from regda_amd.gast.metrics import PixelMetricIgnore
    from regda_amd.utils.eval import evaluate
    from regda_amd.utils.tools import pre_slide, window_groups
    m, ncls = net
    g = torch.Generator().manual_seed(7)
    loader = [(torch.randn(1, 3, 512, 512, generator=g), {'cls': torch.randint(-1, ncls, (1, 512, 512), generator=g)})
              for _ in range(5)]
    loader += [(torch.randn(1, 3, 700, 600, generator=g), {'cls': torch.randint(-1, ncls, (1, 700, 600), generator=g)})
               for _ in range(2)]
    loader += [(torch.randn(1, 3, 300, 200, generator=g), {'cls': torch.randint(-1, ncls, (1, 300, 200), generator=g)})]

    class Cfg:
        DATASETS = 'IsprsDA'
        NUM_CLASSES = ncls
        SNAPSHOT_DIR = None
    for K in (2, 4):
        metric = PixelMetricIgnore(ncls, class_names=[str(i) for i in range(ncls)], ignore_labels=[0])
        for grp in window_groups(loader, window_batch=K):
            cls = pre_slide(m, torch.cat([x for x, _ in grp]).cuda(), num_classes=ncls, window_batch=K)
            metric.forward(torch.cat([y['cls'] for _, y in grp]), ops.argmax_nchw(cls))
        assert evaluate(m, Cfg, is_training=True, dataloader=loader, tta=False, window_batch=K) == metric.summary_all(), K


def test_deeplab_pseudo_labels_batched_are_written_per_tile(net, tmp_path):
    """gener_target_pseudo(window_batch=K): per tile, in loader order, the files the per-tile writer makes of the group's
    pre_slide(tta=True, window_batch=K) probabilities (.pt soft labels bit for bit; hard-label images)."""
    from PIL import Image
    from oracle import labels as olab
    from regda_amd.gast.pseudo_generation import gener_target_pseudo
    from regda_amd.utils.tools import pre_slide
    m, ncls = net
    g = torch.Generator().manual_seed(8)
    loader = [(torch.randn(1, 3, 512, 512, generator=g), {'fname': [f't{i}.png']}) for i in range(3)]
    probs = torch.cat([pre_slide(m, torch.cat([x for x, _ in loader[s:s + 2]]).cuda(), num_classes=ncls, tta=True,
                                 window_batch=2) for s in (0, 2)])

    class Cfg:
        NUM_CLASSES = ncls
        PSEUDO_SELECT = True
    for save_prob in (True, False):
        out = str(tmp_path / f'bat{save_prob}')
        gener_target_pseudo(Cfg, m, loader, out, save_prob=save_prob, size=(512, 512), window_batch=2)
        for i in range(3):
            if save_prob:
                t = torch.load(os.path.join(out, f't{i}.png.pt'))
                assert t.dtype == torch.float32 and torch.equal(t, probs[i].cpu()), i
            else:
                want = olab.pseudo_selection(probs[i:i + 1].cpu().numpy(), 0.8, 0.6, -1) + 1
                assert np.array_equal(np.array(Image.open(os.path.join(out, f't{i}.png'))), want[0].astype(np.uint8)), i
