"""dev: the training augmentation of raw tiles (rgda_augment_tiles) for one 8 + 8 batch of 512 x 512
crops: HIP-event time per batch (source: image + label; target: image + region map, and + soft labels offline),
algorithmic bytes and their share of the 8 TB/s peak, bytes staged raw against prepared, the torch CPU restatement's
time per target tile, and the step time of a recorded SSLStep fed by DevicePrefetcher(augment=...) against resident
inputs, alternated.  --affine: rgda_augment_affine against rgda_augment_tiles on the same inputs,
alternated, at 512 -> 512 and 1024 -> 512: dihedral rows (the same work as rgda_augment_tiles) and drawn scale /
rotation rows.
    python scripts/dev/aug_bench.py [--no-step] [--size 512] [--input 512]
    python scripts/dev/aug_bench.py --affine"""
import argparse
import os
import random
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch

from regda_amd import ops
from regda_amd.aug import albu, augmentation as A

MEAN = (123.675, 116.28, 103.53)
STD = (58.395, 57.12, 57.375)
PEAK = 8e12


def t_of(fn, reps=200):
    for _ in range(10):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3


def pipes(size):
    s = albu.Compose([albu.RandomCrop(size, size), albu.OneOf([albu.HorizontalFlip(True), albu.VerticalFlip(True),
                                                               albu.RandomRotate90(True)], p=0.75),
                      albu.Normalize(MEAN, STD, max_pixel_value=1)], rng=random.Random(0))
    t = A.Compose([A.RandomCrop((size, size)), A.RandomHorizontalFlip(0.5), A.RandomVerticalFlip(0.5),
                   A.RandomRotate90(0.5), A.Normalize(MEAN, STD, clamp=True)], rng=random.Random(1))
    return s, t


def raw_batch(b, hw, c=6, seed=0):
    g = torch.Generator().manual_seed(seed)
    return dict(images_s=torch.randint(0, 256, (b, hw, hw, 3), generator=g, dtype=torch.uint8),
                label_s=torch.randint(0, 6, (b, hw, hw), generator=g, dtype=torch.uint8),
                images_t=torch.randint(0, 256, (b, hw, hw, 3), generator=g, dtype=torch.uint8),
                soft_t=torch.softmax(3 * torch.randn(b, c, hw, hw, generator=g), 1),
                regs_t=torch.randint(0, 200, (b, hw, hw), generator=g, dtype=torch.int32))


def kernel(b, size, hw):
    ps, pt = pipes(size)
    raw = {k: v.cuda() for k, v in raw_batch(b, hw).items()}
    prm_s, prm_t = ps.params(b, hw, hw).cuda(), pt.params(b, hw, hw).cuda()
    (ls, lls), (lt, llt) = ps.device_tables('cuda'), pt.device_tables('cuda')
    c = raw['soft_t'].shape[1]
    for offline in (False, True):
        soft = raw['soft_t'] if offline else None

        def run():
            ops.augment_tiles(raw['images_s'], prm_s, ls, (size, size), label=raw['label_s'], label_lut=lls)
            ops.augment_tiles(raw['images_t'], prm_t, lt, (size, size), soft=soft, regs=raw['regs_t'])
        t = t_of(run)
        px_in, px_out = b * hw * hw, b * size * size
        # source: uint8 image + label read once in the crop, f32 image + int64 label written; target: uint8 image +
        # int32 regions (+ f32 soft) read, f32 image + int64 regions (+ f32 soft) written
        rd = px_out * (3 + 1) + px_out * (3 + 4 + (4 * c if offline else 0))
        wr = px_out * (12 + 8) + px_out * (12 + 8 + (4 * c if offline else 0))
        nb = rd + wr
        staged_raw = px_in * (3 + 1) + px_in * (3 + 4 + (4 * c if offline else 0))
        staged_prep = px_out * (12 + 8) + px_out * (12 + 8 + (4 * c if offline else 0))
        print('%-8s %d + %d x %d^2 -> %d: %6.1f us per batch (2 launches)  %6.1f MB algorithmic, floor %5.1f us at 8 TB/s'
              ' (%4.1f %% of peak, %.2f TB/s)  staged raw %.1f MB vs prepared %.1f MB' % (
                  'offline' if offline else 'online', b, b, hw, size, t, nb / 1e6, nb / PEAK * 1e6,
                  100 * nb / PEAK * 1e6 / t, nb / t / 1e6, staged_raw / 1e6, staged_prep / 1e6), flush=True)


def affine(b, size, hw, rounds=5):
    """One 8 + 8 batch (source: image + label; target: image + soft labels + region map), three tables over the same
    crops: rgda_augment_tiles' (y0, x0, d), the same rows through rgda_augment_affine, and RandomScaleRotate's draws
    (scale 0.5 - 2, +-30 degrees, every coin fires).  The launches alternate inside every round; the median round
    counts.  Bytes: each output pixel once (the dihedral kernel's count), so the warped rows' taps come on top."""
    ps, pt = pipes(size)
    raw = {k: v.cuda() for k, v in raw_batch(b, hw).items()}
    (ls, lls), (lt, llt) = ps.device_tables('cuda'), pt.device_tables('cuda')
    tile_s, tile_t = ps.params(b, hw, hw), pt.params(b, hw, hw)
    rows = lambda t, m=None: torch.tensor([A.affine_row(y0, x0, A.matrix(d) if m is None else m(), (0, 0), size, size,
                                                         hw, hw) for y0, x0, d, _ in t.tolist()], dtype=torch.int32).cuda()
    rng = random.Random(2)
    warp = lambda: A.rotation(rng.uniform(0.5, 2.0), rng.uniform(-30, 30))
    tabs = {'tiles': (tile_s.cuda(), tile_t.cuda()), 'affine, dihedral rows': (rows(tile_s), rows(tile_t)),
            'affine, scale 0.5-2 +-30 deg': (rows(tile_s, warp), rows(tile_t, warp))}
    c = raw['soft_t'].shape[1]

    def run(name):
        prm_s, prm_t = tabs[name]
        if name == 'tiles':
            ops.augment_tiles(raw['images_s'], prm_s, ls, (size, size), label=raw['label_s'], label_lut=lls)
            ops.augment_tiles(raw['images_t'], prm_t, lt, (size, size), soft=raw['soft_t'], regs=raw['regs_t'])
        else:
            ops.augment_affine(raw['images_s'], prm_s, ls, (size, size), label=raw['label_s'], label_lut=lls)
            ops.augment_affine(raw['images_t'], prm_t, lt, (size, size), soft=raw['soft_t'], regs=raw['regs_t'])
    times = {k: [] for k in tabs}
    for _ in range(rounds):
        for name in tabs:
            times[name].append(t_of(lambda: run(name), reps=100))
    px = b * size * size
    nb = px * (3 + 1 + 12 + 8) + px * (3 + 4 + 4 * c + 12 + 8 + 4 * c)
    for name, v in times.items():
        v = sorted(v)
        med = v[len(v) // 2]
        print('%d + %d x %d^2 -> %d  %-30s %6.1f us per batch (min %.1f, max %.1f; 2 launches)  %.1f MB, floor %.1f us at '
              '8 TB/s: %4.1f %% of peak' % (b, b, hw, size, name, med, v[0], v[-1], nb / 1e6, nb / PEAK * 1e6,
                                            100 * nb / PEAK * 1e6 / med), flush=True)


def cpu_restatement(size, threads=16):
    """The torch CPU restatement of the target transform per tile (float conversion, crop, flips, rot90, normalise +
    clamp of the image, the soft label and region map, the collate copy)."""
    torch.set_num_threads(threads)
    g = torch.Generator().manual_seed(0)
    img = torch.randint(0, 256, (size, size, 3), generator=g, dtype=torch.uint8)
    soft = torch.rand(6, size, size, generator=g)
    regs = torch.randint(0, 200, (size, size), generator=g, dtype=torch.int64)[None]
    mean, std = torch.tensor(MEAN).view(3, 1, 1), torch.tensor(STD).view(3, 1, 1)
    out = [torch.empty(8, 3, size, size), torch.empty(8, 6, size, size), torch.empty(8, 1, size, size, dtype=torch.int64)]

    def one(i):
        x = img.float().permute(2, 0, 1)
        m, r = soft, regs
        x, m, r = x.flip(-1), m.flip(-1), r.flip(-1)
        x, m, r = x.flip(-2), m.flip(-2), r.flip(-2)
        x, m, r = (torch.rot90(t, 1, [1, 2]) for t in (x, m, r))
        x = ((x - mean) / std).clamp(max=1.0)
        out[0][i].copy_(x)
        out[1][i].copy_(m)
        out[2][i].copy_(r)
    for i in range(2):
        one(i)
    t0 = time.perf_counter()
    reps = 16
    for i in range(reps):
        one(i % 8)
    dt = (time.perf_counter() - t0) / reps * 1e3
    print('torch CPU restatement of the target transform: %.2f ms per tile at %d threads' % (dt, threads), flush=True)


def step_times(b, size, hw, rounds=3, steps=20):
    from regda_amd.models.Encoder import Deeplabv2
    from regda_amd.ssl import SSLStep
    from regda_amd.synthetic import make_batch
    from regda_amd.utils.prefetch import DevicePrefetcher
    batch = make_batch(b=b, size=size, seed=2333, with_soft=True)
    protos = torch.randn(6, 2048, generator=torch.Generator().manual_seed(0))
    torch.manual_seed(2333)
    model = Deeplabv2(dict(backbone=dict(resnet_type='resnet101', output_stride=16, pretrained=False), multi_layer=True,
                           cascade=False, use_ppm=True, ppm=dict(num_classes=6, use_aux=False, fc_dim=2048),
                           inchannels=2048, num_classes=6, is_ins_norm=True))
    model.sync_weights()
    st = SSLStep(model, protos)
    args = (batch['images_s'], batch['label_s'], batch['images_t'], batch['soft_t'], batch['regs_t'])
    for _ in range(2):
        st.step(*args, 1e-3)
    st.record_plan(*args)
    ps, pt = pipes(size)
    raw = [raw_batch(b, hw, seed=s) for s in (1, 2)]
    pf = DevicePrefetcher(raw, into=st.static_inputs(),
                          augment=[(ps, dict(image='images_s', mask='label_s')),
                                   (pt, dict(image='images_t', soft='soft_t', mask_sup='regs_t'))])
    s_in = st.static_inputs()
    names = ('images_s', 'label_s', 'images_t', 'soft_t', 'regs_t')

    def resident():
        st.step(*args, 1e-3)

    def prefetched():
        x = pf.next()
        st.step(*(x[k] for k in names), 1e-3)
        pf.release(st.inputs_consumed())
    assert s_in['images_s'] is pf.slots[0]['images_s']
    res = {'resident': [], 'prefetch+augment': []}
    for _ in range(rounds):
        for name, fn in (('resident', resident), ('prefetch+augment', prefetched)):
            # the resident step copies its inputs into the same static buffers the prefetcher writes: no overlap
            torch.cuda.current_stream().wait_stream(pf.copy_stream)
            for _ in range(3):
                fn()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                fn()
            torch.cuda.synchronize()
            res[name].append((time.perf_counter() - t0) / steps * 1e3)
    for name, v in res.items():
        print('SSLStep (recorded plan), %-17s: %s ms per step' % (name, ' '.join('%.2f' % x for x in v)), flush=True)
    print('raw bytes staged per batch: %.1f MB' % (pf.bytes_per_batch / 1e6), flush=True)


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--size', type=int, default=512)
    ap.add_argument('--input', type=int, default=512)
    ap.add_argument('--batch', type=int, default=8)
    ap.add_argument('--no-step', action='store_true')
    ap.add_argument('--no-cpu', action='store_true')
    ap.add_argument('--kernel-only', action='store_true')
    ap.add_argument('--affine', action='store_true')
    a = ap.parse_args()
    if a.affine:
        for hw in (512, 1024):
            affine(a.batch, 512, hw)
        sys.exit(0)
    kernel(a.batch, a.size, a.input)
    if a.kernel_only:
        sys.exit(0)
    if not a.no_cpu:
        cpu_restatement(a.size)
    if not a.no_step:
        step_times(a.batch, a.size, a.input)
