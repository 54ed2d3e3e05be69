"""dev: the PyCDA region pyramid term (rgda_upsample_pycda) at 8 x 6 x 32 x 32 -> 512 x 512 with the default sizes
(8, 16, 32, 64, 0): HIP-event time per call with gradients accumulated, next to rgda_upsample_reg with both terms in the
same process (calls alternated, several rounds: the spread is printed) and the algorithmic bytes of both; then one SSL
step with the term on and off as bench.py builds it (ResNet-101, 8 + 8 images, recorded plan; --eager: eager steps), the
two steps alternated as well.
    python scripts/dev/pycda_bench.py [--no-step] [--eager] [--sizes 8,16,32,64,0]"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch

from regda_amd import ops


def t_of(fn, reps=50):
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3


def alternate(runs, rounds=5, reps=50):
    """{name: [us per call, one value per round]}, the runs taken in turn within every round."""
    for _, fn in runs:
        for _ in range(10):
            fn()
    times = {name: [] for name, _ in runs}
    for _ in range(rounds):
        for name, fn in runs:
            times[name].append(t_of(fn, reps))
    return times


def term_calls(sizes):
    g = torch.Generator().manual_seed(0)
    b, c, h, H = 8, 6, 32, 512
    p1, p2 = (torch.randn(b, c, h, h, generator=g) * 2).cuda(), (torch.randn(b, c, h, h, generator=g) * 2).cuda()
    lab = torch.randint(-1, c, (b, H, H), generator=g).cuda()
    # smooth, mostly confident soft labels: regions of every level are active
    coarse = torch.randn(b, c, 6, 6, generator=g) * 6
    soft = torch.nn.functional.interpolate(coarse, (H, H), mode='bilinear', align_corners=True)
    soft = torch.softmax(soft + 0.5 * torch.randn(b, c, H, H, generator=g), 1).cuda()
    g1, g2 = torch.zeros_like(p1), torch.zeros_like(p2)
    ws = ops.upsample_pycda_workspace(p1, soft.shape, sizes)
    loss = torch.zeros(1 + len(sizes), device='cuda')
    n_active = torch.zeros(len(sizes), dtype=torch.int32, device='cuda')
    runs = [('reg ent+kld', lambda: ops.upsample_reg(p1, p2, lab, lambda_ent=0.3, lambda_kld=0.1, g1=g1, g2=g2, accumulate=True,
                                                      empty_is_zero=True)),
            ('pycda', lambda: ops.upsample_pycda(p1, p2, soft, sizes, weight=0.1, g1=g1, g2=g2, accumulate=True, loss=loss,
                                                 n_active=n_active, ws=ws)),
            ('pycda no grad', lambda: ops.upsample_pycda(p1, p2, soft, sizes, want_grad=False, loss=loss, n_active=n_active,
                                                         ws=ws))]
    times = alternate(runs)
    npix = b * H * H
    low = 2 * 2 * b * c * h * h * 4                             # logits read, gradients written and read (accumulate), 2 heads
    s0 = min(sizes[0], 8)
    cells = b * (H // s0) ** 2
    row_t = 2 * b * H * 2 * c * h * 4                           # the row-contracted gradient, written and read
    nbytes = {'reg ent+kld': 2 * npix * 8 + low + row_t,        # the int64 label in the count and in the row pass
              'pycda no grad': c * npix * 4 + low // 2 + cells * 3 * c * 8,
              'pycda': c * npix * 4 + low + cells * 3 * c * 8 + npix // (s0 * s0) * 2 * c * 4 * 2 + row_t}
    print('n_active %s of %s regions, loss %s' % (n_active.tolist(), [b * (-(-H // s)) ** 2 if s else b for s in sizes],
                                                  [round(v, 4) for v in loss.tolist()]))
    base = sorted(times['reg ent+kld'])[len(times['reg ent+kld']) // 2]
    for name, _ in runs:
        ts = sorted(times[name])
        print('%-14s %7.1f us median of %d rounds (min %.1f, max %.1f)  %.2fx reg   %6.1f MB algorithmic' %
              (name, ts[len(ts) // 2], len(ts), ts[0], ts[-1], ts[len(ts) // 2] / base, nbytes[name] / 1e6), flush=True)


def step_times(sizes):
    from regda_amd.models.Encoder import Deeplabv2
    from regda_amd.ssl import SSLStep
    from regda_amd.synthetic import make_batch
    batch = make_batch(b=8, size=512, seed=2333, with_soft=True)
    protos = torch.randn(6, 2048, generator=torch.Generator().manual_seed(0))
    eager = '--eager' in sys.argv
    args = (batch['images_s'], batch['label_s'], batch['images_t'], batch['soft_t'], batch['regs_t'])
    steps = []
    for on in (False, True):
        torch.manual_seed(2333)
        model = Deeplabv2(dict(backbone=dict(resnet_type='resnet101', output_stride=16, pretrained=False),
                               multi_layer=True, cascade=False, use_ppm=True,
                               ppm=dict(num_classes=6, use_aux=False, fc_dim=2048), inchannels=2048, num_classes=6,
                               is_ins_norm=True))
        model.sync_weights()
        st = SSLStep(model, protos, **(dict(pycda_weight=0.1, pycda_sizes=sizes) if on else {}))
        for _ in range(2):
            st.step(*args, 1e-3)
        if not eager:
            st.record_plan(*args)
        steps.append(('pycda_weight=0.1' if on else 'pycda_weight=0', lambda st=st: st.step(*args, 1e-3)))
    times = alternate(steps, rounds=4, reps=10)
    for name, _ in steps:
        ts = sorted(t / 1e3 for t in times[name])
        print('SSLStep(%s): %.2f ms per step, median of %d rounds (min %.2f, max %.2f; %s)' %
              (name, ts[len(ts) // 2], len(ts), ts[0], ts[-1], 'eager' if eager else 'recorded plan'), flush=True)


if __name__ == '__main__':
    sizes = tuple(int(v) for v in sys.argv[sys.argv.index('--sizes') + 1].split(',')) if '--sizes' in sys.argv else (8, 16, 32, 64, 0)
    term_calls(sizes)
    if '--no-step' not in sys.argv:
        step_times(sizes)
