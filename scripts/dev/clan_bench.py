"""The category-level adversarial term at the training shape: 8 + 8 tiles of 512 x 512, C = 6, logits 32 x 32.
  kernels: the three entry points of csrc/clan_kernels.hip (rgda_clan_probs_fwd, rgda_wbce_logits with dz and gw,
           rgda_clan_probs_bwd with gw), one warm-up and then `calls` calls each -- HIP-event medians are printed; run it
           under `rocprofv3 --kernel-trace --stats -- python scripts/dev/clan_bench.py kernels` for the per-kernel times;
  step:    AlignStep (resnet101, as bench.py builds the model) with the adversarial term off, with adv_kind='adaptsegnet'
           (two discriminators) and with adv_kind='clan' (one), every arm warmed up in ONE process and then timed in
           alternating rounds of `steps` steps each; the per-round times, the median and the spread are printed.
    python scripts/dev/clan_bench.py kernels [calls]
    python scripts/dev/clan_bench.py step [steps] [rounds]"""
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from regda_amd import ops  # noqa: E402
from regda_amd.synthetic import make_batch  # noqa: E402

N, S, C = 8, 512, 6


def median_us(fn, calls):
    fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(calls):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1) * 1e3)
    return statistics.median(times), min(times), max(times)


def kernels(calls):
    g = torch.Generator(device='cuda').manual_seed(0)
    x1 = torch.randn(N, C, S // 16, S // 16, device='cuda', generator=g) * 2
    x2 = x1 * 0.5 + torch.randn(N, C, S // 16, S // 16, device='cuda', generator=g)
    z = torch.randn(N, S // 32, S // 32, device='cuda', generator=g)
    P, wmap = ops.clan_probs(x1, x2, (S, S))
    dP = torch.randn(N * S * S, ops.ADV_CP, device='cuda', generator=g).to(torch.bfloat16)
    _, _, gw = ops.wbce_logits(z, (S, S), 0, wmap, 0.4, 40.0, want_gw=True)
    dx1, dx2 = torch.zeros_like(x1), torch.zeros_like(x2)
    px = N * S * S
    rows = (('rgda_clan_probs_fwd', lambda: ops.clan_probs(x1, x2, (S, S)), px * (32 + 4)),
            ('rgda_wbce_logits (dz, gw; 3 launches)', lambda: ops.wbce_logits(z, (S, S), 0, wmap, 0.4, 40.0, want_gw=True),
             px * (4 + 4) + px * 4),
            ('rgda_clan_probs_bwd (gw)', lambda: ops.clan_probs_backward(dP, gw, x1, x2, dx1, dx2, (S, S)), px * (32 + 4)))
    for name, fn, by in rows:
        t = median_us(fn, calls)
        print('%-40s median of %d calls %.1f us (min %.1f, max %.1f); %.1f MB -> %.0f GB/s' % (name, calls, *t, by / 1e6,
                                                                                              by / t[0] / 1e3))


def step(n_steps, rounds):
    from regda_amd.align import AlignStep
    from regda_amd.models.Encoder import Deeplabv2
    b = make_batch(b=N, size=S, classes=C, seed=2333, with_soft=False)
    args = (b['images_s'], b['label_s'], b['images_t'], b['regs_t'])
    arms = {}
    for name, kw in (('term off', {}), ("adv_kind='adaptsegnet'", dict(adv_weight=1e-3)),
                     ("adv_kind='clan'", dict(adv_weight=1e-3, adv_kind='clan'))):
        torch.manual_seed(2333)
        model = Deeplabv2(dict(backbone=dict(resnet_type='resnet101', output_stride=16, pretrained=False), multi_layer=True,
                               cascade=False, use_ppm=True, ppm=dict(num_classes=C, use_aux=False, fc_dim=2048),
                               inchannels=2048, num_classes=C, is_ins_norm=True))
        arms[name] = AlignStep(model, torch.randn(C, 2048, generator=torch.Generator().manual_seed(0)), **kw)
        for _ in range(3):
            arms[name].step(*args, 1e-4)
        torch.cuda.synchronize()
    times = {k: [] for k in arms}
    for _ in range(rounds):
        for name, st in arms.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(n_steps):
                st.step(*args, 1e-4)
            e1.record()
            torch.cuda.synchronize()
            times[name].append(e0.elapsed_time(e1) / n_steps)
    for k, v in times.items():
        print('step %-24s ms/step per round of %d steps: %s; median %.3f (min %.3f, max %.3f)' % (
            k, n_steps, ' '.join('%.3f' % x for x in v), statistics.median(v), min(v), max(v)))


if __name__ == '__main__':
    mode = sys.argv[1] if len(sys.argv) > 1 else 'kernels'
    if mode == 'kernels':
        kernels(int(sys.argv[2]) if len(sys.argv) > 2 else 20)
    else:
        step(int(sys.argv[2]) if len(sys.argv) > 2 else 10, int(sys.argv[3]) if len(sys.argv) > 3 else 5)
