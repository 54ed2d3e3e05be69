"""The strong augmentation of the student's tile (SSLStep(strong=...)) at the training shape: 8 tiles of
3 x 512 x 512.
  (1) HIP-event times of rgda_strong_augment (3 launches) with every switch on at sigma = 1.15, with one switch, with none
      (the kernel's own copy route), of a plain device copy of the same bytes, and of rgda_strong_write_table: one
      warm-up, then the median of `calls`;
  (2) the whole step (resnet101, online teacher, recorded plan, as bench.py runs it) with mix='dacs' alone and with
      mix='dacs' + strong= (every image jittered and blurred), every arm warmed up and recorded in ONE process and then
      timed in alternating rounds of `steps` steps each; each arm's plan size is printed next to it.
    python scripts/dev/strong_bench.py [calls] [steps] [rounds] [out.txt]"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from regda_amd import ops  # noqa: E402
from regda_amd.aug.mix import DomainMix  # noqa: E402
from regda_amd.aug.strong import MEAN, STD, StrongAugment  # noqa: E402
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
    return float(np.median(times)), min(times), max(times)


def kernels(b, calls):
    x = b['images_t'].contiguous().float()
    dev = x.device
    out = torch.empty_like(x)
    ws = torch.empty(128 * N, dtype=torch.uint8, device=dev)
    table = torch.empty(N, ops.STRONG_TABLE_COLS, device=dev)
    by = 2 * x.numel() * 4
    lines = []
    for name, flags in (('jitter + blur', 3), ('jitter only', 1), ('blur only', 2), ('neither (the copy route)', 0)):
        host = np.tile(np.array([[1.1, 0.9, 1.1, 0.2, 1.15, flags, 0, 0]], np.float32), (N, 1))
        ops.strong_write_table(table, host, (S, S))
        t = median_us(lambda: ops.strong_augment(x, table, MEAN, STD, out=out, ws=ws), calls)
        lines.append('rgda_strong_augment %d x 3 x %d x %d, sigma 1.15, %s: median of %d calls %.1f us (min %.1f, max %.1f); '
                     '%.1f MB read + written -> %.0f GB/s' % (N, S, S, name, calls, *t, by / 1e6, by / t[0] / 1e3))
    t = median_us(lambda: out.copy_(x), calls)
    lines.append('plain device copy of the same tensor: median %.1f us (min %.1f, max %.1f) -> %.0f GB/s'
                 % (*t, by / t[0] / 1e3))
    t = median_us(lambda: ops.strong_write_table(table, host, (S, S)), calls)
    lines.append('rgda_strong_write_table: median %.1f us (min %.1f, max %.1f)' % t)
    return lines


def steps(b, n_steps, rounds):
    from regda_amd.models.Encoder import Deeplabv2
    from regda_amd.ssl import SSLStep
    arms = {}
    on = dict(jitter_prob=1.0, blur_prob=1.0, sigma=(1.15, 1.15))
    for name, strong in (("mix='dacs'", None), ("mix='dacs' + strong", StrongAugment(seed=0, **on)),
                         ("mix='dacs' (2nd)", None)):
        torch.manual_seed(2333)
        model = Deeplabv2(dict(backbone=dict(resnet_type='resnet101', output_stride=16, pretrained=False), multi_layer=True,
                               cascade=False, use_ppm=True, ppm=dict(num_classes=C, use_aux=False, fc_dim=2048),
                               inchannels=2048, num_classes=C, is_ins_norm=True))
        protos = torch.randn(C, 2048, generator=torch.Generator().manual_seed(0))
        st = SSLStep(model, protos, ema_decay=0.999, mix=DomainMix('dacs', C, seed=0), strong=strong)
        args = (b['images_s'], b['label_s'], b['images_t'], None, b['regs_t'])
        st.step(*args, 1e-4)
        st.record_plan(*args)
        static = st.static_inputs()
        arms[name] = (st, (static['images_s'], static['label_s'], static['images_t'], None, static['regs_t']))
        for _ in range(3):
            st.step(*arms[name][1], 1e-4)
        torch.cuda.synchronize()
    times = {k: [] for k in arms}
    for _ in range(rounds):
        for name, (st, args) in arms.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(n_steps):
                st.step(*args, 1e-4)
            e1.record()
            torch.cuda.synchronize()
            times[name].append(e0.elapsed_time(e1) / n_steps)
    return ['step %-20s ms/step per round of %d steps: %s; median %.3f; plan %s'
            % (k, n_steps, ' '.join('%.3f' % x for x in v), np.median(v), arms[k][0]._plan.stats()) for k, v in times.items()]


def main():
    calls = int(sys.argv[1]) if len(sys.argv) > 1 else 50
    n_steps = int(sys.argv[2]) if len(sys.argv) > 2 else 10
    rounds = int(sys.argv[3]) if len(sys.argv) > 3 else 4
    b = make_batch(b=N, size=S, classes=C, seed=2333, with_soft=False)
    lines = kernels(b, calls)
    if n_steps > 0:
        lines += steps(b, n_steps, rounds)
    print('\n'.join(lines))
    if len(sys.argv) > 4:
        with open(sys.argv[4], 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
