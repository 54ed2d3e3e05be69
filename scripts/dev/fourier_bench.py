"""The Fourier style transfer of the source tile (the steps' style=...) at the training shape: 8 + 8 tiles
of 3 x 512 x 512.
  (1) HIP-event times of rgda_fourier_style (6 launches) with every row on at b = 5 (beta 0.01) and b = 46 (beta 0.09), with
      every row off (the kernel's own copy route), of a plain device copy of the same bytes, and of
      rgda_fourier_style_write_table: one warm-up, then the median of `calls`;
  (2) the whole step (resnet101, online teacher, recorded plan, as bench.py runs it) without style=, with it (every
      image transformed, beta 0.01) and with it at prob = 0 (the same launches, every image copied: data bit-identical
      to the step without), every arm warmed up and recorded in ONE process and then timed in alternating rounds of
      `steps` steps each; each arm's plan size is printed next to it.
    python scripts/dev/fourier_bench.py [calls] [steps] [rounds] [out.txt]"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from regda_amd import _lib, ops  # noqa: E402
from regda_amd.aug.fourier import MEAN, STD, FourierStyle  # noqa: E402
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
    xs, xt = b['images_s'].contiguous().float(), b['images_t'].contiguous().float()
    dev = xs.device
    out = torch.empty_like(xs)
    need = _lib.lib().size('rgda_fourier_style_workspace', N, N, S, S)
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    table = torch.empty(N, ops.STYLE_TABLE_COLS, dtype=torch.int32, device=dev)
    by = 2 * xs.numel() * 4
    lines = ['workspace for %d + %d tiles of %d x %d: %.1f MB' % (N, N, S, S, need / 1e6)]
    for name, bb, on in (('b = 5 (beta 0.01)', 5, 1), ('b = 46 (beta 0.09)', 46, 1), ('every row off (the copy route)', 5, 0)):
        host = np.array([[(n + 3) % N, bb, on, 0] for n in range(N)], np.int32)
        ops.fourier_style_write_table(table, host, N, (S, S))
        t = median_us(lambda: ops.fourier_style(xs, xt, table, MEAN, STD, MEAN, STD, out=out, ws=ws), calls)
        lines.append('rgda_fourier_style %d + %d x 3 x %d x %d, %s: median of %d calls %.1f us (min %.1f, max %.1f); '
                     '%.1f MB of source read + result written -> %.0f GB/s' % (N, N, S, S, name, calls, *t, by / 1e6, by / t[0] / 1e3))
    t = median_us(lambda: out.copy_(xs), calls)
    lines.append('plain device copy of the source tensor: median %.1f us (min %.1f, max %.1f) -> %.0f GB/s'
                 % (*t, by / t[0] / 1e3))
    t = median_us(lambda: ops.fourier_style_write_table(table, host, N, (S, S)), calls)
    lines.append('rgda_fourier_style_write_table: median %.1f us (min %.1f, max %.1f)' % t)
    return lines


def steps(b, n_steps, rounds):
    from regda_amd.models.Encoder import Deeplabv2
    from regda_amd.ssl import SSLStep
    arms = {}
    # (which step object of the process an arm is matters more than what it runs -- DESIGN.md 4.2j, "In-step mix": compare
    # the first with the third and the second with the fourth)
    for name, style in (('no style', None), ('no style (2nd)', None), ('style, beta 0.01', FourierStyle(beta=0.01, seed=0)),
                        ('style, prob 0', FourierStyle(beta=0.01, prob=0.0, seed=0))):
        torch.manual_seed(2333)
        model = Deeplabv2(dict(backbone=dict(resnet_type='resnet101', output_stride=16, pretrained=False), multi_layer=True,
                               cascade=False, use_ppm=True, ppm=dict(num_classes=C, use_aux=False, fc_dim=2048),
                               inchannels=2048, num_classes=C, is_ins_norm=True))
        protos = torch.randn(C, 2048, generator=torch.Generator().manual_seed(0))
        st = SSLStep(model, protos, ema_decay=0.999, style=style)
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
    return ['step %-18s ms/step per round of %d steps: %s; median %.3f; plan %s'
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
