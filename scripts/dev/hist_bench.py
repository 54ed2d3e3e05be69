"""Histogram matching of the source tile (the steps' style=HistogramStyle) at the training shape: 8 + 8
tiles of 3 x 512 x 512.
  (1) HIP-event times of rgda_hist_style (4 launches) with every row on, for NOISE tiles (uniform levels) and for CONSTANT
      tiles (every pixel in one bin: the LDS atomics of a wave all hit one address), with every row off (the kernel's own
      copy route), of a plain device copy of the same bytes, and of rgda_hist_style_write_table: one warm-up, then the
      median of `calls`.  The floor beside them: the bytes moved (one read of N + M tiles, one read and one write of N
      tiles) over the 6.3 TB/s streaming rate of the part;
  (2) the whole step (resnet101, online teacher, recorded plan, as bench.py runs it) without style=, with it (every
      image matched) and with it at prob = 0 (the same launches, every image copied), every arm warmed up and recorded in
      ONE process and then timed in alternating rounds of `steps` steps each.
    python scripts/dev/hist_bench.py [calls] [steps] [rounds] [out.txt]"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from regda_amd import _lib  # noqa: E402
from regda_amd.aug.histogram import (MEAN, STD, HistogramStyle, hist_style, hist_style_write_table)  # noqa: E402
from regda_amd.synthetic import make_batch  # noqa: E402

N, S, C = 8, 512, 6
STREAM_BYTES_PER_S = 6.3e12     # achievable HBM streaming rate of the MI355X


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


def tiles(levels):
    mean, std = (torch.tensor(v, device='cuda').view(1, 3, 1, 1) for v in (MEAN, STD))
    return ((levels.float() - mean) / std).contiguous()


def kernels(calls):
    g = torch.Generator(device='cuda').manual_seed(2333)
    shape = (N, 3, S, S)
    contents = {
        'noise tiles': (tiles(torch.randint(0, 256, shape, device='cuda', generator=g)),
                        tiles(torch.randint(0, 256, shape, device='cuda', generator=g))),
        'constant tiles': (tiles(torch.full(shape, 90, device='cuda')), tiles(torch.full(shape, 160, device='cuda'))),
    }
    need = _lib.lib().size('rgda_hist_style_workspace', N, N, S, S)
    ws = torch.empty(need, dtype=torch.uint8, device='cuda')
    table = torch.empty(N, 4, dtype=torch.int32, device='cuda')
    out = torch.empty(shape, device='cuda')
    moved = (2 * N + 2 * N) * 3 * S * S * 4         # N + M tiles read, N read again, N written
    floor = moved / STREAM_BYTES_PER_S * 1e6
    lines = ['workspace for %d + %d tiles of %d x %d: %.1f KB; %.1f MB moved, floor %.1f us at %.1f TB/s'
             % (N, N, S, S, need / 1e3, moved / 1e6, floor, STREAM_BYTES_PER_S / 1e12)]
    on = np.array([[(n + 3) % N, 65536, 1, 0] for n in range(N)], np.int32)
    off = on.copy()
    off[:, 2] = 0
    for name, (xs, xt) in contents.items():
        for what, host in (('every row on', on), ('every row off (the copy route)', off)):
            hist_style_write_table(table, host, N, (S, S))
            t = median_us(lambda: hist_style(xs, xt, table, MEAN, STD, MEAN, STD, out=out, ws=ws), calls)
            lines.append('rgda_hist_style %d + %d x 3 x %d x %d, %s, %s: median of %d calls %.1f us (min %.1f, max %.1f) = '
                         '%.2f x floor' % (N, N, S, S, name, what, calls, *t, t[0] / floor))
    xs = contents['noise tiles'][0]
    t = median_us(lambda: out.copy_(xs), calls)
    lines.append('plain device copy of the source tensor: median %.1f us (min %.1f, max %.1f) -> %.0f GB/s'
                 % (*t, 2 * xs.numel() * 4 / t[0] / 1e3))
    t = median_us(lambda: hist_style_write_table(table, on, N, (S, S)), calls)
    lines.append('rgda_hist_style_write_table: median %.1f us (min %.1f, max %.1f)' % t)
    return lines


def steps(n_steps, rounds):
    from regda_amd.models.Encoder import Deeplabv2
    from regda_amd.ssl import SSLStep
    b = make_batch(b=N, size=S, classes=C, seed=2333, with_soft=False)
    arms = {}
    # (which step object of the process an arm is matters more than what it runs -- DESIGN.md 4.2j, "In-step mix": compare
    # the first with the third and the second with the fourth)
    for name, style in (('no style', None), ('no style (2nd)', None), ('style, blend 0.5..1', HistogramStyle(seed=0)),
                        ('style, prob 0', HistogramStyle(prob=0.0, seed=0))):
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
    return ['step %-20s ms/step per round of %d steps: %s; median %.3f; plan %s'
            % (k, n_steps, ' '.join('%.3f' % x for x in v), np.median(v), arms[k][0]._plan.stats()) for k, v in times.items()]


def main():
    calls = int(sys.argv[1]) if len(sys.argv) > 1 else 50
    n_steps = int(sys.argv[2]) if len(sys.argv) > 2 else 10
    rounds = int(sys.argv[3]) if len(sys.argv) > 3 else 4
    lines = kernels(calls)
    if n_steps > 0:
        lines += steps(n_steps, rounds)
    print('\n'.join(lines))
    if len(sys.argv) > 4:
        with open(sys.argv[4], 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
