"""The in-step cross-domain mix (SSLStep(mix=...)) at the training shape: 8 + 8 tiles of 512 x 512, C = 6.
  (1) HIP-event times of the select call (rgda_mix_select_classes) and of the two table launches (rgda_domain_mix_table:
      the image pass, out of place, and the label pass on the pseudo labels), one warm-up, then the median of `calls`;
  (2) the whole step (resnet101, online teacher, recorded plan, as bench.py runs it) with and without mix=, every arm
      warmed up and recorded in ONE process and then timed in alternating rounds of `steps` steps each.
    python scripts/dev/mix_step_bench.py [calls] [steps] [rounds] [out.txt]"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from regda_amd import ops  # noqa: E402
from regda_amd.aug.mix import DomainMix  # noqa: E402
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
    dev = b['images_s'].device
    table = torch.zeros(N, ops.MIX_TABLE_COLS, dtype=torch.int32, device=dev)
    ranks_host = np.stack([np.random.default_rng(n).permutation(C) for n in range(N)]).astype(np.uint8)
    ranks = torch.empty(N, C, dtype=torch.uint8, device=dev)
    ops.mix_write_table(table, C, ranks=ranks, ranks_host=ranks_host)
    ws = torch.empty(N, dtype=torch.int32, device=dev)
    out = torch.empty_like(b['images_t'])
    hard = torch.zeros_like(b['label_s'])
    lines = []
    t = median_us(lambda: ops.mix_select_classes(b['label_s'], ranks, table, ws=ws), calls)
    lines.append('rgda_mix_select_classes %d x %d x %d, C %d (3 launches): median of %d calls %.1f us (min %.1f, max %.1f); '
                 '%.1f MB of labels' % (N, S, S, C, calls, *t, 8 * N * S * S / 1e6))
    lab = b['label_s']
    bits = table[:, 0].to(torch.int64).view(-1, 1, 1)
    cond = (lab >= 0) & (((bits >> lab.clamp(0, 31)) & 1) == 1)
    pasted = float(cond.float().mean())
    t = median_us(lambda: ops.domain_mix_table(b['images_s'], lab, table, ops.MIX_CLASS, images_in=b['images_t'],
                                               images_out=out, class_num=C), calls)
    by = N * S * S * (8 + 12 + 12)
    lines.append('rgda_domain_mix_table, image pass (%.1f %% pasted): median %.1f us (min %.1f, max %.1f); %.1f MB -> %.0f GB/s'
                 % (100 * pasted, *t, by / 1e6, by / t[0] / 1e3))
    t = median_us(lambda: ops.domain_mix_table(b['images_s'], lab, table, ops.MIX_CLASS, label_t=hard, class_num=C), calls)
    by = N * S * S * (8 + 8 * pasted)
    lines.append('rgda_domain_mix_table, label pass: median %.1f us (min %.1f, max %.1f); %.1f MB -> %.0f GB/s'
                 % (*t, by / 1e6, by / t[0] / 1e3))
    t = median_us(lambda: ops.mix_write_table(table, C, ranks=ranks, ranks_host=ranks_host), calls)
    lines.append('rgda_mix_write_table: median %.1f us (min %.1f, max %.1f)' % t)
    return lines


def steps(b, n_steps, rounds):
    from regda_amd.models.Encoder import Deeplabv2
    from regda_amd.ssl import SSLStep
    arms = {}
    # two controls tell the mix's own cost from what differs between two step objects of one process (buffer placement,
    # the plans' memory pools): a second step without a mix, and a mix whose coin never mixes (same launches, empty table)
    for name, mix in (('mix=None', None), ("mix='dacs'", DomainMix('dacs', C, seed=0)), ('mix=None (2nd)', None),
                      ("mix='class' p=0", DomainMix('class', C, prob=0.0, seed=0)),
                      ("mix='class'", DomainMix('class', C, seed=0))):
        torch.manual_seed(2333)
        model = Deeplabv2(dict(backbone=dict(resnet_type='resnet101', output_stride=16, pretrained=False), multi_layer=True,
                               cascade=False, use_ppm=True, ppm=dict(num_classes=C, use_aux=False, fc_dim=2048),
                               inchannels=2048, num_classes=C, is_ins_norm=True))
        protos = torch.randn(C, 2048, generator=torch.Generator().manual_seed(0))
        st = SSLStep(model, protos, ema_decay=0.999, mix=mix)
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
    return ['step %-16s ms/step per round of %d steps: %s; median %.3f' % (k, n_steps, ' '.join('%.3f' % x for x in v), np.median(v))
            for k, v in times.items()]


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
