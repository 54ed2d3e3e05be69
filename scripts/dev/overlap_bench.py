"""dev: the region-overlap term (rgda_upsample_overlap) at 8 x C x 33 x 33 -> 512 x 512 for C = 6, 7, 16: HIP-event time
per call with gradients accumulated (the way the steps launch it) and without gradients (the statistic pass and the
global stage alone: the difference is the gradient pass and the column kernel), next to rgda_upsample_ce on the same
tensors in the same process (calls alternated, several rounds: the spread is printed).  Writes the table to
profiles/overlap_term.txt as well.
    python scripts/dev/overlap_bench.py [--out PATH]"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import torch

from regda_amd import ops


def t_of(fn, reps=200):
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3


def alternate(runs, rounds=5, reps=200):
    """{name: [us per call, one value per round]}, the runs taken in turn within every round."""
    for _, fn in runs:
        for _ in range(10):
            fn()
    times = {name: [] for name, _ in runs}
    for _ in range(rounds):
        for name, fn in runs:
            times[name].append(t_of(fn, reps))
    return times


def term_calls(c, out):
    g = torch.Generator().manual_seed(c)
    b, h, H = 8, 33, 512
    p1, p2 = (torch.randn(b, c, h, h, generator=g) * 3).cuda(), (torch.randn(b, c, h, h, generator=g) * 3).cuda()
    lab = torch.randint(-1, c, (b, H, H), generator=g).cuda()
    g1, g2 = torch.zeros_like(p1), torch.zeros_like(p2)
    c1, c2 = torch.zeros_like(p1), torch.zeros_like(p2)
    ws = ops.upsample_overlap_workspace(p1, lab.shape)
    loss = torch.zeros(1, device='cuda')
    index = torch.zeros(2, c, device='cuda')
    present = torch.zeros(c, dtype=torch.int32, device='cuda')
    keep = dict(loss=loss, index=index, present=present, ws=ws)
    runs = [('ce', lambda: ops.upsample_ce(p1, p2, lab, g1=c1, g2=c2)),
            ('overlap', lambda: ops.upsample_overlap(p1, p2, lab, weight=0.1, g1=g1, g2=g2, accumulate=True, **keep)),
            ('overlap no grad', lambda: ops.upsample_overlap(p1, p2, lab, want_grad=False, **keep))]
    times = alternate(runs)
    npix = b * H * H
    low = 2 * b * c * h * h * 4                                 # the logits of both heads
    row_t = 2 * b * H * 2 * c * h * 4                           # the row-contracted gradient, written and read
    part = b * H * 7 * c * 4 * 2                                # the row partials, written and read
    nbytes = {'ce': npix * 8 + 2 * low + row_t, 'overlap no grad': npix * 8 + low + part,
              'overlap': 2 * npix * 8 + 2 * low + part + row_t + 2 * low}
    med = {name: sorted(ts)[len(ts) // 2] for name, ts in times.items()}
    print('C = %d: loss %.4f, index (head 1) %s' % (c, float(loss), [round(v, 3) for v in index[0].tolist()]), file=out)
    for name, _ in runs:
        ts = sorted(times[name])
        print('  %-16s %7.1f us median of %d rounds (min %.1f, max %.1f)  %.2fx ce   %6.1f MB algorithmic' %
              (name, med[name], len(ts), ts[0], ts[-1], med[name] / med['ce'], nbytes[name] / 1e6), file=out)
    print('  gradient pass + column kernel (the difference): %.1f us' % (med['overlap'] - med['overlap no grad']), file=out)
    out.flush()


class Tee:
    def __init__(self, *files):
        self.files = files

    def write(self, s):
        for f in self.files:
            f.write(s)

    def flush(self):
        for f in self.files:
            f.flush()


if __name__ == '__main__':
    path = sys.argv[sys.argv.index('--out') + 1] if '--out' in sys.argv else os.path.join(ROOT, 'profiles', 'overlap_term.txt')
    with open(path, 'w') as f:
        out = Tee(sys.stdout, f)
        print('rgda_upsample_overlap against rgda_upsample_ce, 8 x C x 33 x 33 -> 512 x 512, %s, torch %s' %
              (torch.cuda.get_device_name(0), torch.__version__), file=out)
        print('(scripts/dev/overlap_bench.py: HIP events around 200 calls, 5 rounds, the three calls alternated)', file=out)
        for c in (6, 7, 16):
            term_calls(c, out)
