"""rgda_transnorm_fwd / rgda_transnorm_bwd at (16, 2048, 32, 32) (plane route) and (16, 2048) (row route), training
mode with running vectors: HIP-event time and achieved GB/s of the forward and of the backward, next to the torch
composition of the same layer (tests/transnorm_ref.py evaluated in float32 on the GPU: forward alone, and forward +
the backward formulae), in the same process, the two alternating over ROUNDS rounds; the median and the spread
(min .. max) of the rounds are printed.
    python scripts/dev/transnorm_bench.py [calls]
Bytes counted for the rate: what the passes must move -- forward x twice and y once (12 B per value), backward g and x
twice each and dx once (20 B per value); the torch composition is charged the same bytes, so its rate says how far its
many passes are from that need.  Under `rocprofv3 --kernel-trace --stats -- python scripts/dev/transnorm_bench.py` the
per-kernel times."""
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import transnorm_ref as R  # noqa: E402
from regda_amd import ops  # noqa: E402

ROUNDS = 5


def timed(fn, calls):
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / calls * 1e3          # us


def main():
    calls = int(sys.argv[1]) if len(sys.argv) > 1 else 300
    gen = torch.Generator().manual_seed(1)
    for shape in ((16, 2048, 32, 32), (16, 2048)):
        C = shape[1]
        x = (torch.randn(shape, generator=gen) * 1.5 + 0.5).cuda()
        g = torch.randn(shape, generator=gen).cuda()
        w, b = (torch.rand(C, generator=gen) + 0.5).cuda(), torch.randn(C, generator=gen).cuda()
        running = (torch.zeros(C).cuda(), torch.ones(C).cuda(), torch.zeros(C).cuda(), torch.ones(C).cuda())
        n_src = shape[0] // 2
        y, dx = torch.empty_like(x), torch.empty_like(x)
        _, saved = ops.transnorm_forward(x, n_src, w, b, running, out=y)
        n = calls if x.numel() > 1 << 20 else calls * 10
        arms = (('kernels forward', lambda: ops.transnorm_forward(x, n_src, w, b, running, out=y), 12),
                ('kernels backward', lambda: ops.transnorm_backward(g, x, saved, n_src, w, dx=dx), 20),
                ('torch forward', lambda: R.transnorm_train(x, w, b, running), 12),
                ('torch forward + backward', lambda: R.transnorm_train(x, w, b, running, g=g), 32))
        for _, fn, _ in arms:          # every arm warm before the first timed round
            for _ in range(3):
                fn()
        times = {name: [] for name, _, _ in arms}
        for _ in range(ROUNDS):
            for name, fn, _ in arms:
                times[name].append(timed(fn, n))
        print('transnorm %s, %d calls per round, %d rounds:' % ('x'.join(map(str, shape)), n, ROUNDS))
        for name, _, per_value in arms:
            t = times[name]
            med = statistics.median(t)
            print('  %-26s %9.1f us (%.1f .. %.1f)  %7.1f GB/s of the %d B per value the pass needs'
                  % (name, med, min(t), max(t), x.numel() * per_value / med / 1e3, per_value))
        kb = statistics.median(times['kernels backward'])
        tb = statistics.median(times['torch forward + backward']) - statistics.median(times['torch forward'])
        print('  torch backward alone (difference of the medians) %.1f us; kernels over torch: forward %.2fx, backward %.2fx'
              % (tb, statistics.median(times['torch forward']) / statistics.median(times['kernels forward']), tb / kb))


if __name__ == '__main__':
    main()
