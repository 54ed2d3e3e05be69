"""rgda_superpixels at the training shape (8 tiles of 512 x 512, S = 16, compactness 10, 10 iterations; the synthetic
rectangle scenes of tests/superpixel_ref.py): one warm-up, then the median HIP-event time of `calls` calls; launches per
call; achieved GB/s over the algorithmic bytes (the image read once per iteration and once for the initial centres, the
label map written once and read by the two component passes that need it); and the CPU time of the numpy restatement
for the same input, the only comparator there is (the reference's generators are third party and not installed).
    python scripts/dev/superpixel_bench.py [calls] [out.txt]
Under `rocprofv3 --kernel-trace --stats -- python scripts/dev/superpixel_bench.py` the per-kernel times."""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import superpixel_ref as R  # noqa: E402
from regda_amd import ops  # noqa: E402
from regda_amd.gast.superpixels import SuperPixelsSLIC  # noqa: E402

N, H, W, S, M, ITERS = 8, 512, 512, 16, 10, 10


def main():
    calls = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    imgs = np.stack([R.rectangle_scene(H, W, 100 + i) for i in range(N)])
    t = torch.from_numpy(imgs).cuda()
    gen = SuperPixelsSLIC(S, M, ITERS).reserve(N, H, W)
    regs = torch.empty(N, H, W, dtype=torch.int32, device='cuda')
    count = torch.empty(N, dtype=torch.int32, device='cuda')
    gen(t, out=(regs, count))                                   # the warm-up
    torch.cuda.synchronize()
    times = []
    for _ in range(calls):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        gen(t, out=(regs, count))
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b))
    ms = float(np.median(times))
    launches = 2 + ITERS + 7                                    # include/rgda_hip.h: rgda_superpixels
    by = N * H * W * (3 * (ITERS + 1) + 4 + 2 * 4)
    t0 = time.perf_counter()
    want = R.superpixels(imgs[0], S, M, ITERS)
    cpu = time.perf_counter() - t0
    same = np.array_equal(regs[0].cpu().numpy(), want[0]) and int(count[0]) == want[1]
    ws = ops.lib().size('rgda_superpixels_workspace', N, H, W, S)
    lines = ['rgda_superpixels %d x %d x %d, S %d, m %d, %d iterations, min_area %d: median of %d calls %.3f ms '
             '(min %.3f, max %.3f), %d launches per call' % (N, H, W, S, M, ITERS, gen.min_area, calls, ms, min(times),
                                                             max(times), launches),
             'algorithmic bytes %.1f MB -> %.1f GB/s; workspace %.1f MB; regions per tile %s'
             % (by / 1e6, by / ms / 1e6, ws / 1e6, count.cpu().tolist()),
             'numpy restatement (tests/superpixel_ref.py), ONE tile on the CPU: %.2f s -> %.1f s for the %d tiles; '
             'tile 0 bit-identical to it: %s' % (cpu, cpu * N, N, same)]
    print('\n'.join(lines))
    if len(sys.argv) > 2:
        with open(sys.argv[2], 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
