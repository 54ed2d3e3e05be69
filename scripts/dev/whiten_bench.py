"""rgda_whiten_loss at the production shape (8 x 2048 x 32 x 32, 32 groups, 6 classes; the inputs of
tests/test_whiten_gpu.py): HIP-event time of forward + gradient and of the forward alone, next to the byte floor
(one read of the fp32 features + one write of the bf16 gradient at the HBM rate of DESIGN.md section 7).
    python scripts/dev/whiten_bench.py [calls]
Under `rocprofv3 --kernel-trace --stats -- python scripts/dev/whiten_bench.py` the per-kernel times."""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
from whiten_ref import production_inputs  # noqa: E402
from regda_amd import ops  # noqa: E402

HBM_TBS = 6.3       # the achievable HBM rate of DESIGN.md section 7


def timed(fn, calls):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / calls


def main():
    calls = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    feats, lab = production_inputs()
    feats, lab = feats.cuda(), lab.cuda()
    b, k, h, w = feats.shape
    rows = torch.zeros(b * h * w, k, dtype=torch.bfloat16, device='cuda')
    loss = torch.zeros(1, device='cuda')
    both = timed(lambda: ops.whiten_loss(feats, lab, 6, 32, -1, 1.0, loss=loss, dfeat=rows, accumulate=True), calls)
    fwd = timed(lambda: ops.whiten_loss(feats, lab, 6, 32, -1, 1.0, loss=loss), calls)
    rd, wr = feats.numel() * 4, rows.numel() * 2
    floor = (rd + wr) / (HBM_TBS * 1e12) * 1e3
    print('whiten_loss %dx%dx%dx%d groups 32 classes 6: forward + gradient %.3f ms, forward %.3f ms; byte floor '
          '(%.1f MB of features read + %.1f MB of gradient written at %.1f TB/s) %.3f ms -> %.1fx'
          % (b, k, h, w, both, fwd, rd / 1e6, wr / 1e6, HBM_TBS, floor, both / floor))


if __name__ == '__main__':
    main()
