"""rgda_mmd_loss next to rgda_coral_loss on the same inputs: the stage-1 / stage-2 feature map, 8 + 8 images of
2048 x 32 x 32 (n = 16384 rows, d = 2048; ReLU-like features, the target scaled and shifted).  HIP-event time of forward +
gradient of both, and the achieved fraction of the bf16 MFMA peak for MMD's three matrix products (the Gram product on
the upper triangle, n^2 d MACs, and the gradient product W X, n^2 d MACs: 3 n^2 d flop = 1.65 TFLOP).
    python scripts/dev/mmd_bench.py [calls] [images per domain]
Under `rocprofv3 --kernel-trace --stats -- python scripts/dev/mmd_bench.py` the per-kernel times."""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from regda_amd import ops  # noqa: E402

MFMA_PEAK_TFLOPS = 2500.0       # dense bf16 MFMA peak of one MI355X


def timed(fn, calls):
    for _ in range(2):
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
    calls = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    b = int(sys.argv[2]) if len(sys.argv) > 2 else 8
    d, h, w = 2048, 32, 32
    gen = torch.Generator(device='cuda').manual_seed(16384)
    base = torch.rand(1, d, 1, 1, device='cuda', generator=gen) * 1.5
    f = torch.clamp(base + torch.randn(2 * b, d, h, w, device='cuda', generator=gen), min=0.0)
    f[b:] = f[b:] * 1.3 + 0.2
    n = 2 * b * h * w
    rows = torch.zeros(n, d, dtype=torch.bfloat16, device='cuda')
    loss = torch.zeros(1, device='cuda')
    half = b * h * w
    mmd = timed(lambda: ops.mmd_loss(f[:b], f[b:], 1.0, loss=loss, dfeat_s=rows[:half], dfeat_t=rows[half:]), calls)
    mmd_fwd = timed(lambda: ops.mmd_loss(f[:b], f[b:], 1.0, loss=loss), calls)
    coral = timed(lambda: ops.coral_loss(f[:b], f[b:], 1.0, loss=loss, dfeat_s=rows[:half], dfeat_t=rows[half:]), calls)
    flop_mmd = 3.0 * n * n * d
    flop_coral = 3.0 * n * d * d          # both covariances on the upper triangle (n d^2), the gradient product (2 n d^2)
    print('%d + %d x %d x %d x %d (n = %d): mmd_loss forward + gradient %.3f ms (forward %.3f ms), %.2f TFLOP -> %.0f TFLOP/s, '
          '%.1f %% of the bf16 MFMA peak; coral_loss forward + gradient %.3f ms, %.2f TFLOP -> %.0f TFLOP/s, %.1f %%'
          % (b, b, d, h, w, n, mmd, mmd_fwd, flop_mmd / 1e12, flop_mmd / mmd / 1e9, 100 * flop_mmd / mmd / 1e9 / MFMA_PEAK_TFLOPS,
             coral, flop_coral / 1e12, flop_coral / coral / 1e9, 100 * flop_coral / coral / 1e9 / MFMA_PEAK_TFLOPS))


if __name__ == '__main__':
    main()
