"""rgda_saw_loss at the production shape (8 x 2048 x 32 x 32, 6 classes, relax_denom 2.0; the inputs of
tests/test_saw_gpu.py): HIP-event time of forward + gradient and of the forward alone, next to the byte floor (one read
of the b G C gathered fp32 planes; with the gradient one write of the bf16 rows more, at the HBM rate of DESIGN.md
section 7) and next to what the chosen gradient route moves (the planes again, the fp32 slot gradients written and
read, the bf16 rows read and written: DESIGN.md 4.2q).
    python scripts/dev/saw_bench.py [calls]
Under `rocprofv3 --kernel-trace --stats -- python scripts/dev/saw_bench.py` the per-kernel times."""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
from saw_ref import production_inputs  # noqa: E402
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
    feats, W = production_inputs()
    feats, W = feats.cuda(), W.cuda()
    b, k, h, w = feats.shape
    sel = list(range(6))
    C, G = len(sel), k // len(sel)
    rows = torch.zeros(b * h * w, k, dtype=torch.bfloat16, device='cuda')
    loss = torch.zeros(1, device='cuda')
    both = timed(lambda: ops.saw_loss(feats, W, sel, 2.0, 1.0, loss=loss, dfeat=rows, accumulate=True), calls)
    plain = timed(lambda: ops.saw_loss(feats, W, sel, 2.0, 1.0, loss=loss, dfeat=rows), calls)
    fwd = timed(lambda: ops.saw_loss(feats, W, sel, 2.0, 1.0, loss=loss), calls)
    # every group active (relax_denom 0): the most the gradient route can move
    full = timed(lambda: ops.saw_loss(feats, W, sel, 0, 1.0, loss=loss, dfeat=rows, accumulate=True), calls)
    planes, wr = b * G * C * h * w * 4, rows.numel() * 2
    floor_f = planes / (HBM_TBS * 1e12) * 1e3
    floor_b = (planes + wr) / (HBM_TBS * 1e12) * 1e3
    _, ws = ops.saw_loss(feats, W, sel, 2.0, return_ws=True)
    active = ops.saw_tables(ws, b, k, C)['active'].float().mean().item()
    print('saw_loss %dx%dx%dx%d classes 6 relax_denom 2.0 (%.0f %% of the groups active): forward + gradient %.3f ms '
          '(accumulate; %.3f ms plain), forward %.3f ms; relax_denom 0 (all active) forward + gradient %.3f ms'
          % (b, k, h, w, 100 * active, both, plain, fwd, full))
    print('byte floor at %.1f TB/s: forward (%.1f MB of planes read) %.3f ms -> %.1fx; forward + gradient (+ %.1f MB of '
          'rows written) %.3f ms -> %.1fx' % (HBM_TBS, planes / 1e6, floor_f, fwd / floor_f, wr / 1e6, floor_b, both / floor_b))


if __name__ == '__main__':
    main()
