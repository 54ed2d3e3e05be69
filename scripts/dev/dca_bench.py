"""rgda_dca_loss on the stage-2 feature maps, 8 + 8 images of 2048 x 32 x 32 with 6 and with 16 classes (features =
0.5 * centroid[label] + noise, two logit maps = 2 * onehot + noise per domain), as AlignStep(dca_weight=) calls it: CCR
(the source a constant, the target rows receive, accumulate on) and ICR of one domain (both halves receive).  HIP-event
time per call next to the byte floor: the f32 feature map of both sides read once (134 MB for 8 + 8) plus the bf16
gradient rows written (34 MB per domain, twice that with accumulate), at 4.6 TB/s.
    python scripts/dev/dca_bench.py [calls] [images per domain]
Under `rocprofv3 --kernel-trace --stats -- python scripts/dev/dca_bench.py 5` the per-kernel times."""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from regda_amd import ops  # noqa: E402

STREAM_TBS = 4.6        # what this project's streaming kernels reach on one MI355X


def timed(fn, calls, warm=2):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / calls


def domain(b, C, c, h, w, centroid, gen):
    lab = torch.randint(0, C, (b, h * w), device='cuda', generator=gen)
    lab[:, :C] = torch.arange(C, device='cuda')
    feat = 0.5 * centroid[lab].permute(0, 2, 1) + torch.randn(b, c, h * w, device='cuda', generator=gen)
    onehot = torch.nn.functional.one_hot(lab, C).permute(0, 2, 1).float()
    logits = tuple((2.0 * onehot + torch.randn(b, C, h * w, device='cuda', generator=gen)).view(b, C, h, w) for _ in range(2))
    return feat.view(b, c, h, w).contiguous(), logits


def main():
    calls = int(sys.argv[1]) if len(sys.argv) > 1 else 10
    b = int(sys.argv[2]) if len(sys.argv) > 2 else 8
    c, h, w = 2048, 32, 32
    hw = h * w
    for C in (6, 16):
        gen = torch.Generator(device='cuda').manual_seed(2048 + C)
        centroid = torch.randn(C, c, device='cuda', generator=gen)
        (fs, ps), (ft, pt) = domain(b, C, c, h, w, centroid, gen), domain(b, C, c, h, w, centroid, gen)
        rows = torch.zeros(2 * b * hw, c, dtype=torch.bfloat16, device='cuda')
        rs, rt = rows[:b * hw], rows[b * hw:]
        loss = torch.zeros(1, device='cuda')
        q = b // 2
        feat_mb, rows_mb = 2 * b * c * hw * 4 / 1e6, b * hw * c * 2 / 1e6
        for kind in ('cov', 'mse'):
            fwd = timed(lambda: ops.dca_loss(fs, ps, ft, pt, 'logits2', kind, True, 1.0, loss=loss), calls)
            ccr = timed(lambda: ops.dca_loss(fs, ps, ft, pt, 'logits2', kind, True, 1.0, loss=loss, dfeat_b=rt), calls)
            ccr_acc = timed(lambda: ops.dca_loss(fs, ps, ft, pt, 'logits2', kind, True, 1.0, loss=loss, dfeat_b=rt,
                                                 accumulate=True), calls)
            rows.zero_()
            icr = timed(lambda: ops.dca_loss(fs[:q], tuple(p[:q] for p in ps), fs[q:], tuple(p[q:] for p in ps), 'logits2', kind,
                                             True, 1.0, loss=loss, dfeat_a=rs[:q * hw], dfeat_b=rs[q * hw:], accumulate=True), calls)
            rows.zero_()
            loss.zero_()
            ops.dca_loss(fs, ps, ft, pt, 'logits2', kind, True, 1.0, loss=loss)

            def floor(mb):
                return mb / STREAM_TBS
            print('%d + %d x %d x %d x %d, %2d classes, %s: loss %.5f | forward %.1f us (floor %.1f) | CCR forward + target rows '
                  '%.1f us (floor %.1f), accumulate %.1f us (floor %.1f) | ICR of one domain, accumulate %.1f us (floor %.1f)'
                  % (b, b, c, h, w, C, kind, loss.item(), 1e3 * fwd, floor(feat_mb), 1e3 * ccr, floor(feat_mb + rows_mb),
                     1e3 * ccr_acc, floor(feat_mb + 2 * rows_mb), 1e3 * icr, floor(feat_mb / 2 + 2 * rows_mb)))


if __name__ == '__main__':
    main()
