"""rgda_triplet_loss on the stage-2 feature map, 8 images of 2048 x 32 x 32 (n = 8192 rows, k = 2048; rows = 0.4 *
centroid[label] + noise, 7 classes, about 5 % of the rows ignored), next to a torch composition of the reference's
algorithm (regda/gast/triple.py: the (n, n) distance matrix, then a Python loop over the rows with two boolean-indexed
reductions each) on the same GPU.  HIP-event time of the op's forward and forward + gradient, and the achieved fraction
of the bf16 MFMA peak for the mining pass's Gram product over all T x T tiles (2 n^2 k flop = 0.27 TFLOP).
    python scripts/dev/triplet_bench.py [calls] [images]
Under `rocprofv3 --kernel-trace --stats -- python scripts/dev/triplet_bench.py 5 8 op` the per-kernel times (`op`
leaves the torch composition out)."""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from regda_amd import ops  # noqa: E402

MFMA_PEAK_TFLOPS = 2500.0       # dense bf16 MFMA peak of one MI355X


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


def reference_composition(x, targets, margin=0.3):
    """the reference's algorithm, statement by statement, on torch"""
    n = x.shape[0]
    dist = x.pow(2).sum(1, keepdim=True).expand(n, n)
    dist = dist + dist.t()
    dist = torch.addmm(dist, x, x.t(), beta=1, alpha=-2).clamp(min=1e-12).sqrt()
    mask = targets.expand(n, n).eq(targets.expand(n, n).t())
    d_ap, d_an = [], []
    for i in range(n):
        d_ap.append(dist[i][mask[i]].max().unsqueeze(0))
        d_an.append(dist[i][mask[i] == 0].min().unsqueeze(0))
    d_ap, d_an = torch.cat(d_ap), torch.cat(d_an)
    return torch.relu(d_ap - d_an + margin).mean()


def main():
    calls = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    b = int(sys.argv[2]) if len(sys.argv) > 2 else 8
    op_only = len(sys.argv) > 3 and sys.argv[3] == 'op'
    k, h, w = 2048, 32, 32
    n = b * h * w
    gen = torch.Generator(device='cuda').manual_seed(8192)
    labels = torch.randint(0, 7, (n,), device='cuda', generator=gen)
    centroid = torch.randn(7, k, device='cuda', generator=gen)
    rows = 0.4 * centroid[labels] + torch.randn(n, k, device='cuda', generator=gen)
    labels[torch.rand(n, device='cuda', generator=gen) < 0.05] = -1
    f = rows.view(b, h, w, k).permute(0, 3, 1, 2).contiguous()
    grad = torch.zeros(n, k, dtype=torch.bfloat16, device='cuda')
    loss = torch.zeros(1, device='cuda')
    fwd = timed(lambda: ops.triplet_loss(f, labels, 0.3, -1, 1.0, loss=loss), calls)
    both = timed(lambda: ops.triplet_loss(f, labels, 0.3, -1, 1.0, loss=loss, dfeat=grad), calls)
    loss.zero_()
    _, stats = ops.triplet_loss(f, labels, 0.3, -1, 1.0, loss=loss)
    flop = 2.0 * n * n * k
    print('%d x %d x %d x %d (n = %d): triplet_loss forward %.3f ms, forward + gradient %.3f ms; loss %.5f, (m, positive '
          'hinges) = %s; the Gram product alone is %.2f TFLOP: the forward runs at >= %.0f TFLOP/s, %.1f %% of the bf16 MFMA peak'
          % (b, k, h, w, n, fwd, both, loss.item(), tuple(stats.tolist()), flop / 1e12, flop / fwd / 1e9,
             100 * flop / fwd / 1e9 / MFMA_PEAK_TFLOPS))
    if op_only:
        return
    valid = labels != -1
    xr, tr = rows[valid].clone().requires_grad_(True), labels[valid]
    state = {}

    def composed():
        state['loss'] = reference_composition(xr, tr)
    t_fwd = timed(composed, 1, warm=1)

    def composed_backward():
        xr.grad = None
        reference_composition(xr, tr).backward()
    t_both = timed(composed_backward, 1, warm=0)
    print('torch composition of the reference on the %d valid rows: forward %.1f ms, forward + backward %.1f ms; loss %.5f'
          % (int(valid.sum()), t_fwd, t_both, state['loss'].item()))


if __name__ == '__main__':
    main()
