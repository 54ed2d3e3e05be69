"""PixelContrastLoss on the stage-2 feature map, 8 images of 2048 x 32 x 32 (labels 512 x 512, four classes per image,
30 % of the predictions wrong: A = 32 anchors, n_view = 32, N = 1024 rows): HIP-event time of rgda_pixel_contrast_select,
wall time of the host plan (the read-back of the counts and the randperm draws), HIP-event time of
rgda_pixel_contrast_loss forward + gradient -- and, next to them on the same GPU and inputs, a torch composition of the
reference's algorithm (regda/gast/contrastive.py: unique / nonzero / randperm per image and class, the dense (N, N)
mask algebra, autograd backward), wall time around a synchronised call.
    python scripts/dev/pixel_contrast_bench.py [calls]"""
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from regda_amd import ops  # noqa: E402
from regda_amd.gast.contrastive import plan_anchors  # noqa: E402


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


def wall(fn, calls):
    fn()
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3 / calls


def torch_composition(feats, labels, predict, T=0.1, Tb=0.07, eps=1e-5, max_samples=1024, max_views=100):
    """the reference's algorithm step by step in torch on the GPU, forward and backward"""
    feats = feats.detach().requires_grad_(True)
    b, k, h, w = feats.shape
    lab = torch.nn.functional.interpolate(labels.unsqueeze(1).float(), (h, w), mode='nearest').squeeze(1).long().view(b, -1)
    pr = predict.view(b, -1)
    rows = feats.permute(0, 2, 3, 1).reshape(b, h * w, k)
    classes = []
    for i in range(b):
        cs = [c for c in torch.unique(lab[i]) if c != -1]
        classes.append([c for c in cs if (lab[i] == c).nonzero().shape[0] > max_views])
    total = sum(len(c) for c in classes)
    n_view = min(max_samples // total, max_views)
    X, y = [], []
    for i in range(b):
        for c in classes[i]:
            hard = ((lab[i] == c) & (pr[i] != c)).nonzero()
            easy = ((lab[i] == c) & (pr[i] == c)).nonzero()
            nh, ne = hard.shape[0], easy.shape[0]
            if nh >= n_view / 2 and ne >= n_view / 2:
                hk = n_view // 2
                ek = n_view - hk
            elif nh >= n_view / 2:
                ek = ne
                hk = n_view - ek
            else:
                hk = nh
                ek = n_view - hk
            idx = torch.cat((hard[torch.randperm(nh)[:hk].to(hard.device)], easy[torch.randperm(ne)[:ek].to(easy.device)]), 0)
            X.append(rows[i, idx, :].squeeze(1))
            y.append(c)
    X, y = torch.stack(X), torch.stack(y).view(-1, 1)
    A = X.shape[0]
    mask = torch.eq(y, y.T).float()
    F = torch.cat(torch.unbind(X, dim=1), dim=0)
    adc = torch.matmul(F, F.T) / T
    logits = adc - adc.max(1, keepdim=True).values.detach()
    mask = mask.repeat(n_view, n_view)
    neg_mask = 1 - mask
    mask = mask * (1 - torch.eye(A * n_view, device=F.device))
    neg = (torch.exp(logits) * neg_mask).sum(1, keepdim=True)
    log_prob = logits - torch.log(torch.exp(logits) + neg + eps)
    loss = (-(T / Tb) * (mask * log_prob).sum(1) / (mask.sum(1) + eps)).mean()
    loss.backward()
    return loss


def main():
    calls = int(sys.argv[1]) if len(sys.argv) > 1 else 10
    b, k, h, w, C = 8, 2048, 32, 32, 7
    gen = torch.Generator(device='cuda').manual_seed(1024)
    feats = torch.randn(b, k, h, w, device='cuda', generator=gen)
    down = (torch.arange(w, device='cuda') // (w // 4))[None, None, :].expand(b, h, w).clone()
    down = (down + torch.arange(b, device='cuda')[:, None, None]) % C
    labels = down.repeat_interleave(16, 1).repeat_interleave(16, 2).contiguous()
    predict = torch.where(torch.rand(b, h, w, device='cuda', generator=gen) < 0.3, (down + 1) % C, down)
    t_sel = timed(lambda: ops.pixel_contrast_select(labels, predict, C, (h, w)), calls)
    counts, order, _ = ops.pixel_contrast_select(labels, predict, C, (h, w))
    t_plan = wall(lambda: [t.cuda() for t in plan_anchors(counts.cpu())], calls)
    anchors, ranks = (t.cuda() for t in plan_anchors(counts.cpu()))
    g = torch.empty(b * h * w, k, dtype=torch.bfloat16, device='cuda')
    loss = torch.zeros(1, device='cuda')
    t_loss = timed(lambda: ops.pixel_contrast_loss(feats, order, counts, anchors, ranks, loss=loss, dfeat=g), calls)
    t_fwd = timed(lambda: ops.pixel_contrast_loss(feats, order, counts, anchors, ranks, loss=loss), calls)
    t_ref = wall(lambda: torch_composition(feats, labels, predict), calls)
    print('%d x %d x %d x %d, A = %d, n_view = %d, N = %d: select %.3f ms, host plan %.3f ms, loss forward + gradient %.3f ms '
          '(forward %.3f ms), together %.3f ms; torch composition of the reference forward + backward %.3f ms'
          % (b, k, h, w, anchors.shape[0], ranks.shape[1], ranks.numel(), t_sel, t_plan, t_loss, t_fwd, t_sel + t_plan + t_loss, t_ref))


if __name__ == '__main__':
    main()
