"""dev: one PseudoLabelAnalysis.update (rgda_pseudo_analysis + rgda_pseudo_analysis_fold) at 1 x 6 x 1024 x 1024,
1 x 16 x 1024 x 1024 and 8 x 6 x 512 x 512, against the per-bin formulation of the same
summary in torch ops on the same GPU (the maps, then 100 range_static passes with their host reads: how the reference
goes about it, pseudo_generation.py:177-207), image by image.  Prints both times and the achieved rate of the
soft-label read (b * C * H * W * 4 bytes per update; the maximum pass reads them a second time, mostly from cache)."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch
from regda_amd import ops
from regda_amd.gast.pseudo_generation import PseudoLabelAnalysis, entropy_bin_edges, range_static
def t_of(fn, reps):
    for _ in range(3): fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps): fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3
def per_bin_formulation(soft, gt, C, R=100):
    """The same summary the per-bin way, written from the contract (include/rgda_hip.h): three full-size maps, then one
    masked reduction per bin (range_static) whose two counts are read on the host, bin after bin."""
    _, lo, hi = entropy_bin_edges(C, R)
    chosen = ops.pseudo_select(soft, 0.8, 0.6, -1)
    chosen = torch.where(chosen < 0, torch.full_like(chosen, C), chosen)
    entropy = -(soft * soft.log()).sum(1)
    own = soft.gather(1, gt.clamp(min=0).unsqueeze(1)).squeeze(1)
    difficulty = torch.where(gt < 0, torch.ones_like(own), 1 - own)
    seen = 0
    for i in range(R):
        n_true, n_used, acc, diffi = range_static(entropy, difficulty, chosen, gt, float(lo[i]), float(hi[i]), C)
        seen += bool(n_used != 0) + bool(diffi != 0)
    return seen
g = torch.Generator().manual_seed(11)
for b, C, S in ((1, 6, 1024), (1, 16, 1024), (8, 6, 512)):
    blocks = torch.randn(b, C, S // 16, S // 16, generator=g).repeat_interleave(16, 2).repeat_interleave(16, 3)
    for name, conf in (('confident', 3.0), ('noisy', 0.5)):
        soft = torch.softmax(conf * blocks + torch.randn(b, C, S, S, generator=g), 1).contiguous().cuda()
        gt = torch.randint(-1, C, (b, S, S), generator=g).cuda()
        a = PseudoLabelAnalysis(C)
        us = t_of(lambda: a.update(soft, gt), 50)
        ref = sum(t_of(lambda: per_bin_formulation(soft[i:i + 1], gt[i:i + 1], C), 3) for i in range(b))     # (the loop is per image)
        print('%d x %2d x %4d x %4d %-9s: update %8.1f us (soft-label read %.2f TB/s)   per-bin torch ops %10.1f us  (%.0fx)'
              % (b, C, S, S, name, us, soft.numel() * 4 / us * 1e-6, ref, ref / us), flush=True)
