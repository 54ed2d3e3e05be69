"""PyCDA's region pyramid term (Lian et al., ICCV 2019, "Constructing Self-motivated Pyramid Curriculums") as a loss
module over the fused kernels (`rgda_upsample_pycda`, include/rgda_hip.h): at every level of a pyramid of square regions
the student's mean prediction over a region is drawn towards the teacher's label distribution of that region.  The
pixel level of the paper (confident pixels under CE) is the pseudo-label selection plus the target loss the steps already
have; this is the part above it.
"""
import torch

from .. import ops


class _PyramidTerm(torch.autograd.Function):
    @staticmethod
    def forward(ctx, p1, p2, soft, mod):
        heads = 1 if p2 is None else 2
        a = p1.detach()
        b = a if heads == 1 else p2.detach()
        want = ctx.needs_input_grad[0] or (heads == 2 and ctx.needs_input_grad[1])
        loss, n_active, g1, g2 = ops.upsample_pycda(a, b, soft.detach(), mod.sizes, thresh=mod.thresh,
                                                    level_weight=mod.level_weight, want_grad=want, heads=heads,
                                                    flag=mod.flag)
        mod.last_levels, mod.last_active = loss[1:], n_active
        ctx.heads = heads
        if want and heads == 1:
            ctx.grads = (g1.add_(g2).to(p1.dtype), None)
        elif want:
            ctx.grads = (g1.to(p1.dtype), g2.to(p2.dtype))
        return loss[0].clone()

    @staticmethod
    def backward(ctx, grad_out):
        g1, g2 = ctx.grads
        return grad_out * g1, None if g2 is None else grad_out * g2, None, None


class PyramidCurriculumLoss(torch.nn.Module):
    """forward(preds, soft) -> the term's total (a scalar, differentiable in the logits).  preds: one logit tensor
    (b, c, h, w) or a list of two heads (the total is then the mean over the heads); soft: the teacher's probabilities
    (b, c, H, W), no gradient.  sizes: the levels' region sides, powers of two in [2, 256], strictly increasing, 0 last =
    the whole image; a class is active in a region where its mean probability exceeds `thresh`; level_weight: one float per
    level (default 1 / L each).  After a call `last_levels` (f32 [L], the unscaled levels) and `last_active` (int32 [L],
    the regions with an active class) stay on the device; `flag_value()` is the deferred check of the input contract."""

    def __init__(self, sizes=(8, 16, 32, 64, 0), thresh=0.5, level_weight=None):
        super().__init__()
        self.sizes = ops.pycda_sizes(sizes)
        if not 0.0 <= float(thresh) <= 1.0:
            raise ValueError(f'PyramidCurriculumLoss: thresh {thresh!r} outside [0, 1]')
        self.thresh = float(thresh)
        if level_weight is not None and len(level_weight) != len(self.sizes):
            raise ValueError(f'PyramidCurriculumLoss: {len(level_weight)} level weights for {len(self.sizes)} levels')
        self.level_weight = None if level_weight is None else tuple(float(v) for v in level_weight)
        self.flag = None
        self.last_levels = self.last_active = None

    def forward(self, preds, soft):
        heads = list(preds) if isinstance(preds, (list, tuple)) else [preds]
        if len(heads) not in (1, 2):
            raise ValueError(f'PyramidCurriculumLoss: {len(heads)} predictions; one tensor or a list of two')
        if self.flag is None or self.flag.device != heads[0].device:
            self.flag = torch.zeros(1, dtype=torch.int32, device=heads[0].device)
        return _PyramidTerm.apply(heads[0], heads[1] if len(heads) == 2 else None, soft, self)

    def flag_value(self):
        """Deferred check (host sync): bit 0 = a soft value outside [0, 1] was clamped."""
        return 0 if self.flag is None else int(self.flag.item())
