"""WeightedBCEWithLogitsLoss -- mirror of regda/loss.py:60-85 (CLAN's loss, Luo et al., CVPR 2019) on rgda_wbce_logits
(csrc/clan_kernels.hip): mean or sum over the elements of (alpha + beta * weight) * BCE-with-logits(input, target), the
plain BCE with weight None.

Same constructor and call signature.  The loss and both gradients come out of one forward call of the kernel at the
input's own size (the kernel's upsample is then the identity); backward only scales them.  Served: f32 tensors on the GPU,
`weight` of the input's size (the reference would broadcast a smaller one).  As in the reference a target of another size
is a ValueError; so is a target that requires a gradient (the reference's formula has one, no caller uses it, the kernel
does not form it)."""
import torch
import torch.nn as nn

from . import ops


class _WbceFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, input, target, weight, alpha, beta, mean):
        shape = input.shape
        b, H, W = (int(torch.Size(shape[:-2]).numel()), shape[-2], shape[-1]) if input.dim() >= 2 else (1, 1, input.numel())
        z = input.detach().contiguous().view(b, H, W)
        wm = None if weight is None else weight.detach().contiguous().view(b, H, W)
        need_gw = weight is not None and ctx.needs_input_grad[2]
        loss, dz, gw = ops.wbce_logits(z, (H, W), target.detach().contiguous().view(b, H, W), wm, alpha, beta, 1.0, mean,
                                       want_dz=ctx.needs_input_grad[0], want_gw=need_gw)
        ctx.save_for_backward(dz, gw)
        ctx.shape = shape
        return loss.view(())

    @staticmethod
    def backward(ctx, g):
        dz, gw = ctx.saved_tensors
        return (None if dz is None else (dz * g).view(ctx.shape), None, None if gw is None else (gw * g).view(ctx.shape),
                None, None, None)


class WeightedBCEWithLogitsLoss(nn.Module):
    def __init__(self, size_average=True):
        super().__init__()
        self.size_average = size_average

    def forward(self, input, target, weight, alpha, beta):
        if target.size() != input.size():
            raise ValueError('Target size ({}) must be the same as input size ({})'.format(target.size(), input.size()))
        if target.requires_grad:
            raise ValueError('WeightedBCEWithLogitsLoss: the target is a constant here; detach it')
        if weight is not None and weight.size() != input.size():
            raise ValueError('Weight size ({}) must be the same as input size ({})'.format(weight.size(), input.size()))
        for t in (input, target, weight):
            if t is not None and (t.dtype != torch.float32 or not t.is_cuda):
                raise ValueError('WeightedBCEWithLogitsLoss: f32 tensors on the GPU (there is no CPU fallback)')
        if input.numel() == 0:
            raise ValueError('WeightedBCEWithLogitsLoss: an empty input')
        return _WbceFn.apply(input, target, weight, float(alpha), float(beta), bool(self.size_average))
