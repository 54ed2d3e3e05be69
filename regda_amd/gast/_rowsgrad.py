"""What the feature-loss modules share: their ops compute the loss and, in the same call, the gradient w.r.t. the
feature inputs as pixel-major bf16 rows (the precision of the feature gradient the fused steps hand to the
instance-norm backward); backward scales the stored rows by the incoming gradient."""
import torch


def _rows(x):
    """(n, d) rows, or the pixels of an NCHW (b, d, h, w) map: -> (row count, d)"""
    return (x.shape[0], x.shape[1]) if x.dim() == 2 else (x.shape[0] * x.shape[2] * x.shape[3], x.shape[1])


def _as_input(g, shape):
    """pixel-major bf16 rows -> f32 in the input's shape"""
    if len(shape) == 2:
        return g.float()
    b, d, h, w = shape
    return g.float().view(b, h, w, d).permute(0, 3, 1, 2)


class _RowsGrad(torch.autograd.Function):
    @staticmethod
    def forward(ctx, op, *feats):
        rows = [torch.empty(_rows(f), dtype=torch.bfloat16, device=f.device) if want else None
                for f, want in zip(feats, ctx.needs_input_grad[1:])]
        loss = op(*(f.detach() for f in feats), *rows)
        ctx.save_for_backward(*rows)
        ctx.shapes = [f.shape for f in feats]
        return loss.view(())

    @staticmethod
    def backward(ctx, g):
        return (None,) + tuple(None if r is None else g * _as_input(r, s) for r, s in zip(ctx.saved_tensors, ctx.shapes))


def rows_loss(op, *feats):
    """op(*detached feats, *gradient rows) -> the f32 [1] loss at weight 1, having written d loss / d feat into the rows
    (bf16 [n, d]; None for an input that needs no gradient).  -> the scalar loss, differentiable w.r.t. feats."""
    return _RowsGrad.apply(op, *feats)
