"""PixelDiscriminator -- mirror of regda/models/Discriminator.py:60-78 (FADA's feature-space, class-level discriminator,
Wang et al., ECCV 2020) on the kernels of csrc/fada_kernels.hip and the generic convolution routes.

Same constructor, the reference's parameter names and OIHW layout (`D.0`, `D.2`, `cls1`, `cls2` `.weight/.bias`, f32), so
`state_dict()` round-trips with a reference checkpoint and a caller's `torch.optim` sees ordinary `.grad`s.  The forward
packs the f32 NCHW input as bf16 pixel rows (`rgda_feat_pack_rows`), runs D.0 and D.2 on `rgda_conv2d` (3 x 3, pad 1)
followed by `rgda_disc_bias_lrelu`, and both heads as one 32-column MFMA convolution (`rgda_fada_head`, source half
first); the backward is one `torch.autograd.Function` over the head's data gradient (`rgda_fada_head_bwd_data`), the
generic data gradients (`rgda_conv2d` mode 1 on the transposed operand copies, `rgda_lrelu_mask_rows` behind D.2's), the
generic deterministic weight gradient and the fixed-order bias sums.  The bf16 operand copies of the weights (both
orientations; the heads stacked into one [32][9][ndf/2] operand with zero rows beyond 2 * num_classes) are rebuilt when a
parameter's `_version` has moved, e.g. after an optimizer step.

It lives in its own module: `regda_amd.models.Discriminator` holds FCDiscriminator only.

Served: f32 inputs on the GPU, input_nc % 64 == 0 and ndf == 64 or ndf % 128 == 0 (rgda_conv2d takes operands of 64 n
channels; at ndf = 64 D.2's data gradient has the head's 32-column geometry and runs on the head's kernel),
1 <= num_classes <= 16, any H, W >= 1; anything else raises with the cause.
"""
import torch
import torch.nn as nn

from .. import ops

PARAMS = ('D.0.weight', 'D.0.bias', 'D.2.weight', 'D.2.bias', 'cls1.weight', 'cls1.bias', 'cls2.weight', 'cls2.bias')


def _taps_last(w):
    """OIHW f32 -> [O, 9, I]"""
    return w.permute(0, 2, 3, 1).reshape(w.shape[0], 9, w.shape[1])


def _oihw(dw):
    """[O, 9, I] -> OIHW"""
    return dw.view(dw.shape[0], 3, 3, dw.shape[2]).permute(0, 3, 1, 2).contiguous()


class PixelOperands:
    """The kernels' view of the parameters: wf bf16 [Cout, 9, Cin] and wt bf16 [Cin, 9, Cout] (rgda_weight_transpose_bf16)
    of D.0, D.2 and the stacked heads ([32, 9, ndf/2], zero rows beyond 2 nc), and the f32 biases (the heads' padded to 32)."""

    def __init__(self, module):
        nc = module.num_classes
        dev = module.cls1.weight.device
        heads = torch.zeros((ops.FADA_CP, 9, module.cls1.weight.shape[1]), dtype=torch.float32, device=dev)
        heads[:nc] = _taps_last(module.cls1.weight.detach())
        heads[nc:2 * nc] = _taps_last(module.cls2.weight.detach())
        self.wf, self.wt, self.bias = [], [], []
        for w32 in (_taps_last(module.D[0].weight.detach()).contiguous(), _taps_last(module.D[2].weight.detach()).contiguous(),
                    heads):
            Co, _, Ci = w32.shape
            wt = torch.empty((Ci, 9, Co), dtype=torch.bfloat16, device=dev)
            ops.weight_transpose_bf16(w32, wt, Co, 9, Ci)
            self.wf.append(w32.to(torch.bfloat16))
            self.wt.append(wt)
        bh = torch.zeros(ops.FADA_CP, dtype=torch.float32, device=dev)
        bh[:nc] = module.cls1.bias.detach()
        bh[nc:2 * nc] = module.cls2.bias.detach()
        self.bias = [module.D[0].bias.detach().contiguous(), module.D[2].bias.detach().contiguous(), bh]
        self.nc = nc


def trunk_rows(op, X, b, H, W):
    """X bf16 [b*H*W, input_nc] -> [X, a1, a2]: D.0 and D.2 with their LeakyReLUs, stored after the activation"""
    acts = [X]
    for i in range(2):
        y = torch.empty((b * H * W, op.wf[i].shape[0]), dtype=torch.bfloat16, device=X.device)
        ops.conv2d(acts[-1], op.wf[i], y, b, H, W, H, W, 3, 3, 1, 1, 1)
        acts.append(ops.disc_bias_lrelu(y, op.bias[i]))
    return acts


def backward_rows(op, dz, acts, b, H, W, need_dparams=True, need_dinput=True, onto=None):
    """dz bf16 [b*H*W, 32], the gradient of the heads' output -> (dX bf16 [b*H*W, input_nc], grads): grads maps the
    reference's parameter names to OIHW f32 gradients (empty without need_dparams); dX is None without need_dinput.
    onto: bf16 rows of dX's shape that the input gradient is ADDED to in the convolution's epilogue (one rounding) --
    they are then the result."""
    X, a1, a2 = acts
    nc, grads = op.nc, {}

    def params(name, x, g):
        dw = torch.zeros((g.shape[1], 9, x.shape[1]), dtype=torch.float32, device=g.device)
        ops.conv2d_wgrad_grouped([(x, g, dw, b, H, W, H, W, 3, 3, 1, 1, 1)])
        return dw, ops.disc_bias_grad(g)
    if need_dparams:
        dw, db = params('heads', a2, dz)
        grads['cls1.weight'], grads['cls1.bias'] = _oihw(dw[:nc]), db[:nc].clone()
        grads['cls2.weight'], grads['cls2.bias'] = _oihw(dw[nc:2 * nc]), db[nc:2 * nc].clone()
    g2 = ops.fada_head_backward_data(dz, op.wt[2], a2, b, H, W)
    if need_dparams:
        dw, grads['D.2.bias'] = params('D.2', a1, g2)
        grads['D.2.weight'] = _oihw(dw)
    if g2.shape[1] == ops.FADA_CP:      # ndf = 64: 32 gradient columns, the head's geometry (rgda_conv2d refuses them)
        g1 = ops.fada_head_backward_data(g2, op.wt[1], a1, b, H, W)
    else:
        g1 = torch.empty_like(a1)
        ops.conv2d(g2, op.wt[1], g1, b, H, W, H, W, 3, 3, 1, 1, 1, mode=1)
        ops.lrelu_mask_rows(g1, a1)
    if need_dparams:
        dw, grads['D.0.bias'] = params('D.0', X, g1)
        grads['D.0.weight'] = _oihw(dw)
    dX = None
    if need_dinput:
        dX = onto if onto is not None else torch.empty_like(X)
        # res and y are the same rows: the epilogue's lane reads res[m][co .. co+7] and then writes y at those elements,
        # and no other lane touches them
        ops.conv2d(g1, op.wt[0], dX, b, H, W, H, W, 3, 3, 1, 1, 1, mode=1, res=onto)
    return dX, grads


def pack_dz(gz):
    """f32 (b, 2 nc, H, W) -> bf16 [b*H*W, 32] with the dead columns zero"""
    b, c, H, W = gz.shape
    rows = torch.zeros((b * H * W, ops.FADA_CP), dtype=torch.bfloat16, device=gz.device)
    return ops.feat_pack_rows(gz, out=rows)


class _PixelFn(torch.autograd.Function):
    """z = D(x); gradients for x and the eight parameters"""

    @staticmethod
    def forward(ctx, module, x, *params):
        op = module.operands()
        b, _, H, W = x.shape
        acts = trunk_rows(op, ops.feat_pack_rows(x), b, H, W)
        z = ops.fada_head(acts[2], op.wf[2], op.bias[2], b, H, W, op.nc)
        ctx.op, ctx.acts, ctx.shape = op, acts, tuple(x.shape)
        return z.view(b, H, W, ops.FADA_CP)[..., :2 * op.nc].permute(0, 3, 1, 2).contiguous()

    @staticmethod
    def backward(ctx, gz):
        b, C, H, W = ctx.shape
        need_dp = any(ctx.needs_input_grad[2:])
        dX, grads = backward_rows(ctx.op, pack_dz(gz.float()), ctx.acts, b, H, W, need_dp, ctx.needs_input_grad[1])
        dx = None
        if ctx.needs_input_grad[1]:
            dx = ops.feat_unpack_rows(dX, torch.empty((b, C, H, W), dtype=torch.float32, device=dX.device))
        out = [grads.get(k) if need else None for k, need in zip(PARAMS, ctx.needs_input_grad[2:])]
        return (None, dx, *out)


class PixelDiscriminator(nn.Module):
    PARAMS = PARAMS

    def __init__(self, input_nc, ndf=512, num_classes=1):
        super().__init__()
        # nn.Conv2d holds the parameters under the reference's names with the reference's initialisation; the convolutions
        # themselves run in forward() below
        self.D = nn.Sequential(
            nn.Conv2d(input_nc, ndf, kernel_size=3, stride=1, padding=1),
            nn.LeakyReLU(negative_slope=ops.DISC_SLOPE, inplace=True),
            nn.Conv2d(ndf, ndf // 2, kernel_size=3, stride=1, padding=1),
            nn.LeakyReLU(negative_slope=ops.DISC_SLOPE, inplace=True))
        self.cls1 = nn.Conv2d(ndf // 2, num_classes, kernel_size=3, stride=1, padding=1)
        self.cls2 = nn.Conv2d(ndf // 2, num_classes, kernel_size=3, stride=1, padding=1)
        self.input_nc, self.ndf, self.num_classes = input_nc, ndf, num_classes
        self._op, self._op_versions = None, None

    def _params(self):
        return [self.get_parameter(k) for k in self.PARAMS]

    def check_served(self, shape, who='PixelDiscriminator'):
        """ValueError unless an input of `shape` (b, input_nc, H, W) is served"""
        if len(shape) != 4:
            raise ValueError(f'{who}: expected a (b, C, H, W) input, got {tuple(shape)}')
        b, C, H, W = shape
        if C != self.input_nc:
            raise ValueError(f'{who}: {C} input channels, built for input_nc = {self.input_nc}')
        if self.input_nc % 64 or self.input_nc < 64:
            raise ValueError(f'{who}: input_nc = {self.input_nc}; the generic convolution serves input_nc % 64 == 0')
        if self.ndf != 64 and (self.ndf % 128 or self.ndf < 128):
            raise ValueError(f'{who}: ndf = {self.ndf}; served are ndf = 64 and ndf % 128 == 0 (the generic convolution '
                             f'takes operands of 64 n channels, ndf / 2 is one)')
        ops.check_fada_classes(self.num_classes, who)
        if b < 1 or H < 1 or W < 1:
            raise ValueError(f'{who}: an empty input {tuple(shape)}')

    def operands(self):
        """The bf16 operand copies, rebuilt when a parameter has been written since they were made"""
        ps = self._params()
        versions = tuple((p._version, p.data_ptr()) for p in ps)
        if self._op is None or versions != self._op_versions:
            self._op, self._op_versions = PixelOperands(self), versions
        return self._op

    def forward(self, x):
        self.check_served(x.shape)
        if x.dtype != torch.float32:
            raise ValueError(f'PixelDiscriminator: f32 inputs, got {x.dtype}')
        if not x.is_cuda or not self.cls1.weight.is_cuda:
            raise RuntimeError('PixelDiscriminator runs on the GPU only (there is no CPU fallback)')
        return _PixelFn.apply(self, x, *self._params())
