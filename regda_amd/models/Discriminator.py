"""FCDiscriminator -- mirror of regda/models/Discriminator.py:4-28 (AdaptSegNet's output-space discriminator, Tsai et
al. 2018) on the kernels of csrc/adv_kernels.hip.

Same constructor, the reference's parameter names and OIHW layout (`conv1..conv4.weight/bias`, `classifier.weight/bias`,
f32), so `state_dict()` round-trips with a reference checkpoint and a caller's `torch.optim` sees ordinary `.grad`s.  The
forward packs the input as bf16 pixel rows (16 channels), runs the first layer on `rgda_disc_conv_fwd` (4 x 4, stride 2, bias and
LeakyReLU(0.2) in the epilogue), the layers with Cin % 64 == 0 (2-4 at ndf = 64) on the generic `rgda_conv2d` followed by `rgda_disc_bias_lrelu`
(measured faster) and the one-channel head (`rgda_disc_head_fwd`); the backward is one
`torch.autograd.Function` over `rgda_disc_head_bwd`, the parity data gradient `rgda_disc_conv_bwd_data`, the generic
deterministic weight gradient and the fixed-order bias sums.  The bf16 operand copies of the weights (both orientations)
are rebuilt when a parameter's `_version` has moved, e.g. after an optimizer step.

Served: f32 inputs on the GPU, 6 <= num_classes <= 16, H % 32 == 0 and W % 32 == 0, ndf % 32 == 0; anything else raises
with the cause.  Not provided: FCDiscriminator_Local (a 2048 + C channel input; CLAN's upsampled-output role is served by
this class and rgda_wbce_logits' fused upsample, regda_amd/gast/clan.py).  PixelDiscriminator lives in its own module,
regda_amd/models/PixelDiscriminator.py.
"""
import torch
import torch.nn as nn

from .. import ops

LAYERS = ('conv1', 'conv2', 'conv3', 'conv4')


class DiscOperands:
    """The kernels' view of a discriminator's parameters: per layer wf bf16 [Cout, 16, Cin'] (tap = kh * 4 + kw, the first
    layer's Cin = ci[0] zero-padded to 16), wt bf16 [Cin', 16, Cout] (rgda_weight_transpose_bf16) and the f32 bias; the head's
    f32 [16, C] weight and bias."""

    def __init__(self, module):
        self.wf, self.wt, self.bias, self.ci = [], [], [], []
        for name in LAYERS:
            conv = getattr(module, name)
            w = conv.weight.detach()
            Co, Ci = w.shape[:2]
            Cp = ops.ADV_CP if name == 'conv1' else Ci
            w32 = torch.zeros((Co, 16, Cp), dtype=torch.float32, device=w.device)
            w32[:, :, :Ci] = w.permute(0, 2, 3, 1).reshape(Co, 16, Ci)
            wt = torch.empty((Cp, 16, Co), dtype=torch.bfloat16, device=w.device)
            ops.weight_transpose_bf16(w32, wt, Co, 16, Cp)
            self.wf.append(w32.to(torch.bfloat16))
            self.wt.append(wt)
            self.bias.append(conv.bias.detach().contiguous())
            self.ci.append(Ci)
        hw = module.classifier.weight.detach()
        self.wh = hw.permute(0, 2, 3, 1).reshape(16, hw.shape[1]).contiguous()
        self.bh = module.classifier.bias.detach().contiguous()


def forward_rows(op, P, b, H, W):
    """P bf16 [b*H*W, 16] -> (z f32 [b, H/32 * W/32], [P, a1, a2, a3, a4])"""
    acts, h, w = [P], H, W
    for i in range(4):
        if op.wf[i].shape[2] % 64:      # 16 (the first layer) or 32 input channels: the specialised kernel, bias and
            acts.append(ops.disc_conv(acts[-1], op.wf[i], op.bias[i], b, h, w))       # LeakyReLU in its epilogue
        else:           # Cin % 64 == 0, what rgda_conv2d serves: measured faster (scripts/dev/adv_bench.py) as the generic
            #             implicit GEMM and one epilogue pass
            y = torch.empty((b * (h // 2) * (w // 2), op.wf[i].shape[0]), dtype=torch.bfloat16, device=P.device)
            ops.conv2d(acts[-1], op.wf[i], y, b, h, w, h // 2, w // 2, 4, 4, 2, 1, 1)
            acts.append(ops.disc_bias_lrelu(y, op.bias[i]))
        h, w = h // 2, w // 2
    return ops.disc_head(acts[4], op.wh, op.bh, b, h, w), acts


def backward_rows(op, dz, acts, b, H, W, need_dparams=True, need_dinput=True):
    """dz f32 [b, H/32 * W/32] -> (dP bf16 [b*H*W, 16], grads): grads maps the reference's parameter names to OIHW f32
    gradients (empty without need_dparams); dP is None without need_dinput."""
    h, w = H // 16, W // 16
    g, dwh, dbh = ops.disc_head_backward(dz, acts[4], op.wh, b, h, w, True, need_dparams)
    grads = {}
    if need_dparams:
        C = dwh.shape[1]
        grads['classifier.weight'] = dwh.view(4, 4, C).permute(2, 0, 1).unsqueeze(0).contiguous()
        grads['classifier.bias'] = dbh
    for i in (3, 2, 1, 0):
        h, w = h * 2, w * 2                    # the size of layer i's input
        g, dw, db = ops.disc_conv_backward(g, acts[i], op.wt[i], b, h, w, below=i > 0, need_dx=i > 0 or need_dinput,
                                           need_dparams=need_dparams)
        if need_dparams:
            Co, _, Cp = dw.shape
            grads[LAYERS[i] + '.weight'] = dw.view(Co, 4, 4, Cp)[..., :op.ci[i]].permute(0, 3, 1, 2).contiguous()
            grads[LAYERS[i] + '.bias'] = db
    return g, grads


class _DiscFn(torch.autograd.Function):
    """z = D(x) for given probabilities x; gradients for x and the ten parameters"""

    @staticmethod
    def forward(ctx, module, x, *params):
        op = module.operands()
        b, C, H, W = x.shape
        P = ops.adv_probs(x, softmax=False)
        z, acts = forward_rows(op, P, b, H, W)
        ctx.op, ctx.acts, ctx.shape = op, acts, (b, C, H, W)
        return z.view(b, 1, H // 32, W // 32)

    @staticmethod
    def backward(ctx, gz):
        b, C, H, W = ctx.shape
        need_dp = any(ctx.needs_input_grad[2:])
        dP, grads = backward_rows(ctx.op, gz.contiguous().float().view(b, -1), ctx.acts, b, H, W, need_dp,
                                   need_dinput=ctx.needs_input_grad[1])
        dx = None
        if ctx.needs_input_grad[1]:
            dx = torch.zeros((b, C, H, W), dtype=torch.float32, device=dP.device)
            ops.adv_probs_backward(dP, dx, dx, softmax=False)
        out = [grads.get(k) if need else None for k, need in zip(FCDiscriminator.PARAMS, ctx.needs_input_grad[2:])]
        return (None, dx, *out)


class FCDiscriminator(nn.Module):
    PARAMS = tuple(n + s for n in LAYERS + ('classifier',) for s in ('.weight', '.bias'))

    def __init__(self, num_classes, ndf=64):
        super().__init__()
        # nn.Conv2d holds the parameters under the reference's names with the reference's initialisation; the convolutions
        # themselves run in forward() below
        self.conv1 = nn.Conv2d(num_classes, ndf, kernel_size=4, stride=2, padding=1)
        self.conv2 = nn.Conv2d(ndf, ndf * 2, kernel_size=4, stride=2, padding=1)
        self.conv3 = nn.Conv2d(ndf * 2, ndf * 4, kernel_size=4, stride=2, padding=1)
        self.conv4 = nn.Conv2d(ndf * 4, ndf * 8, kernel_size=4, stride=2, padding=1)
        self.classifier = nn.Conv2d(ndf * 8, 1, kernel_size=4, stride=2, padding=1)
        self.leaky_relu = nn.LeakyReLU(negative_slope=ops.DISC_SLOPE, inplace=True)
        self.num_classes, self.ndf = num_classes, ndf
        self._op, self._op_versions = None, None

    def _params(self):
        return [self.get_parameter(k) for k in self.PARAMS]

    def check_served(self, shape, who='FCDiscriminator'):
        """ValueError unless an input of `shape` (b, C, H, W) is served"""
        if len(shape) != 4:
            raise ValueError(f'{who}: expected a (b, C, H, W) input, got {tuple(shape)}')
        b, C, H, W = shape
        if C != self.num_classes:
            raise ValueError(f'{who}: {C} input channels, built for {self.num_classes} classes')
        ops.check_class_count(C, who)
        if self.ndf % 32 or self.ndf < 32:
            raise ValueError(f'{who}: ndf = {self.ndf}; the convolution kernels serve ndf % 32 == 0')
        if H % 32 or W % 32 or H < 32 or W < 32:
            raise ValueError(f'{who}: a {H} x {W} input; five stride-2 layers serve H % 32 == 0 and W % 32 == 0')

    def operands(self):
        """The bf16 operand copies, rebuilt when a parameter has been written since they were made"""
        ps = self._params()
        versions = tuple((p._version, p.data_ptr()) for p in ps)
        if self._op is None or versions != self._op_versions:
            self._op, self._op_versions = DiscOperands(self), versions
        return self._op

    def forward(self, x):
        self.check_served(x.shape)
        if x.dtype != torch.float32:
            raise ValueError(f'FCDiscriminator: f32 inputs, got {x.dtype}')
        if not x.is_cuda or not self.conv1.weight.is_cuda:
            raise RuntimeError('FCDiscriminator runs on the GPU only (there is no CPU fallback)')
        return _DiscFn.apply(self, x.contiguous(), *self._params())
