"""The three adversarial families: output-space FCDiscriminator layers and BCE (csrc/adv_kernels.hip), category-level
CLAN probabilities and weighted BCE (csrc/clan_kernels.hip), feature-space PixelDiscriminator heads and row packing
(csrc/fada_kernels.hip).  They share the probability-row format and the LeakyReLU slope, so they sit together."""
import torch

from .._lib import lib
from .base import _need_cuda, _p, _stream, _ws, check_class_count
from .feature import _feat_rows, _loss_out


ADV_CP = 16         # channels of a probability row: the classes zero-padded to one K slice of the bf16 MFMA
DISC_SLOPE = 0.2    # nn.LeakyReLU(negative_slope=0.2), regda/models/Discriminator.py:15


def _rows_bf16(t, cols, who):
    assert t.dtype == torch.bfloat16 and t.dim() == 2 and t.shape[1] == cols and t.is_contiguous(), (who, t.shape, t.dtype)
    return t


def adv_probs(x, size=None, softmax=True, out=None):
    """x f32 (b, C, h, w) on the GPU -> P bf16 [b*H*W, 16]: softmax over the classes of the bilinear (align_corners=True)
    upsample to size = (H, W), or with softmax=False the given probabilities packed as they are (size is x's own)."""
    _need_cuda(x, out)
    assert x.dim() == 4 and x.dtype == torch.float32 and x.is_contiguous(), 'adv_probs: contiguous f32 (b, C, h, w)'
    b, C, h, w = x.shape
    check_class_count(C, 'adv_probs')
    H, W = (h, w) if size is None else (int(size[0]), int(size[1]))
    if not softmax and (H, W) != (h, w):
        raise ValueError('adv_probs: given probabilities are packed at their own size')
    P = out if out is not None else torch.empty((b * H * W, ADV_CP), dtype=torch.bfloat16, device=x.device)
    _rows_bf16(P, ADV_CP, 'adv_probs')
    assert P.shape[0] == b * H * W
    lib().call('rgda_adv_probs_fwd', x.data_ptr(), P.data_ptr(), b, C, h, w, H, W, ADV_CP, 0 if softmax else 1, _stream())
    return P


def adv_probs_backward(dP, x, dx, size=None, softmax=True, scale=1.0):
    """dx f32 (b, C, h, w) += scale * (adv_probs' gradient of dP bf16 [b*H*W, 16]); x: the forward's input."""
    _need_cuda(dP, x, dx)
    assert dx.dim() == 4 and dx.dtype == torch.float32 and dx.is_contiguous() and x.shape == dx.shape
    assert x.dtype == torch.float32 and x.is_contiguous()
    b, C, h, w = dx.shape
    check_class_count(C, 'adv_probs_backward')
    H, W = (h, w) if size is None else (int(size[0]), int(size[1]))
    _rows_bf16(dP, ADV_CP, 'adv_probs_backward')
    assert dP.shape[0] == b * H * W
    lib().call('rgda_adv_probs_bwd', dP.data_ptr(), x.data_ptr(), dx.data_ptr(), b, C, h, w, H, W, ADV_CP,
               0 if softmax else 1, float(scale), _stream())
    return dx


def disc_conv(x, w, bias, N, H, W, slope=DISC_SLOPE, out=None):
    """One discriminator layer: x bf16 [N*H*W, Cin], w bf16 [Cout, 16, Cin], bias f32 [Cout] or None ->
    lrelu(conv 4x4 / stride 2 / pad 1 + bias) as bf16 [N*(H/2)*(W/2), Cout]."""
    _need_cuda(x, w, bias, out)
    Cout, taps, Cin = w.shape
    assert taps == 16 and w.dtype == torch.bfloat16 and w.is_contiguous()
    _rows_bf16(x, Cin, 'disc_conv')
    assert x.shape[0] == N * H * W and (bias is None or (bias.dtype == torch.float32 and bias.numel() == Cout and bias.is_contiguous()))
    y = out if out is not None else torch.empty((N * (H // 2) * (W // 2), Cout), dtype=torch.bfloat16, device=x.device)
    _rows_bf16(y, Cout, 'disc_conv')
    lib().call('rgda_disc_conv_fwd', x.data_ptr(), w.data_ptr(), _p(bias), y.data_ptr(), N, H, W, Cin, Cout, float(slope), _stream())
    return y


def disc_bias_lrelu(y, bias, slope=DISC_SLOPE):
    """y bf16 [M, C] = lrelu(y + bias) in place (the epilogue pass behind the generic convolution)."""
    _need_cuda(y, bias)
    M, C = y.shape
    _rows_bf16(y, C, 'disc_bias_lrelu')
    assert bias.dtype == torch.float32 and bias.numel() == C and bias.is_contiguous()
    lib().call('rgda_disc_bias_lrelu', y.data_ptr(), bias.data_ptr(), M, C, float(slope), _stream())
    return y


def disc_bias_grad(g):
    """g bf16 [M, C] -> f32 [C] column sums in a fixed order."""
    _need_cuda(g)
    M, C = g.shape
    _rows_bf16(g, C, 'disc_bias_grad')
    db = torch.empty(C, dtype=torch.float32, device=g.device)
    L = lib()
    ws = _ws(L.size('rgda_disc_bias_grad_workspace', M, C), g.device)
    L.call('rgda_disc_bias_grad', g.data_ptr(), M, C, db.data_ptr(), ws.data_ptr(), ws.numel(), _stream())
    return db


def disc_conv_backward(g, x, wt, N, H, W, below=True, need_dx=True, need_dparams=True, slope=DISC_SLOPE):
    """The gradients of disc_conv from g bf16 [N*(H/2)*(W/2), Cout], the gradient of the layer's PRE-activation.
    x bf16 [N*H*W, Cin]: the layer's input; wt bf16 [Cin, 16, Cout]: the transposed operand copy.
    -> (dx, dw, db): dx bf16 [N*H*W, Cin] masked by x's sign where `below` (x is a stored LeakyReLU output) -- the
    pre-activation gradient of the layer underneath; dw f32 [Cout, 16, Cin] (rgda_conv2d_wgrad_grouped) and db f32 [Cout]."""
    _need_cuda(g, x, wt)
    Cin, taps, Cout = wt.shape
    assert taps == 16 and wt.dtype == torch.bfloat16 and wt.is_contiguous()
    _rows_bf16(x, Cin, 'disc_conv_backward')
    _rows_bf16(g, Cout, 'disc_conv_backward')
    assert x.shape[0] == N * H * W and g.shape[0] == N * (H // 2) * (W // 2)
    dx = dw = db = None
    if need_dparams:
        dw = torch.zeros((Cout, 16, Cin), dtype=torch.float32, device=g.device)
        from .. import ops      # the convolution wrappers are reached through regda_amd.ops, where the benchmark patches them
        ops.conv2d_wgrad_grouped([(x, g, dw, N, H, W, H // 2, W // 2, 4, 4, 2, 1, 1)])
        db = disc_bias_grad(g)
    if need_dx:
        dx = torch.empty_like(x)
        lib().call('rgda_disc_conv_bwd_data', g.data_ptr(), wt.data_ptr(), x.data_ptr() if below else 0, dx.data_ptr(), N, H, W,
                   Cin, Cout, float(slope), _stream())
    return dx, dw, db


def disc_head(a4, w, bias, N, H, W):
    """The classifier: a4 bf16 [N*H*W, C], w f32 [16, C], bias f32 [1] -> z f32 [N, (H/2)*(W/2)]."""
    _need_cuda(a4, w, bias)
    C = w.shape[1]
    assert w.shape == (16, C) and w.dtype == torch.float32 and w.is_contiguous()
    _rows_bf16(a4, C, 'disc_head')
    assert a4.shape[0] == N * H * W
    z = torch.empty((N, (H // 2) * (W // 2)), dtype=torch.float32, device=a4.device)
    lib().call('rgda_disc_head_fwd', a4.data_ptr(), w.data_ptr(), _p(bias), z.data_ptr(), N, H, W, C, _stream())
    return z


def disc_head_backward(dz, a4, w, N, H, W, need_da=True, need_dparams=True, slope=DISC_SLOPE):
    """-> (da4 bf16 [N*H*W, C] masked by a4's sign, dw f32 [16, C], db f32 [1]) from dz f32 [N, (H/2)*(W/2)]."""
    _need_cuda(dz, a4, w)
    C = w.shape[1]
    _rows_bf16(a4, C, 'disc_head_backward')
    assert dz.dtype == torch.float32 and dz.is_contiguous() and dz.numel() == N * (H // 2) * (W // 2)
    da = torch.empty_like(a4) if need_da else None
    dw = torch.empty((16, C), dtype=torch.float32, device=a4.device) if need_dparams else None
    db = torch.empty(1, dtype=torch.float32, device=a4.device) if need_dparams else None
    lib().call('rgda_disc_head_bwd', dz.data_ptr(), a4.data_ptr(), w.data_ptr(), _p(da), _p(dw), _p(db), N, H, W, C,
               float(slope), _stream())
    return da, dw, db


def bce_logits(z, label, scale=1.0, loss=None, accumulate=False, want_grad=True):
    """scale * F.binary_cross_entropy_with_logits(z, full_like(z, label)) for label 0 or 1 -> (loss f32 [1] on the
    device, dz f32 of z's shape or None).  accumulate: added onto `loss`."""
    _need_cuda(z, loss)
    assert z.dtype == torch.float32 and z.is_contiguous()
    if float(label) not in (0.0, 1.0):
        raise ValueError('bce_logits: the label is 0 or 1, got %r' % (label,))
    if loss is None:
        assert not accumulate
        loss = torch.empty(1, dtype=torch.float32, device=z.device)
    dz = torch.empty_like(z) if want_grad else None
    lib().call('rgda_bce_logits', z.data_ptr(), z.numel(), float(label), float(scale), loss.data_ptr(), int(bool(accumulate)),
               _p(dz), _stream())
    return loss, dz


def _pair_logits(x1, x2, who):
    _need_cuda(x1, x2)
    assert x1.dim() == 4 and x1.dtype == torch.float32 and x1.is_contiguous(), who + ': contiguous f32 (b, C, h, w)'
    assert x2.shape == x1.shape and x2.dtype == torch.float32 and x2.is_contiguous(), who + ': x2 as x1'
    check_class_count(x1.shape[1], who)
    return x1.shape


def clan_probs(x1, x2, size=None):
    """The two heads' logits x1, x2 f32 (b, C, h, w) -> (P bf16 [b*H*W, 16] = softmax(up x1 + up x2), what the
    discriminator reads, and wmap f32 (b, H, W) = 1 - cos(softmax(up x1), softmax(up x2))); `up`: bilinear,
    align_corners=True, to size = (H, W)."""
    b, C, h, w = _pair_logits(x1, x2, 'clan_probs')
    H, W = (h, w) if size is None else (int(size[0]), int(size[1]))
    P = torch.empty((b * H * W, ADV_CP), dtype=torch.bfloat16, device=x1.device)
    wmap = torch.empty((b, H, W), dtype=torch.float32, device=x1.device)
    lib().call('rgda_clan_probs_fwd', x1.data_ptr(), x2.data_ptr(), P.data_ptr(), wmap.data_ptr(), b, C, h, w, H, W, ADV_CP,
               _stream())
    return P, wmap


def clan_probs_backward(dP, gw, x1, x2, dx1, dx2, size=None, scale=1.0):
    """dx1, dx2 f32 (b, C, h, w) += scale * (clan_probs' gradient of dP bf16 [b*H*W, 16] and of gw f32 (b, H, W), the
    gradient with respect to wmap; gw None: the weight map is a constant); x1, x2: the forward's inputs."""
    b, C, h, w = _pair_logits(x1, x2, 'clan_probs_backward')
    _need_cuda(dP, gw, dx1, dx2)
    for dx in (dx1, dx2):
        assert dx.shape == x1.shape and dx.dtype == torch.float32 and dx.is_contiguous()
    H, W = (h, w) if size is None else (int(size[0]), int(size[1]))
    _rows_bf16(dP, ADV_CP, 'clan_probs_backward')
    assert dP.shape[0] == b * H * W
    assert gw is None or (gw.dtype == torch.float32 and gw.is_contiguous() and gw.numel() == b * H * W)
    lib().call('rgda_clan_probs_bwd', dP.data_ptr(), _p(gw), x1.data_ptr(), x2.data_ptr(), dx1.data_ptr(), dx2.data_ptr(), b, C,
               h, w, H, W, ADV_CP, float(scale), _stream())
    return dx1, dx2


def wbce_logits(z, size, target, wmap=None, alpha=1.0, beta=0.0, scale=1.0, mean=True, loss=None, accumulate=False,
                want_dz=True, want_gw=False):
    """WeightedBCEWithLogitsLoss (regda/loss.py:60-85) on z f32 (b, hz, wz) upsampled (bilinear, align_corners=True) to
    size = (H, W): scale * mean-or-sum over the pixels of (alpha + beta * wmap) * BCE(up z, target); wmap f32 (b, H, W) or
    None for the plain loss; target a tensor f32 (b, H, W) or the constant label 0 / 1.
    -> (loss f32 [1] on the device, dz f32 of z's shape or None, gw f32 (b, H, W), the gradient for wmap, or None)."""
    _need_cuda(z, wmap, loss)
    assert z.dim() == 3 and z.dtype == torch.float32 and z.is_contiguous(), 'wbce_logits: contiguous f32 (b, hz, wz)'
    b, hz, wz = z.shape
    H, W = int(size[0]), int(size[1])
    label = 0.0
    if isinstance(target, torch.Tensor):
        _need_cuda(target)
        assert target.dtype == torch.float32 and target.is_contiguous() and target.numel() == b * H * W
    else:
        if float(target) not in (0.0, 1.0):
            raise ValueError('wbce_logits: a constant label is 0 or 1, got %r' % (target,))
        label, target = float(target), None
    assert wmap is None or (wmap.dtype == torch.float32 and wmap.is_contiguous() and wmap.numel() == b * H * W)
    if want_gw and wmap is None:
        raise ValueError('wbce_logits: no weight map, no gradient with respect to it')
    if loss is None:
        assert not accumulate
        loss = torch.empty(1, dtype=torch.float32, device=z.device)
    dz = torch.empty_like(z) if want_dz else None
    gw = torch.empty((b, H, W), dtype=torch.float32, device=z.device) if want_gw else None
    L = lib()
    nbytes = L.size('rgda_wbce_logits_workspace', b, H, W)
    if not nbytes:
        raise ValueError(f'wbce_logits: {b} x {H} x {W} pixels are not served')
    ws = _ws(nbytes, z.device)
    L.call('rgda_wbce_logits', z.data_ptr(), b, hz, wz, H, W, _p(target), label, _p(wmap), float(alpha), float(beta),
           float(scale), int(bool(mean)), loss.data_ptr(), int(bool(accumulate)), _p(dz), _p(gw), ws.data_ptr(), ws.numel(),
           _stream())
    return loss, dz, gw


FADA_CP = 32            # columns of a head row of PixelDiscriminator: 2 * num_classes <= 32
FADA_MAX_CLASSES = 16


def check_fada_classes(nc, who='num_classes'):
    """ValueError unless 1 <= nc <= FADA_MAX_CLASSES (the two heads share one 32-column tile)."""
    if not 1 <= int(nc) <= FADA_MAX_CLASSES:
        raise ValueError(f'{who}: {nc} classes; the head kernel serves 1 <= num_classes <= {FADA_MAX_CLASSES}')


def feat_pack_rows(x, out=None):
    """x f32 (b, k, h, w) on the GPU (read in place through its channel and image strides where the pixels of an image
    are contiguous) -> bf16 rows [b*h*w, ld] with columns 0 .. k-1 written; `out` gives a wider, caller-filled buffer."""
    if x.dim() != 4 or x.dtype != torch.float32:
        raise ValueError(f'feat_pack_rows: f32 (b, k, h, w) features, got {x.dtype} {tuple(x.shape)}')
    _need_cuda(x, out)
    x, b, hw, ldc, ldb, k = _feat_rows(x, 'feat_pack_rows')
    if out is None:
        if k % 8:
            raise ValueError(f'feat_pack_rows: {k} channels; dense rows need k % 8 == 0 (or a wider `out`)')
        out = torch.empty((b * hw, k), dtype=torch.bfloat16, device=x.device)
    _rows_bf16(out, out.shape[1], 'feat_pack_rows')
    assert out.shape[0] == b * hw and out.shape[1] >= k
    lib().call('rgda_feat_pack_rows', x.data_ptr(), b, hw, ldc, ldb, k, out.data_ptr(), out.shape[1], _stream())
    return out


def feat_unpack_rows(rows, dx, scale=1.0, accumulate=False):
    """dx f32 (b, k, h, w) (a strided view as in feat_pack_rows) = (accumulate ? dx : 0) + scale * rows[:, :k]"""
    _need_cuda(rows, dx)
    assert dx.dim() == 4 and dx.dtype == torch.float32
    b, k, h, w = dx.shape
    ldb, ldc = dx.stride(0), dx.stride(1)
    assert (w == 1 or dx.stride(3) == 1) and (h == 1 or dx.stride(2) == w) and ldc >= h * w and (b == 1 or ldb >= ldc * k), \
        'feat_unpack_rows: the pixels of one image must be contiguous'
    _rows_bf16(rows, rows.shape[1], 'feat_unpack_rows')
    assert rows.shape[0] == b * h * w and rows.shape[1] >= k
    lib().call('rgda_feat_unpack_rows', rows.data_ptr(), rows.shape[1], dx.data_ptr(), b, h * w, ldc, ldb, k, float(scale),
               int(bool(accumulate)), _stream())
    return dx


def _fada_head_operands(a2, wh, bias, N, H, W, who):
    _need_cuda(a2, wh, bias)
    rows, taps, Ch = wh.shape
    assert rows == FADA_CP and taps == 9 and wh.dtype == torch.bfloat16 and wh.is_contiguous(), who
    assert bias.dtype == torch.float32 and bias.numel() == FADA_CP and bias.is_contiguous(), who
    _rows_bf16(a2, Ch, who)
    assert a2.shape[0] == N * H * W
    return Ch


def fada_head(a2, wh, bias, N, H, W, nc):
    """The two heads of PixelDiscriminator: a2 bf16 [N*H*W, Ch], wh bf16 [32, 9, Ch], bias f32 [32] -> z f32 [N*H*W, 32]
    (columns 0 .. 2 nc - 1 live)."""
    check_fada_classes(nc, 'fada_head')
    Ch = _fada_head_operands(a2, wh, bias, N, H, W, 'fada_head')
    z = torch.empty((N * H * W, FADA_CP), dtype=torch.float32, device=a2.device)
    lib().call('rgda_fada_head', a2.data_ptr(), wh.data_ptr(), bias.data_ptr(), N, H, W, Ch, int(nc), z.data_ptr(), 0, 0, 1.0,
               1.0, 0.0, 0, 0, 0, 0, _stream())
    return z


def fada_loss(a2, wh, bias, x2, side, temperature=1.8, clip=0.9, scale=1.0, loss=None, want_z=False):
    """The fused head + loss: with z = head(a2), a = min(softmax(x2 / temperature), clip) (x2 f32 (N, nc, H, W) logits, no
    gradient) and M = N*H*W, loss (f32 [1], accumulating) += scale * l(z, a, side) and dz bf16 [M, 32] = scale * dl/dz.
    -> (loss, dz, z or None)."""
    if x2.dim() != 4 or x2.dtype != torch.float32:
        raise ValueError(f'fada_loss: f32 (N, nc, H, W) logits, got {x2.dtype} {tuple(x2.shape)}')
    N, nc, H, W = x2.shape
    check_fada_classes(nc, 'fada_loss')
    if side not in (0, 1):
        raise ValueError(f'fada_loss: side is 0 (source) or 1 (target), got {side!r}')
    if not temperature > 0 or not clip > 0:
        raise ValueError(f'fada_loss: temperature and clip must be positive, got {temperature!r} and {clip!r}')
    _need_cuda(x2, loss)
    Ch = _fada_head_operands(a2, wh, bias, N, H, W, 'fada_loss')
    x2 = x2.contiguous()
    loss = _loss_out(loss, a2.device)
    M = N * H * W
    dz = torch.empty((M, FADA_CP), dtype=torch.bfloat16, device=a2.device)
    z = torch.empty((M, FADA_CP), dtype=torch.float32, device=a2.device) if want_z else None
    L = lib()
    ws = _ws(L.size('rgda_fada_head_workspace', M), a2.device)
    L.call('rgda_fada_head', a2.data_ptr(), wh.data_ptr(), bias.data_ptr(), N, H, W, Ch, nc, _p(z), x2.data_ptr(), int(side),
           float(temperature), float(clip), float(scale), loss.data_ptr(), dz.data_ptr(), ws.data_ptr(), ws.numel(), _stream())
    return loss, dz, z


def fada_head_backward_data(dz, wt, below, N, H, W, slope=DISC_SLOPE):
    """da bf16 [N*H*W, Ch] from dz bf16 [N*H*W, 32] and wt bf16 [Ch, 9, 32], masked by the sign of `below` bf16 [N*H*W, Ch],
    the stored activation."""
    _need_cuda(dz, wt, below)
    Ch, taps, cp = wt.shape
    assert taps == 9 and cp == FADA_CP and wt.dtype == torch.bfloat16 and wt.is_contiguous()
    _rows_bf16(dz, FADA_CP, 'fada_head_backward_data')
    assert dz.shape[0] == N * H * W
    _rows_bf16(below, Ch, 'fada_head_backward_data')
    assert below.shape[0] == N * H * W
    da = torch.empty((N * H * W, Ch), dtype=torch.bfloat16, device=dz.device)
    lib().call('rgda_fada_head_bwd_data', dz.data_ptr(), wt.data_ptr(), below.data_ptr(), da.data_ptr(), N, H, W, Ch, float(slope),
               _stream())
    return da


def lrelu_mask_rows(g, a, slope=DISC_SLOPE):
    """g bf16 [M, C] *= (a > 0 ? 1 : slope) in place (a: the stored activation, same shape)"""
    _need_cuda(g, a)
    M, C = g.shape
    _rows_bf16(g, C, 'lrelu_mask_rows')
    _rows_bf16(a, C, 'lrelu_mask_rows')
    assert a.shape[0] == M
    lib().call('rgda_lrelu_mask_rows', g.data_ptr(), a.data_ptr(), M, C, float(slope), _stream())
    return g
