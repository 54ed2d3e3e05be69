"""float64 restatement, in plain torch on the CPU, of the feature-space adversarial path: the pixel rows, the four layers
of PixelDiscriminator (regda/models/Discriminator.py:60-78), FADA's soft labels, the class-level loss and every gradient,
layer by layer -- and its "storage model", the same arithmetic with the operands and the stored activations / gradients
rounded to bf16 where the kernels store bf16 (csrc/fada_kernels.hip and the generic routes), including the second rounding
behind rgda_conv2d + rgda_disc_bias_lrelu, behind rgda_conv2d (mode 1) + rgda_lrelu_mask_rows and behind the residual add of
the convolution's epilogue.  Also the cases the GPU tests and derive_fada_tolerances.py share, drawn here so that both see
the same numbers.  Error measures, the tolerance rule (3 x the storage model's deviation + K * 2^-24) and the Adam helpers
are adv_ref's."""
import torch
import torch.nn.functional as F

from adv_ref import (F64, SLOPE, U32, adam_first_step_check, bf, err, mask_of, nchw, opposite, opposite_bound,  # noqa: F401
                     rel2, rows)

CP = 32
PARAMS = ('D.0.weight', 'D.0.bias', 'D.2.weight', 'D.2.bias', 'cls1.weight', 'cls1.bias', 'cls2.weight', 'cls2.bias')
T_DEFAULT, CLIP_DEFAULT = 1.8, 0.9


# ------------------------------------------------------------------------------------------------ pieces
def conv(x, w, b=None):
    return F.conv2d(x, w, b, stride=1, padding=1)


def conv_vjp(x, w, g):
    """(dx, dw, db) of conv(x, w, b) for the upstream gradient g"""
    x = x.clone().requires_grad_(True)
    w = w.clone().requires_grad_(True)
    dx, dw = torch.autograd.grad(conv(x, w), (x, w), g)
    return dx, dw, g.sum((0, 2, 3))


def soft_labels(x2, T=T_DEFAULT, clip=CLIP_DEFAULT):
    """a = min(softmax(x2 / T), clip) over the classes of x2 (n, C, h, w); no gradient"""
    return torch.softmax(x2.detach().to(F64) / T, 1).clamp(max=clip)


def loss_and_dz(z, a, side):
    """l(z, a, side) = -(1/M) sum_p sum_k a[p, k] log_softmax(z[p])[side nc + k] and dl/dz = (S softmax(z) - a') / M
    for z (n, 2 nc, h, w), a (n, nc, h, w)"""
    z, a = z.to(F64), a.to(F64)
    nc = a.shape[1]
    M = z.shape[0] * z.shape[2] * z.shape[3]
    logp = F.log_softmax(z, 1)
    placed = torch.zeros_like(z)
    placed[:, side * nc:(side + 1) * nc] = a
    loss = -(placed * logp).sum() / M
    return loss, (a.sum(1, keepdim=True) * logp.exp() - placed) / M


def params64(sd):
    return {k: sd[k].detach().cpu().to(F64) for k in PARAMS}


def heads(p):
    """cls1 and cls2 stacked, source half first: (weight (2 nc, ndf/2, 3, 3), bias (2 nc))"""
    return torch.cat((p['cls1.weight'], p['cls2.weight'])), torch.cat((p['cls1.bias'], p['cls2.bias']))


# ------------------------------------------------------------------------------------------------ the whole discriminator
def disc_forward(p, x, storage=False):
    """p: float64 parameters under the reference's names; x (b, input_nc, H, W).  -> (z (b, 2 nc, H, W), [x, a1, a2]).
    storage: x, the weights and every stored activation rounded to bf16; D.0 and D.2 round twice (rgda_conv2d stores its
    raw bf16 result, the epilogue pass rounds again); z stays f32 (the heads' bias is f32)."""
    r = bf if storage else (lambda t: t)
    acts = [r(x.to(F64))]
    for n in ('D.0', 'D.2'):
        raw = r(conv(acts[-1], r(p[n + '.weight'])))
        acts.append(r(F.leaky_relu(raw + p[n + '.bias'].view(1, -1, 1, 1), SLOPE)))
    wh, bh = heads(p)
    return conv(acts[2], r(wh), bh), acts


def disc_backward(p, acts, dz, storage=False, onto=None):
    """layer by layer, as the kernels run it: every stored gradient is the gradient of a PRE-activation (masked by the
    stored activation's sign).  dz (b, 2 nc, H, W) is stored as bf16 rows.  D.2's data gradient is rounded once where
    ndf / 2 == 32 (the head's kernel, mask fused) and twice otherwise (rgda_conv2d, then the mask pass); the input
    gradient is rounded once, and once more where it is added `onto` given rows (b, input_nc, H, W) in the convolution's
    epilogue.  -> (dx, {name: gradient})"""
    r = bf if storage else (lambda t: t)
    nc = p['cls1.weight'].shape[0]
    wh, _ = heads(p)
    dz = r(dz.to(F64))
    grads = {}
    g, dw, db = conv_vjp(acts[2], r(wh), dz)
    grads['cls1.weight'], grads['cls2.weight'], grads['cls1.bias'], grads['cls2.bias'] = dw[:nc], dw[nc:], db[:nc], db[nc:]
    g = r(g * mask_of(acts[2]))
    dx, grads['D.2.weight'], grads['D.2.bias'] = conv_vjp(acts[1], r(p['D.2.weight']), g)
    g = r(dx * mask_of(acts[1])) if g.shape[1] == CP else r(r(dx) * mask_of(acts[1]))
    dx, grads['D.0.weight'], grads['D.0.bias'] = conv_vjp(acts[0], r(p['D.0.weight']), g)
    dx = r(dx)
    if onto is not None:
        dx = r(dx + onto.to(F64))
    return dx, grads


def disc_loss_grads(p, x, x2, side, T=T_DEFAULT, clip=CLIP_DEFAULT, scale=1.0, storage=False, onto=None):
    """scale * l(D(x), soft_labels(x2), side) -> dict(z, loss, dz, dx, grads)"""
    z, acts = disc_forward(p, x, storage)
    loss, dz = loss_and_dz(z, soft_labels(x2, T, clip), side)
    dx, grads = disc_backward(p, acts, dz * scale, storage, onto)
    return dict(z=z, loss=loss * scale, dz=dz * scale, dx=dx, grads=grads)


def autograd_reference(sd, x, x2, side, T=T_DEFAULT, clip=CLIP_DEFAULT, dtype=F64, forward=None):
    """the reference's formulation (nn.Conv2d / LeakyReLU / torch.cat, autograd) in `dtype`, the loss formed on its
    output with torch ops; forward(x) -> z replaces the restated forward (the goldens pass the reference's own module)"""
    p = {k: sd[k].detach().to(dtype).clone().requires_grad_(True) for k in PARAMS}
    x = x.detach().to(dtype).clone().requires_grad_(True)
    if forward is None:
        a = F.leaky_relu(F.conv2d(x, p['D.0.weight'], p['D.0.bias'], padding=1), SLOPE)
        a = F.leaky_relu(F.conv2d(a, p['D.2.weight'], p['D.2.bias'], padding=1), SLOPE)
        z = torch.cat((F.conv2d(a, p['cls1.weight'], p['cls1.bias'], padding=1),
                       F.conv2d(a, p['cls2.weight'], p['cls2.bias'], padding=1)), 1)
    else:
        z = forward(x)
    a = torch.softmax(x2.detach().to(dtype) / T, 1).clamp(max=clip)
    nc = a.shape[1]
    loss = -(a * F.log_softmax(z, 1)[:, side * nc:(side + 1) * nc]).sum() / (z.shape[0] * z.shape[2] * z.shape[3])
    if forward is None:
        loss.backward()
        grads = {k: v.grad for k, v in p.items()}
    else:
        grads = None
    return dict(z=z.detach(), loss=loss.detach(), dx=x.grad, grads=grads, graph_loss=loss, x=x)


# ------------------------------------------------------------------------------------------------ shared cases
def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _bfr(*shape, gen, scale=1.0):
    return bf(torch.randn(*shape, generator=gen) * scale)


def _seed(base, name):
    return base + sum((i + 1) * ord(ch) for i, ch in enumerate(name))


SHAPES = {'1x1x1': (1, 1, 1), '1x5x7': (1, 5, 7), '2x8x8': (2, 8, 8), '3x3x33': (3, 3, 33)}
# (b, H, W): one pixel; 35 rows, no multiple of 32; 128 rows whose 32-pixel tiles cross an image boundary; 297 rows of a
# border-dominated map in three workgroups
CLASS_COUNTS = (1, 6, 7, 16)
HEAD_CHANNELS = (32, 256)        # ndf / 2
LOSS_SETTINGS = tuple((side, T, clip) for side in (0, 1) for T in (1.0, 1.8) for clip in (0.9, 1.0))

# pack / unpack: name -> (b, k, h, w, view): 'full', a channel slice [8:8+k] of a map with k + 24 channels, or a batch
# slice [1:1+b] of b + 2 images
PACK_CASES = {}
for _hw, (_h, _w) in {1: (1, 1), 35: (5, 7), 64: (8, 8), 70: (7, 10)}.items():
    for _k in (32, 2048):
        PACK_CASES['hw%d_k%d' % (_hw, _k)] = (2, _k, _h, _w, 'full')
PACK_CASES['channel_slice'] = (2, 32, 5, 7, 'channels')
PACK_CASES['batch_slice'] = (2, 32, 7, 10, 'batch')


def pack_case(name):
    """-> (base map f32, the view to pack)"""
    b, k, h, w, view = PACK_CASES[name]
    gen = _gen(_seed(100, name))
    if view == 'channels':
        base = torch.randn(b, k + 24, h, w, generator=gen)
        return base, (slice(None), slice(8, 8 + k))
    if view == 'batch':
        base = torch.randn(b + 2, k, h, w, generator=gen)
        return base, (slice(1, 1 + b),)
    return torch.randn(b, k, h, w, generator=gen), (slice(None),)


def head_case(shape, Ch, nc):
    """bf16-representable float64 operands of the heads: a2 (with exact zeros, negative zeros and negatives: it is also
    the activation the data gradient is masked by), the stacked weights (2 nc, Ch, 3, 3), bias f32, logits x2 (with +-80 in
    two pixels' classes), and dz (b, 2 nc, H, W) for the data gradient"""
    b, H, W = SHAPES[shape]
    gen = _gen(_seed(200, '%s_%d_%d' % (shape, Ch, nc)))
    a = _bfr(b, Ch, H, W, gen=gen)
    flat = a.view(-1)
    flat[0::7] = 0.0
    flat[3::11] = -0.0
    w = _bfr(2 * nc, Ch, 3, 3, gen=gen, scale=(9 * Ch) ** -0.5)
    bias = (torch.randn(2 * nc, generator=gen) * 0.1).float().to(F64)
    x2 = (torch.randn(b, nc, H, W, generator=gen) * 2).float()
    x2.view(-1)[0] = 80.0
    x2.view(-1)[-1] = -80.0
    dz = _bfr(b, 2 * nc, H, W, gen=gen)
    return dict(a=a, w=w, bias=bias, x2=x2, dz=dz, b=b, H=H, W=W, Ch=Ch, nc=nc)


def head_reference(c):
    z = conv(c['a'], c['w'], c['bias'])
    da, dw, db = conv_vjp(c['a'], c['w'], c['dz'])
    out = dict(z=z, da=da * mask_of(c['a']), dw=dw, db=db)
    for side, T, clip in LOSS_SETTINGS:
        out['loss', side, T, clip], out['dz', side, T, clip] = loss_and_dz(z, soft_labels(c['x2'], T, clip), side)
    return out


def head_tolerances(c, ref):
    """z: an f32 accumulation of K = 9 Ch exact products per element, nothing stored in bf16.  With dzabs = K 2^-24
    max(1, max|z|) the absolute error that leaves in z: log_softmax moves by at most 2 dzabs, so a pixel's term (S <= 1)
    by 2 dzabs and the mean by as much, plus M + 64 roundings of the f32 sums relative to the loss; softmax(z)_j moves by at
    most 2 dzabs p_j, and max|dl/dz| is at least about half the 1/M factor both carry, so relative to it a value of dz moves by 4
    dzabs, plus the exp / log / division roundings (64) and its bf16 store (the storage term).  da: 9 * 32 terms; dw and
    db: one term per pixel."""
    K = 9 * c['Ch']
    M = c['b'] * c['H'] * c['W']
    dzabs = K * U32 * max(1.0, float(ref['z'].abs().max()))
    t = dict(z=K * U32, da=3 * err(bf(ref['da']), ref['da']) + 9 * CP * U32, dw=(M + 8) * U32, db=(M + 8) * U32)
    for s in LOSS_SETTINGS:
        dz = ref[('dz',) + s]
        t['loss_%d_%g_%g' % s] = 2 * dzabs + (M + 64) * U32 * abs(float(ref[('loss',) + s]))
        t['dz_%d_%g_%g' % s] = 3 * err(bf(dz), dz) + 4 * dzabs + 64 * U32
    return t


def head_name(shape, Ch, nc):
    return '%s_ch%d_nc%d' % (shape, Ch, nc)


# the generic 3 x 3 routes on the new geometry: name -> (shape, Cin, Cout)
GENERIC_CASES = {'%s_ci%d' % (s, ci): (s, ci, 64) for s in SHAPES for ci in (64, 2048)}


def generic_case(name):
    """x (also the rows the accumulate test adds onto, and with zeros / negative zeros), w (OIHW), bias, g (the gradient of
    the layer's pre-activation)"""
    shape, Ci, Co = GENERIC_CASES[name]
    b, H, W = SHAPES[shape]
    gen = _gen(_seed(300, name))
    x = _bfr(b, Ci, H, W, gen=gen)
    x.view(-1)[0::7] = 0.0
    x.view(-1)[3::11] = -0.0
    w = _bfr(Co, Ci, 3, 3, gen=gen, scale=(9 * Ci) ** -0.5)
    bias = (torch.randn(Co, generator=gen) * 0.1).float().to(F64)
    g = _bfr(b, Co, H, W, gen=gen)
    return dict(x=x, w=w, bias=bias, g=g, b=b, H=H, W=W, Ci=Ci, Co=Co)


def generic_reference(c):
    y = F.leaky_relu(conv(c['x'], c['w'], c['bias']), SLOPE)
    dx, dw, db = conv_vjp(c['x'], c['w'], c['g'])
    return dict(y=y, dx=dx, dx_onto=dx + c['x'], dw=dw, db=db)


def generic_tolerances(c, ref):
    M = c['b'] * c['H'] * c['W']
    y_model = bf(F.leaky_relu(bf(conv(c['x'], c['w'])) + c['bias'].view(1, -1, 1, 1), SLOPE))
    return dict(y=3 * err(y_model, ref['y']) + 9 * c['Ci'] * U32,
                dx=3 * err(bf(ref['dx']), ref['dx']) + 9 * c['Co'] * U32,
                dx_onto=3 * err(bf(bf(ref['dx']) + c['x']), ref['dx_onto']) + 9 * c['Co'] * U32,
                dw=(M + 8) * U32, db=(M + 8) * U32)


# name -> (nc, b, H, W); input_nc = ndf = 64
MODULE_NC, MODULE_NDF = 64, 64
MODULE_CASES = {'nc%d_%dx%dx%d' % (nc, b, H, W): (nc, b, H, W) for nc in (1, 6, 7) for (b, H, W) in ((2, 8, 8), (1, 5, 7))}


def module_case(name):
    """weights drawn here (the reference's initialisation scale), features, logits for the soft labels"""
    nc, b, H, W = MODULE_CASES[name]
    gen = _gen(_seed(400, name))
    shapes = {'D.0': (MODULE_NDF, MODULE_NC), 'D.2': (MODULE_NDF // 2, MODULE_NDF), 'cls1': (nc, MODULE_NDF // 2),
              'cls2': (nc, MODULE_NDF // 2)}
    sd = {}
    for n, (co, ci) in shapes.items():
        k = (9 * ci) ** -0.5
        sd[n + '.weight'] = ((torch.rand(co, ci, 3, 3, generator=gen) * 2 - 1) * k * 3 ** 0.5).float()
        sd[n + '.bias'] = ((torch.rand(co, generator=gen) * 2 - 1) * k).float()
    x = torch.randn(b, MODULE_NC, H, W, generator=gen).float()
    x2 = (torch.randn(b, nc, H, W, generator=gen) * 2).float()
    return dict(sd=sd, x=x, x2=x2, nc=nc, b=b, H=H, W=W)


def module_reference(c, side, storage=False):
    return disc_loss_grads(params64(c['sd']), c['x'], c['x2'], side, storage=storage)


def module_floor():
    """K of the f32 floor: the longest accumulation of the chain, 9 * 64 terms"""
    return 9 * max(MODULE_NC, MODULE_NDF) * U32


def module_tolerances(c):
    """{side: {quantity: tolerance}}: z per element (err), the loss relative, dx and every parameter gradient by rel2, and
    per parameter the most elements that may move against the restatement in an Adam step (opposite_bound)"""
    floor = module_floor()
    out = {}
    for side in (0, 1):
        ref, sto = module_reference(c, side), module_reference(c, side, storage=True)
        t = dict(z=3 * err(sto['z'], ref['z']) + floor, dx=3 * rel2(sto['dx'], ref['dx']) + floor,
                 loss=3 * abs(float(sto['loss'] - ref['loss'])) / abs(float(ref['loss'])) + floor)
        for k in PARAMS:
            t[k] = 3 * rel2(sto['grads'][k], ref['grads'][k]) + floor
            t['opposite.' + k] = opposite_bound(sto['grads'][k], ref['grads'][k])
        out[str(side)] = t
    return out


# ------------------------------------------------------------------------------------------------ goldens (tests/golden/fada*.npz)
GOLDEN_CASES = tuple(MODULE_CASES)


def golden_part(name, side):
    return 'fada_%s_s%d.npz' % (name, side)


def golden_case(load, name):
    """one case of the fada*.npz fixtures as torch tensors: sd, x, x2, z, loss<s>, dx<s>, g<s> = {key: gradient}"""
    base = load('fada.npz')
    nc = MODULE_CASES[name][0]
    c = dict(sd={k: torch.from_numpy(base['nc%d_sd.%s' % (nc, k)]) for k in PARAMS}, z=torch.from_numpy(base[name + '_z']),
             x=torch.from_numpy(base[name + '_x']), x2=torch.from_numpy(base[name + '_x2']))
    for s in (0, 1):
        part = load(golden_part(name, s))
        c['loss%d' % s], c['dx%d' % s] = torch.from_numpy(part['loss']), torch.from_numpy(part['dx'])
        c['g%d' % s] = {k: torch.from_numpy(part['g.' + k]) for k in PARAMS}
    return c


def golden_tolerances(c):
    """{side: {quantity: bound}}: three times the deviation of the float32 evaluation from the float64 one on the golden's
    inputs; the single values (the loss, a one-class bias) add one f32 rounding, as in adv_ref"""
    out = {}
    for s in (0, 1):
        lo, hi = autograd_reference(c['sd'], c['x'], c['x2'], s, dtype=torch.float32), autograd_reference(c['sd'], c['x'], c['x2'], s)
        t = {q: 3 * err(lo[q], hi[q]) for q in ('z', 'loss', 'dx')}
        t.update({k: 3 * err(lo['grads'][k], hi['grads'][k]) + (U32 if hi['grads'][k].numel() == 1 else 0.0) for k in PARAMS})
        t['loss'] += U32
        out[str(s)] = t
    return out
