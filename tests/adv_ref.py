"""float64 restatement, in plain torch on the CPU, of the adversarial path: the probability rows, the five layers of
FCDiscriminator (regda/models/Discriminator.py:4-28), BCE against a constant label and every gradient -- and its "storage
model", the same arithmetic with the operands and the stored activations / gradients rounded to bf16 where the kernels
store bf16 (csrc/adv_kernels.hip).  Also the cases the GPU tests and derive_adv_tolerances.py share, drawn here so that
both see the same numbers.

Error measures (one per tensor):
    err(a, b)  = max |a - b| / max |b|          "per element": every element within a bound scaled by the tensor's largest
    rel2(a, b) = |a - b|_2 / |b|_2              the relative L2 norm (whole-module gradients)
A tolerance is 3 x (the storage model's deviation from float64 on the same inputs) + K * 2^-24, K the length of the
longest f32 accumulation behind one element: the storage model knows nothing of f32 rounding, whose worst case grows
linearly with the number of terms (its random-walk expectation, sqrt(K) * 2^-24, lies well below)."""
import torch
import torch.nn.functional as F

F64 = torch.float64
SLOPE = 0.2
CP = 16
LAYERS = ('conv1', 'conv2', 'conv3', 'conv4')
PARAMS = tuple(n + s for n in LAYERS + ('classifier',) for s in ('.weight', '.bias'))
U32 = 2.0 ** -24


def bf(t):
    """round to bf16 (nearest even), back in float64"""
    return t.to(torch.float32).to(torch.bfloat16).to(F64)


def err(a, b):
    a, b = a.to(F64), b.to(F64)
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))


def rel2(a, b):
    a, b = a.to(F64), b.to(F64)
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


def rows(x):
    """(N, C, H, W) -> pixel-major [N*H*W, C]"""
    return x.permute(0, 2, 3, 1).reshape(-1, x.shape[1]).contiguous()


def nchw(r, N, H, W):
    return r.reshape(N, H, W, r.shape[1]).permute(0, 3, 1, 2).contiguous()


def mask_of(a):
    """the LeakyReLU derivative read from a stored post-activation: a > 0 ? 1 : slope (torch's convention at 0)"""
    return torch.where(a > 0, torch.ones_like(a), torch.full_like(a, SLOPE))


# ------------------------------------------------------------------------------------------------ pieces
def probs(x, size=None, softmax=True):
    """x (b, C, h, w) -> probabilities (b, C, H, W) in float64"""
    x = x.to(F64)
    if not softmax:
        return x
    if size is not None and tuple(size) != tuple(x.shape[-2:]):
        x = F.interpolate(x, size=tuple(size), mode='bilinear', align_corners=True)
    return F.softmax(x, dim=1)


def probs_backward(x, dP, size=None, softmax=True):
    """the gradient of probs() with respect to x for the upstream gradient dP (b, C, H, W)"""
    x = x.to(F64).clone().requires_grad_(True)
    probs(x, size, softmax).backward(dP.to(F64))
    return x.grad


def conv(x, w, b=None):
    return F.conv2d(x, w, b, stride=2, padding=1)


def layer(x, w, b):
    return F.leaky_relu(conv(x, w, b), SLOPE)


def conv_vjp(x, w, g):
    """(dx, dw, db) of conv(x, w, b) for the upstream gradient g"""
    x = x.clone().requires_grad_(True)
    w = w.clone().requires_grad_(True)
    dx, dw = torch.autograd.grad(conv(x, w), (x, w), g)
    return dx, dw, g.sum((0, 2, 3))


def bce(z, t):
    """mean(softplus(z) - t z) and its gradient"""
    z = z.to(F64)
    return (F.softplus(z) - t * z).mean(), (torch.sigmoid(z) - t) / z.numel()


def pad_classes(p):
    """(b, C, H, W) -> (b, 16, H, W) with zero channels"""
    return F.pad(p, (0, 0, 0, 0, 0, CP - p.shape[1]))


# ------------------------------------------------------------------------------------------------ the whole discriminator
def params64(sd):
    return {k: sd[k].detach().cpu().to(F64) for k in PARAMS}


def disc_forward(p, x, storage=False):
    """p: float64 parameters under the reference's names; x: probabilities (b, C, H, W).  -> (z (b, 1, H/32, W/32),
    [a0 .. a4]) with a0 = x.  storage: conv weights, x and every stored activation rounded to bf16; the head's weights
    stay f32 as in the kernels."""
    r = bf if storage else (lambda t: t)
    acts = [r(x.to(F64))]
    for n in LAYERS:
        if p[n + '.weight'].shape[1] % 64:      # rgda_disc_conv_fwd, bias and LeakyReLU in its epilogue: one rounding
            acts.append(r(layer(acts[-1], r(p[n + '.weight']), p[n + '.bias'])))
        else:                   # Cin % 64 == 0: rgda_conv2d stores its raw bf16 result, the epilogue pass rounds again
            raw = r(conv(acts[-1], r(p[n + '.weight'])))
            acts.append(r(F.leaky_relu(raw + p[n + '.bias'].view(1, -1, 1, 1), SLOPE)))
    return conv(acts[4], p['classifier.weight'], p['classifier.bias']), acts


def disc_backward(p, acts, dz, storage=False):
    """layer by layer, as the kernels run it: every stored gradient is the gradient of a PRE-activation (masked by the
    stored activation's sign).  -> (dx, {name: gradient})"""
    r = bf if storage else (lambda t: t)
    grads = {}
    g, grads['classifier.weight'], grads['classifier.bias'] = conv_vjp(acts[4], p['classifier.weight'], dz.to(F64))
    g = r(g * mask_of(acts[4]))
    for i in (3, 2, 1, 0):
        dx, grads[LAYERS[i] + '.weight'], grads[LAYERS[i] + '.bias'] = conv_vjp(acts[i], r(p[LAYERS[i] + '.weight']), g)
        g = r(dx * mask_of(acts[i]) if i > 0 else dx)
    return g, grads


def disc_loss_grads(p, x, label, storage=False, scale=1.0):
    """BCE(D(x), label) * scale -> dict(z, loss, dx, grads)"""
    z, acts = disc_forward(p, x, storage)
    loss, dz = bce(z, label)
    dx, grads = disc_backward(p, acts, dz * scale, storage)
    return dict(z=z, loss=loss * scale, dx=dx, grads=grads)


def adam_first_step_check(before, after, g, lr=1e-4, eps=1e-8):
    """One torch.optim.Adam step from zero state moves an element by -lr g / (|g| + eps).  True where `after - before` is
    that movement for the gradient g in every element, within 2^-22 |p| (the f32 parameter update) and lr 2^-20 (Adam's
    own f32 arithmetic).  With g the module's own .grad this says the gradient sits where the optimizer reads it."""
    g = g.detach().cpu().to(F64)
    p0 = before.detach().cpu().to(F64).reshape(g.shape)
    got = after.detach().cpu().to(F64).reshape(g.shape) - p0
    want = -lr * g / (g.abs() + eps)
    return bool(((got - want).abs() <= 2.0 ** -22 * p0.abs() + lr * 2.0 ** -20).all())


def opposite(a, b):
    """the number of elements in which a and b have opposite signs"""
    return int((a.detach().cpu().to(F64).reshape(b.shape) * b.to(F64) < 0).sum())


def opposite_bound(g_model, g_ref):
    """Adam's first step has size lr whatever the size of the gradient, so `the parameters move as the restatement's`
    means: in the restatement's direction, element by element, and a norm of the movement says nothing.  An element
    whose gradient the bf16 rounding points push across zero moves the other way, legitimately; the kernels share the
    storage model's rounding points, so the number of such elements is a count of the same expectation as the model's
    own.  The bound is three times (the model's count + 1): the + 1 is the Laplace estimate of a count that may be
    observed as 0 (one flipped element of 512 next to a model count of 0 is no error).  A single value has no such
    population: its relative bound is far below 1, so its sign must agree."""
    return 0 if g_ref.numel() == 1 else 3 * (opposite(g_model, g_ref) + 1)


# ------------------------------------------------------------------------------------------------ shared cases
def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _bfr(*shape, gen, scale=1.0):
    return bf(torch.randn(*shape, generator=gen) * scale)


# name -> (N, H, W of the layer's input, Cin, Cout)
CONV_CASES = {
    'pixel': (1, 2, 2, 64, 64),         # one output pixel: every tap row and column but the middle 2 x 2 lies in the padding
    'ragged': (3, 6, 10, 64, 128),      # odd batch, 45 output pixels: a ragged 64-pixel tile
    'fullk': (2, 32, 32, 256, 512),     # K = 4096, several workgroups
    'first': (1, 64, 64, CP, 64),       # the first layer: one tap = one K slice
    'narrow': (2, 6, 6, 32, 32),        # ndf = 32's second layer shape class: 32 input channels (rgda_conv2d refuses them) and
    #                                     32-wide channel tiles in both kernels
    'first32': (1, 8, 8, CP, 32),       # ndf = 32's first layer: one tap = one K slice, a 32-wide channel tile
}


def conv_case(name):
    """bf16-representable float64 inputs: x (with exact zeros, negative zeros and negatives: it is also the activation the
    data gradient is masked by), w (OIHW), bias f32, g (the gradient of the layer's pre-activation)"""
    N, H, W, Ci, Co = CONV_CASES[name]
    gen = _gen(1000 + sum(map(ord, name)))
    x = _bfr(N, Ci, H, W, gen=gen)
    flat = x.view(-1)
    flat[0::7] = 0.0
    flat[3::11] = -0.0
    w = _bfr(Co, Ci, 4, 4, gen=gen, scale=(16 * Ci) ** -0.5)
    b = (torch.randn(Co, generator=gen) * 0.1).float().to(F64)
    g = _bfr(N, Co, H // 2, W // 2, gen=gen)
    return dict(x=x, w=w, b=b, g=g, N=N, H=H, W=W, Ci=Ci, Co=Co)


def conv_reference(c):
    """float64 on the case's inputs: y, dx (masked by x's sign), dw, db"""
    y = layer(c['x'], c['w'], c['b'])
    dx, dw, db = conv_vjp(c['x'], c['w'], c['g'])
    return dict(y=y, dx=dx * mask_of(c['x']), dx_plain=dx, dw=dw, db=db)


def conv_generic_reference(c, storage=False):
    """the generic route of layers 2-4: the raw bf16 convolution, then lrelu(raw + bias) rounded again"""
    raw = conv(c['x'], c['w'])
    raw = bf(raw) if storage else raw
    y = F.leaky_relu(raw + c['b'].view(1, -1, 1, 1), SLOPE)
    return bf(y) if storage else y


def conv_tolerances(c, ref):
    m_out = c['N'] * (c['H'] // 2) * (c['W'] // 2)
    return dict(y_generic=3 * err(conv_generic_reference(c, True), ref['y']) + 16 * c['Ci'] * U32,
                y=3 * err(bf(ref['y']), ref['y']) + 16 * c['Ci'] * U32,
                dx=3 * err(bf(ref['dx']), ref['dx']) + 4 * c['Co'] * U32,
                dx_plain=3 * err(bf(ref['dx_plain']), ref['dx_plain']) + 4 * c['Co'] * U32,
                dw=m_out * U32, db=m_out * U32)


# name -> (b, C, h, w, H, W, kind)
PROBS_CASES = {}
for _C in (6, 7, 16):
    PROBS_CASES['up16_c%d' % _C] = (2, _C, 2, 2, 32, 32, 'logits')        # scale 16, as in production
    PROBS_CASES['wide_c%d' % _C] = (2, _C, 2, 3, 32, 48, 'logits')
PROBS_CASES['interior_c6'] = (1, 6, 8, 8, 128, 128, 'logits')          # scale 16 with interior pixels: footprints smaller than the map
PROBS_CASES['pack_c7'] = (2, 7, 32, 32, 32, 32, 'pack')
PROBS_CASES['onehot_c6'] = (2, 6, 2, 2, 32, 32, 'onehot')


def probs_case(name):
    b, C, h, w, H, W, kind = PROBS_CASES[name]
    gen = _gen(2000 + sum(map(ord, name)))
    if kind == 'pack':
        x = torch.softmax(torch.randn(b, C, h, w, generator=gen) * 2, 1)
    elif kind == 'onehot':
        hot = torch.randint(0, C, (b, h, w), generator=gen)
        x = torch.full((b, C, h, w), -30.0).scatter_(1, hot[:, None], 30.0)
    else:
        x = torch.randn(b, C, h, w, generator=gen) * 2
    dP = _bfr(b, C, H, W, gen=gen)
    return dict(x=x.float(), dP=dP, size=(H, W), softmax=kind != 'pack', b=b, C=C, h=h, w=w, H=H, W=W)


def probs_reference(c):
    return dict(P=probs(c['x'], c['size'], c['softmax']), dx=probs_backward(c['x'], c['dP'], c['size'], c['softmax']))


def probs_tolerances(c, ref):
    # forward: a handful of f32 operations per value (two lerps, exp, the sum over C, a division) before the bf16 store;
    # backward: the full-resolution pixels of one bilinear footprint, at most (2 scale + 2) per axis and never more than the
    # map, add onto one low-resolution value
    fy, fx = min(c['H'], 2 * -(-c['H'] // c['h']) + 2), min(c['W'], 2 * -(-c['W'] // c['w']) + 2)
    return dict(P=3 * err(bf(ref['P']), ref['P']) + 32 * U32, dx=(fy * fx + 32) * U32)


# name -> (N, H, W of a4, C)
HEAD_CASES = {'one': (2, 2, 2, 512), 'grid': (2, 4, 6, 512)}


def head_case(name):
    N, H, W, C = HEAD_CASES[name]
    gen = _gen(3000 + sum(map(ord, name)))
    a = _bfr(N, C, H, W, gen=gen)
    a.view(-1)[0::5] = 0.0
    a.view(-1)[2::13] = -0.0
    w = (torch.randn(1, C, 4, 4, generator=gen) * (16 * C) ** -0.5).float().to(F64)
    b = torch.randn(1, generator=gen).float().to(F64)
    dz = torch.randn(N, 1, H // 2, W // 2, generator=gen).float().to(F64)
    return dict(a=a, w=w, b=b, dz=dz, N=N, H=H, W=W, C=C)


def head_reference(c):
    da, dw, db = conv_vjp(c['a'], c['w'], c['dz'])
    return dict(z=conv(c['a'], c['w'], c['b']), da=da * mask_of(c['a']), dw=dw, db=db)


def head_tolerances(c, ref):
    nz = c['N'] * (c['H'] // 2) * (c['W'] // 2)
    return dict(z=16 * c['C'] * U32, da=3 * err(bf(ref['da']), ref['da']) + 4 * U32, dw=nz * U32, db=nz * U32)


BCE_SIZES = {'small': 2, 'rows': 300}        # below and above one workgroup's 256 threads


def bce_case(name):
    n = BCE_SIZES[name]
    gen = _gen(4000 + n)
    z = torch.randn(n, generator=gen) * 5
    z[0], z[-1] = 40.0, -40.0                 # softplus / sigmoid at the ends of the stable form
    return z.float()


def bce_tolerances(n):
    # loss: n values summed in f32, each of a few f32 operations; dz: a few f32 operations per value
    return dict(loss=(n + 8) * U32, dz=8 * U32)


# name -> (ndf, C, b, H, W)
MODULE_CASES = {}
for _ndf in (32, 64):
    for _C in (6, 7):
        for _hw in ((32, 32), (64, 96)):
            MODULE_CASES['ndf%d_c%d_%dx%d' % (_ndf, _C, *_hw)] = (_ndf, _C, 2, *_hw)


def module_case(name):
    """weights drawn here (the reference's initialisation scale), an input of probabilities, and both labels"""
    ndf, C, b, H, W = MODULE_CASES[name]
    gen = _gen(5000 + sum(map(ord, name)))
    shapes = {'conv1': (ndf, C), 'conv2': (2 * ndf, ndf), 'conv3': (4 * ndf, 2 * ndf), 'conv4': (8 * ndf, 4 * ndf),
              'classifier': (1, 8 * ndf)}
    sd = {}
    for n, (co, ci) in shapes.items():
        k = (16 * ci) ** -0.5
        sd[n + '.weight'] = ((torch.rand(co, ci, 4, 4, generator=gen) * 2 - 1) * k * 3 ** 0.5).float()
        sd[n + '.bias'] = ((torch.rand(co, generator=gen) * 2 - 1) * k).float()
    x = torch.softmax(torch.randn(b, C, H, W, generator=gen) * 2, 1).float()
    return dict(sd=sd, x=x, ndf=ndf, C=C, b=b, H=H, W=W)


def module_reference(c, label, storage=False):
    return disc_loss_grads(params64(c['sd']), c['x'], label, storage)


def module_tolerances(c):
    """{label: {quantity: tolerance}}: z per element (err), dx and every parameter gradient by rel2, and per parameter the
    most elements that may move against the restatement in an Adam step (opposite_bound).  K of the f32 floor: the longest
    accumulation of the chain, 16 * 8 ndf terms."""
    floor = 16 * 8 * c['ndf'] * U32
    out = {}
    for label in (0, 1):
        ref, sto = module_reference(c, label), module_reference(c, label, storage=True)
        t = dict(z=3 * err(sto['z'], ref['z']) + floor, dx=3 * rel2(sto['dx'], ref['dx']) + floor)
        for k in PARAMS:
            t[k] = 3 * rel2(sto['grads'][k], ref['grads'][k]) + floor
            t['opposite.' + k] = opposite_bound(sto['grads'][k], ref['grads'][k])
        out[str(label)] = t
    return out


# ------------------------------------------------------------------------------------------------ goldens (tests/golden/adv.npz)
GOLDEN_CASES = ('c6_32x32', 'c7_32x32', 'c6_64x96', 'c7_64x96')
GOLDEN_NDF = 8


def golden_part(name, label):
    return 'adv_%s_t%d.npz' % (name, label)


def golden_case(load, name):
    """one case of the adv*.npz fixtures as torch tensors: sd, x, z, loss<t>, dx<t>, g<t> = {key: gradient}.
    load(file name) -> the opened npz (the `gold` fixture)"""
    base = load('adv.npz')
    c = dict(sd={k: torch.from_numpy(base['%s_sd.%s' % (name.split('_')[0], k)]) for k in PARAMS},
             z=torch.from_numpy(base[name + '_z']))
    for lab in (0, 1):
        part = load(golden_part(name, lab))
        if lab == 0:
            c['x'] = torch.from_numpy(part['x'])
        c['loss%d' % lab], c['dx%d' % lab] = torch.from_numpy(part['loss']), torch.from_numpy(part['dx'])
        c['g%d' % lab] = {k: torch.from_numpy(part['g.' + k]) for k in PARAMS}
    return c


def autograd_reference(sd, x, label, dtype=F64):
    """the reference's own formulation (F.conv2d, F.leaky_relu, F.binary_cross_entropy_with_logits, autograd) in `dtype`:
    float32 is, operation for operation, what the reference computes"""
    p = {k: sd[k].detach().to(dtype).clone().requires_grad_(True) for k in PARAMS}
    x = x.detach().to(dtype).clone().requires_grad_(True)
    a = x
    for n in LAYERS:
        a = F.leaky_relu(conv(a, p[n + '.weight'], p[n + '.bias']), SLOPE)
    z = conv(a, p['classifier.weight'], p['classifier.bias'])
    loss = F.binary_cross_entropy_with_logits(z, torch.full_like(z, float(label)))
    loss.backward()
    return dict(z=z.detach(), loss=loss.detach(), dx=x.grad, grads={k: v.grad for k, v in p.items()})


def golden_tolerances(c):
    """{label: {quantity: bound}}: three times the deviation of the float32 evaluation from the float64 one on the golden's
    inputs.  The two single values, loss and classifier.bias, add one f32 rounding (2^-24, relative): a lucky draw of a
    scalar otherwise sets a bound of 0."""
    out = {}
    for lab in (0, 1):
        lo, hi = autograd_reference(c['sd'], c['x'], lab, torch.float32), autograd_reference(c['sd'], c['x'], lab)
        t = {q: 3 * err(lo[q], hi[q]) for q in ('z', 'loss', 'dx')}
        t.update({k: 3 * err(lo['grads'][k], hi['grads'][k]) for k in PARAMS})
        t['loss'] += U32
        t['classifier.bias'] += U32
        out[str(lab)] = t
    return out
