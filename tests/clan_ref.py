"""float64 restatement, in plain torch on the CPU, of the category-level adversarial path (csrc/clan_kernels.hip,
regda_amd/gast/clan.py): the pair probabilities softmax(up x1 + up x2) and the weight map 1 - cos(softmax(up x1),
softmax(up x2)), WeightedBCEWithLogitsLoss (regda/loss.py:60-85) on an upsampled map, and every gradient by autograd.
Its storage model rounds P and the discriminator's rows (adv_ref) to bf16 where the kernels store bf16; everything else
the kernels keep in f32.  Also the cases the GPU tests and derive_clan_tolerances.py share.

Tolerances follow adv_ref's convention, 3 x (the storage model's deviation from float64 on the same case) + K * 2^-24.
Only P is stored as bf16 by the kernels that run alone, so for every other tensor the storage term is 0 and the bound is
the f32 term, which is worked out below from the operations behind one element:

  * an interpolated logit is two lerps, six roundings of values up to A = max(1, max |x|): 6 A u absolute, u = 2^-24;
    adding two heads and subtracting the row maximum brings the argument of expf to 8 A u per head;
  * expf and log1pf are allowed ULP_EXPF and ULP_LOG1PF ulps (2 u each), the figures of the HIP math accuracy table of the
    ROCm documentation ("HIP math API", single precision: expf 1 ULP, log1pf 1 ULP);
  * a probability therefore carries K_p(heads) = 2 (8 A heads) + 2 ULP_EXPF + C + 2 relative roundings (its own exponent
    and the normaliser's, the sum over C, the division);
  * a sum of n terms in f32 adds n u: for the pair backward that is the footprint's length, as adv_ref counts it for
    rgda_adv_probs_bwd; the weighted BCE's dz, whose terms k (sigmoid - t) differ in size by the factor 1 + beta / alpha,
    measures its sum against the terms' magnitudes, read from the float64 reference, never from the code under test."""
import itertools

import torch
import torch.nn.functional as F

import adv_ref as R

F64, U32 = R.F64, R.U32
ULP_EXPF, ULP_LOG1PF = 1, 1


# ------------------------------------------------------------------------------------------------ pieces
def up(x, size):
    """(b, C, h, w) -> (b, C, H, W), bilinear, align_corners=True; the identity where the sizes agree"""
    if tuple(size) == tuple(x.shape[-2:]):
        return x
    return F.interpolate(x, size=tuple(size), mode='bilinear', align_corners=True)


def up_transpose(v, hw):
    """the transpose of up() applied to v (b, C, H, W) -> (b, C, h, w)"""
    z = torch.zeros(*v.shape[:2], *hw, dtype=F64, requires_grad=True)
    (up(z, v.shape[-2:]) * v).sum().backward()
    return z.grad


def pair_at(u1, u2):
    """full-resolution logits -> (q = softmax(u1 + u2), wmap = 1 - cos(softmax u1, softmax u2))"""
    p1, p2 = F.softmax(u1, 1), F.softmax(u2, 1)
    wmap = 1 - (p1 * p2).sum(1) / (p1.norm(dim=1) * p2.norm(dim=1))
    return F.softmax(u1 + u2, 1), wmap


def pair(x1, x2, size):
    """x1, x2 (b, C, h, w) -> (P (b, C, H, W), wmap (b, H, W)) in float64"""
    return pair_at(up(x1.to(F64), size), up(x2.to(F64), size))


def pair_backward(x1, x2, dP, gw, size):
    """(dx1, dx2): the gradient of pair() for the upstream gradients dP (b, C, H, W) and gw (b, H, W) or None"""
    x1, x2 = x1.to(F64).clone().requires_grad_(True), x2.to(F64).clone().requires_grad_(True)
    P, wmap = pair_at(up(x1, size), up(x2, size))
    obj = (P * dP.to(F64)).sum()
    if gw is not None:
        obj = obj + (wmap * gw.to(F64)).sum()
    return torch.autograd.grad(obj, (x1, x2))


def bce_elements(zu, t):
    """max(z, 0) - t z + log1p(exp(-|z|)): BCE with logits in its stable form"""
    return zu.clamp(min=0) - t * zu + torch.log1p(torch.exp(-zu.abs()))


def wbce(z, size, target, wmap=None, alpha=1.0, beta=0.0, scale=1.0, mean=True):
    """z (b, hz, wz), target a (b, H, W) tensor or a number, wmap (b, H, W) or None -> the loss"""
    zu = up(z.to(F64).unsqueeze(1), size).squeeze(1)
    t = target.to(F64) if isinstance(target, torch.Tensor) else float(target)
    kl = bce_elements(zu, t)
    if wmap is not None:
        kl = (alpha + beta * wmap.to(F64)) * kl
    return scale * (kl.mean() if mean else kl.sum())


def wbce_grads(z, size, target, wmap=None, alpha=1.0, beta=0.0, scale=1.0, mean=True):
    """-> (loss, dz of z's shape, gw (b, H, W) or None)"""
    z = z.to(F64).clone().requires_grad_(True)
    w = None if wmap is None else wmap.to(F64).clone().requires_grad_(True)
    loss = wbce(z, size, target, w, alpha, beta, scale, mean)
    loss.backward()
    return loss.detach(), z.grad, None if w is None else w.grad


# ------------------------------------------------------------------------------------------------ the aligner's two terms
def generator_term(p, x1, x2, size, weight, label, epsilon, lambda_local, weighted=True, weight_grad=True, storage=False):
    """weight * wBCE(up D(P), label, wmap) and its gradient with respect to both heads' logits, through the
    discriminator's data gradients and (weight_grad) the weight map.  p: adv_ref.params64.  -> dict(loss, dx1, dx2)"""
    r = R.bf if storage else (lambda t: t)
    P, wmap = pair(x1, x2, size)
    z, acts = R.disc_forward(p, r(P), storage)
    loss, dz, gw = wbce_grads(z[:, 0], size, label, wmap if weighted else None, epsilon, lambda_local, weight)
    dP, _ = R.disc_backward(p, acts, dz.unsqueeze(1), storage)
    dx1, dx2 = pair_backward(x1, x2, dP, gw if weighted and weight_grad else None, size)
    return dict(loss=loss, dx1=dx1, dx2=dx2)


def discriminator_term(p, source, target, size, source_label, target_label, epsilon, lambda_local, weighted=True,
                       storage=False):
    """0.5 * (BCE(up D(P_s), source_label) + wBCE(up D(P_t), target_label, wmap)) -> dict(loss, grads)"""
    r = R.bf if storage else (lambda t: t)
    loss, total = 0.0, None
    for (x1, x2), label, use in ((source, source_label, False), (target, target_label, weighted)):
        P, wmap = pair(x1, x2, size)
        z, acts = R.disc_forward(p, r(P), storage)
        li, dz, _ = wbce_grads(z[:, 0], size, label, wmap if use else None, epsilon, lambda_local, 0.5)
        _, grads = R.disc_backward(p, acts, dz.unsqueeze(1), storage)
        loss = loss + li
        total = grads if total is None else {k: total[k] + grads[k] for k in grads}
    return dict(loss=loss, grads=total)


# ------------------------------------------------------------------------------------------------ f32 terms of the bounds
def amp(*ts):
    return max(1.0, max(float(t.abs().max()) for t in ts))


def k_prob(A, C, heads):
    return 2 * (8 * A * heads) + 2 * ULP_EXPF + C + 2


def footprint(n_in, n_out):
    """the most full-resolution indices whose lerp touches one low-resolution index"""
    return n_out if n_in <= 1 else min(n_out, 2 * -(-n_out // n_in) + 2)


# ------------------------------------------------------------------------------------------------ shared cases
def _gen(seed):
    return torch.Generator().manual_seed(seed)


# name -> (b, C, h, w, H, W, same)
PAIR_SHAPES = {'one': (1, 1, 32, 32),            # the degenerate in <= 1 branch of the footprint
               'border': (2, 3, 32, 64),         # every low-resolution pixel on a border
               'ratio': (5, 7, 64, 96),          # a non-integer ratio
               'identity': (33, 35, 33, 35)}     # the identity map; 2 * 33 * 35 pixels are no multiple of 256
PAIR_CASES = {'%s_c%d' % (n, C): (2, C, *s, False) for C in (6, 7, 16) for n, s in PAIR_SHAPES.items()}
PAIR_CASES['same_c6'] = (2, 6, 2, 3, 32, 64, True)          # x1 == x2: the weight map is 0, its gradient path stays finite


def pair_case(name):
    b, C, h, w, H, W, same = PAIR_CASES[name]
    gen = _gen(6000 + sum(map(ord, name)))
    x1 = (torch.randn(b, C, h, w, generator=gen) * 2).float()
    x2 = x1.clone() if same else (x1 * 0.5 + torch.randn(b, C, h, w, generator=gen) * 1.5).float()
    dP = R.bf(torch.randn(b, C, H, W, generator=gen))
    gw = (torch.randn(b, H, W, generator=gen) * 3).float()
    return dict(x1=x1, x2=x2, dP=dP, gw=gw, size=(H, W), b=b, C=C, h=h, w=w, H=H, W=W)


def pair_reference(c):
    P, wmap = pair(c['x1'], c['x2'], c['size'])
    out = dict(P=P, wmap=wmap)
    for key, gw in (('', c['gw']), ('_nogw', None)):
        out['dx1' + key], out['dx2' + key] = pair_backward(c['x1'], c['x2'], c['dP'], gw, c['size'])
    return out


K_SOFTMAX = 32          # adv_ref.probs_tolerances' count for one upsampled softmax and its backward: two lerps, exp, the sum
#                         over C, a division, the dot product


def pair_tolerances(c, ref):
    """P, dx*: err() bounds; wmap: an ABSOLUTE bound (it may be 0 everywhere).  The cosine is a quotient of three dot
    products of probabilities: 4 K_p(1) + C + 8 roundings of a value of at most 1.  dx, as adv_ref's for the sibling
    kernel: K = the full-resolution pixels of one bilinear footprint, summed in f32 onto one low-resolution value, plus the
    operations behind one term -- without gw one softmax (K_SOFTMAX, 2 ULP_EXPF for its expf, 6 for the second head's
    lerps); with gw three softmaxes and 8 for the norms, the quotient and the products of the weight map's derivative."""
    A, C = amp(c['x1'], c['x2']), c['C']
    n_sum = footprint(c['h'], c['H']) * footprint(c['w'], c['W'])
    out = dict(P=3 * R.err(R.bf(ref['P']), ref['P']) + k_prob(A, C, 2) * U32, wmap=(4 * k_prob(A, C, 1) + C + 8) * U32)
    one = K_SOFTMAX + 2 * ULP_EXPF
    for i in (1, 2):
        out['dx%d' % i] = (n_sum + 3 * one + 6 + 8) * U32
        out['dx%d_nogw' % i] = (n_sum + one + 6) * U32
    return out


# name -> (b, hz, wz, H, W)
WBCE_SHAPES = {'one': (2, 1, 1, 32, 32), 'ragged': (2, 2, 3, 64, 96), 'odd': (2, 3, 3, 33, 35), 'tile': (1, 16, 16, 512, 512)}
# (target: 0, 1 or 'tensor'; wmap given; mean; accumulate; dz wanted; gw wanted): every combination the entry point takes
# (the gradient for the weight map needs one); the aligner's own are (0, w, mean, acc, dz, gw) and (1, w, mean, acc, dz, -)
WBCE_VARIANTS = tuple(v for v in itertools.product((0, 1, 'tensor'), (False, True), (True, False), (False, True),
                                                   (True, False), (False, True)) if v[1] or not v[5])
TILE_VARIANT = (0, True, True, True, True, True)
ALPHA, BETA, SCALE = 0.4, 40.0, 0.5


def wbce_variants(shape):
    return (TILE_VARIANT,) if shape == 'tile' else WBCE_VARIANTS


def bounds_key(shape, v):
    """the bounds depend on the shape, the kind of target and whether a weight map is given -- not on the other switches"""
    return '%s.t%s_%s' % (shape, v[0], 'w' if v[1] else 'plain')


def variant_name(v):
    return 't%s_%s_%s_%s_%s%s' % (v[0], 'w' if v[1] else 'plain', 'mean' if v[2] else 'sum', 'acc' if v[3] else 'set',
                                  'dz' if v[4] else '', 'gw' if v[5] else '')


def wbce_case(shape):
    """logits with +-80 at the ends of the stable form, a soft target in [0, 1], a weight map in [0, 1]"""
    b, hz, wz, H, W = WBCE_SHAPES[shape]
    gen = _gen(7000 + sum(map(ord, shape)))
    z = (torch.randn(b, hz, wz, generator=gen) * 3).float()
    z.view(-1)[0], z.view(-1)[-1] = 80.0, -80.0
    target = torch.rand(b, H, W, generator=gen).float()
    target.view(-1)[::3] = 1.0
    target.view(-1)[1::3] = 0.0
    wmap = torch.rand(b, H, W, generator=gen).float() ** 2
    return dict(z=z, target=target, wmap=wmap, size=(H, W), b=b, hz=hz, wz=wz, H=H, W=W)


def wbce_reference(c, v):
    t, use_w, mean = v[0], v[1], v[2]
    loss, dz, gw = wbce_grads(c['z'], c['size'], c['target'] if t == 'tensor' else t, c['wmap'] if use_w else None,
                              ALPHA, BETA, SCALE, mean)
    return dict(loss=loss, dz=dz, gw=gw)


def wbce_tolerances(z, size, target, wmap, alpha, beta, ref, workgroup=256):
    """loss: a RELATIVE bound; dz, gw: err() bounds.  An upsampled logit carries 6 Az u (Az = max(1, max |z|)); an element
    l = max(zu, 0) - t zu + log1p(exp(-|zu|)) then 10 Az + 2 (ULP_EXPF + ULP_LOG1PF) absolute roundings, the sigmoid (slope <=
    1 / 4) 2 Az + 2 ULP_EXPF + 4; the loss is a sum of k l through a tree of depth 8 per workgroup, ceil(workgroups / 256)
    strided terms and another tree of depth 8; dz sums its footprint's terms."""
    b, hz, wz = z.shape
    H, W = size
    Az = amp(z)
    zu = up(z.to(F64).unsqueeze(1), size).squeeze(1)
    t = target.to(F64) if isinstance(target, torch.Tensor) else float(target)
    k = torch.ones_like(zu) if wmap is None else alpha + beta * wmap.to(F64)
    l = bce_elements(zu, t)
    k_l = 10 * Az + 2 * (ULP_EXPF + ULP_LOG1PF)
    depth = 16 + -(-(-(-(b * H * W) // workgroup)) // 256)         # 8 + ceil(ceil(n / 256) / 256) + 8
    out = dict(loss=(depth + 3 + k_l * float(k.sum() / (k * l).sum())) * U32)
    if ref.get('gw') is not None:
        out['gw'] = (k_l / float(l.max()) + 3) * U32
    if ref.get('dz') is not None:
        g = k * (torch.sigmoid(zu) - t)
        n_sum = footprint(hz, H) * footprint(wz, W)
        mag, ksum = up_transpose(g.abs().unsqueeze(1), (hz, wz)), up_transpose(k.unsqueeze(1), (hz, wz))
        unit = up_transpose(g.unsqueeze(1), (hz, wz)).abs().max()          # dz without its scale
        out['dz'] = float(((n_sum + 4) * mag.max() + (2 * Az + 2 * ULP_EXPF + 4) * ksum.max()) / unit) * U32
    return out


# ------------------------------------------------------------------------------------------------ goldens (tests/golden/clan.npz)
# name -> (shape, target kind, weight given, alpha, beta, size_average)
GOLDEN_CASES = {'map_mean': ((2, 1, 8, 12), 'domain', True, 0.4, 40.0, True),
                'map_sum': ((2, 1, 8, 12), 'domain', True, 0.4, 40.0, False),
                'soft_mean': ((3, 5, 7), 'soft', True, 1.0, 2.5, True),
                'plain_mean': ((2, 1, 8, 12), 'soft', False, 0.4, 40.0, True),
                'plain_sum': ((70,), 'domain', False, 0.0, 0.0, False)}


def golden_inputs(name):
    """float32 inputs (exact in float64): logits with +-80, a domain label (all ones) or a soft target, a weight in [0, 1]"""
    shape, kind, use_w, alpha, beta, mean = GOLDEN_CASES[name]
    gen = _gen(8000 + sum(map(ord, name)))
    x = (torch.randn(*shape, generator=gen) * 3).float()
    x.view(-1)[0], x.view(-1)[-1] = 80.0, -80.0
    target = torch.ones(*shape) if kind == 'domain' else torch.rand(*shape, generator=gen).float()
    weight = torch.rand(*shape, generator=gen).float() if use_w else None
    return dict(input=x, target=target, weight=weight, alpha=alpha, beta=beta, size_average=mean)


def golden_case(load, name):
    npz = load('clan.npz')
    c = {k: torch.from_numpy(npz['%s_%s' % (name, k)]) for k in ('input', 'target', 'loss', 'dinput')}
    for k in ('weight', 'dweight'):
        c[k] = torch.from_numpy(npz['%s_%s' % (name, k)]) if '%s_%s' % (name, k) in npz.files else None
    c['alpha'], c['beta'] = float(npz[name + '_alpha']), float(npz[name + '_beta'])
    c['size_average'] = bool(npz[name + '_size_average'])
    return c


def as_map(t):
    """an input of the module, any shape -> the (b, H, W) the kernel sees (regda_amd/loss.py)"""
    return t.reshape(-1, *t.shape[-2:]) if t.dim() >= 2 else t.reshape(1, 1, -1)


def golden_restatement(c):
    """-> (loss, dinput, dweight) of the restatement on a golden's inputs, at the input's own size"""
    z = as_map(c['input'])
    loss, dz, gw = wbce_grads(z, z.shape[-2:], as_map(c['target']), None if c['weight'] is None else as_map(c['weight']),
                              c['alpha'], c['beta'], 1.0, c['size_average'])
    return loss, dz.reshape(c['input'].shape), None if gw is None else gw.reshape(c['input'].shape)


def golden_tolerances(c):
    z = as_map(c['input'])
    ref = dict(dz=c['dinput'], gw=c['dweight'])
    return wbce_tolerances(z, tuple(z.shape[-2:]), as_map(c['target']), None if c['weight'] is None else as_map(c['weight']),
                           c['alpha'], c['beta'], ref)
