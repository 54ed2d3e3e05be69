"""A restatement of the TransNorm contract (include/rgda_hip.h: rgda_transnorm_fwd / rgda_transnorm_bwd), written from
its formulae in plain torch: forward, backward, running update and eval, every intermediate returned.  It computes in
the dtype of `x` -- float64 for the tests' reference values, float32 where a tolerance script wants an fp32 evaluation.
Not the reference's code: the goldens (tests/golden/transnorm.npz) tie it to the reference's own modules."""
import torch

RUNNING = ('running_mean_source', 'running_var_source', 'running_mean_target', 'running_var_target')


def _cview(v, x):
    """a per-channel vector, broadcastable against x (n, C, ...)"""
    return v.view(1, -1, *([1] * (x.dim() - 2)))


def _alpha(mean_s, var_s, mean_t, var_t, eps):
    dis = (mean_s / (var_s + eps).sqrt() - mean_t / (var_t + eps).sqrt()).abs()
    prob = 1.0 / (1.0 + dis)
    return dis, prob, prob.numel() * prob / prob.sum()


def transnorm_train(x, weight=None, bias=None, running=None, eps=1e-5, momentum=0.1, g=None, n_src=None):
    """x (n, C) or (n, C, h, w); weight / bias [C] or None; running: (rm_s, rv_s, rm_t, rv_t) or None (not modified).
    -> dict: y, z, xhat, mean / var_b / var_u / rstd (each [2, C], source row first), dis, prob, alpha, saved [5, C],
    running (the four updated vectors, when given) and, with the upstream gradient g: dx, dweight, dbias."""
    n, C = x.shape[:2]
    n_src = n // 2 if n_src is None else n_src
    dims = [0] + list(range(2, x.dim()))
    w = torch.ones(C, dtype=x.dtype) if weight is None else weight.to(x.dtype)
    b = torch.zeros(C, dtype=x.dtype) if bias is None else bias.to(x.dtype)
    halves = (x[:n_src], x[n_src:])
    mean = torch.stack([h.mean(dims) for h in halves])
    var_b = torch.stack([h.var(dims, unbiased=False) for h in halves])
    var_u = torch.stack([h.var(dims, unbiased=True) for h in halves])
    rstd = 1.0 / (var_b + eps).sqrt()
    xhat = torch.cat([(h - _cview(mean[d], x)) * _cview(rstd[d], x) for d, h in enumerate(halves)])
    z = xhat * _cview(w, x) + _cview(b, x)
    dis, prob, alpha = _alpha(mean[0], var_u[0], mean[1], var_u[1], eps)
    a = 1.0 + alpha
    out = dict(y=z * _cview(a, x), z=z, xhat=xhat, mean=mean, var_b=var_b, var_u=var_u, rstd=rstd, dis=dis, prob=prob,
               alpha=alpha, saved=torch.stack([mean[0], rstd[0], mean[1], rstd[1], alpha]), n_src=n_src)
    if running is not None:
        r = [t.to(x.dtype) for t in running]
        out['running'] = ((1 - momentum) * r[0] + momentum * mean[0], (1 - momentum) * r[1] + momentum * var_u[0],
                          (1 - momentum) * r[2] + momentum * mean[1], (1 - momentum) * r[3] + momentum * var_u[1])
    if g is not None:
        g = g.to(x.dtype)
        ga = g * _cview(a, x)
        gh = ga * _cview(w, x)
        dx = []
        for d, sl in enumerate((slice(0, n_src), slice(n_src, n))):
            m1 = gh[sl].mean(dims)
            m2 = (gh[sl] * xhat[sl]).mean(dims)
            dx.append(_cview(rstd[d], x) * (gh[sl] - _cview(m1, x) - xhat[sl] * _cview(m2, x)))
        out.update(dx=torch.cat(dx), dweight=(ga * xhat).sum(dims), dbias=ga.sum(dims))
    return out


def transnorm_eval(x, weight, bias, running, eps=1e-5, g=None):
    """eval mode: the target's running statistics for every sample, alpha from the four running vectors
    -> dict: y, z, xhat, rstd_t, dis, prob, alpha, saved and, with g: dx, dweight, dbias."""
    C = x.shape[1]
    dims = [0] + list(range(2, x.dim()))
    w = torch.ones(C, dtype=x.dtype) if weight is None else weight.to(x.dtype)
    b = torch.zeros(C, dtype=x.dtype) if bias is None else bias.to(x.dtype)
    rm_s, rv_s, rm_t, rv_t = [t.to(x.dtype) for t in running]
    rstd_s, rstd_t = 1.0 / (rv_s + eps).sqrt(), 1.0 / (rv_t + eps).sqrt()
    xhat = (x - _cview(rm_t, x)) * _cview(rstd_t, x)
    z = xhat * _cview(w, x) + _cview(b, x)
    dis, prob, alpha = _alpha(rm_s, rv_s, rm_t, rv_t, eps)
    a = 1.0 + alpha
    out = dict(y=z * _cview(a, x), z=z, xhat=xhat, rstd_t=rstd_t, dis=dis, prob=prob, alpha=alpha,
               saved=torch.stack([rm_s, rstd_s, rm_t, rstd_t, alpha]))
    if g is not None:
        g = g.to(x.dtype)
        ga = g * _cview(a, x)
        out.update(dx=ga * _cview(w * rstd_t, x), dweight=(ga * xhat).sum(dims), dbias=ga.sum(dims))
    return out


def rel(a, ref):
    """the relative norm of a deviation (0 where both vanish)"""
    a, ref = a.double(), ref.double()
    den = ref.norm().item()
    num = (a - ref).norm().item()
    return num / den if den > 0 else num


GOLDEN_CASES = ('plain', 'shift', 'odd', 'rows', 'one')


def golden_case(g, name):
    """one case of tests/golden/transnorm.npz -> dict of torch tensors (f32 as stored) and floats"""
    keys = [k for k in g.files if k.startswith(name + '_')]
    out = {k[len(name) + 1:]: torch.from_numpy(g[k]) for k in keys}
    out['name'] = name
    out['eps'], out['momentum'] = float(out['eps']), float(out['momentum'])
    return out


def golden_steps(c, dtype=torch.float64):
    """What the golden's recipe gives in `dtype` by the restatement: one training step with gradient on x, a second
    training step on x2, then eval on x.  -> (step-1 dict, the running vectors after two steps, the eval dict)"""
    x, x2, w, b, g = (c[k].to(dtype) for k in ('x', 'x2', 'weight', 'bias', 'g'))
    C = x.shape[1]
    run = (torch.zeros(C, dtype=dtype), torch.ones(C, dtype=dtype), torch.zeros(C, dtype=dtype), torch.ones(C, dtype=dtype))
    s1 = transnorm_train(x, w, b, run, c['eps'], c['momentum'], g)
    s2 = transnorm_train(x2, w, b, s1['running'], c['eps'], c['momentum'])
    ev = transnorm_eval(x, w, b, s2['running'], c['eps'], g)
    return s1, s2['running'], ev


def production_inputs(seed=2019, n=8, C=2048, h=32, w=32):
    """-> (x, weight, bias, g) f32 at the production shape of the GPU test and of derive_transnorm_tolerances.py: per
    channel and domain a mean of scale 1 and a standard deviation in [0.5, 1.5] (the domains differ, so alpha varies over
    the channels), weight uniform in [0.5, 1.5), bias and g unit normal"""
    gen = torch.Generator().manual_seed(seed)
    mu = torch.randn(2, C, generator=gen)
    sd = torch.rand(2, C, generator=gen) + 0.5
    x = torch.randn(n, C, h, w, generator=gen)
    half = n // 2
    x[:half] = x[:half] * sd[0].view(1, C, 1, 1) + mu[0].view(1, C, 1, 1)
    x[half:] = x[half:] * sd[1].view(1, C, 1, 1) + mu[1].view(1, C, 1, 1)
    weight = torch.rand(C, generator=gen) + 0.5
    bias = torch.randn(C, generator=gen)
    g = torch.randn(n, C, h, w, generator=gen)
    return x, weight, bias, g


# ---- the edge shapes of the GPU test, shared with derive_transnorm_tolerances.py, which derives a bound per shape.
# (n, C, s, dims): s 1, 2, 63, 64, 65, 255, 257, 1025 and 15 | 16, the two sides of the route threshold; C 1, 3, 65 and 2048
# at s = 1; n 2, 3, 5 (4 and 6 where s = 1 needs two rows per half).  dims 2: an (n, C) input; 4: (n, C, 1, s).  Every
# shape has a few hundred values at least, so that a deviation is not the draw of a handful of roundings.
EDGE_SHAPES = ((5, 65, 1, 2), (4, 2048, 1, 2), (6, 70, 1, 2), (4, 65, 1, 4), (5, 65, 2, 4), (3, 65, 2, 4), (5, 3, 15, 4),
               (5, 3, 16, 4), (2, 65, 15, 4), (2, 65, 16, 4), (4, 37, 15, 4), (4, 37, 16, 4), (2, 37, 16, 4), (2, 65, 63, 4),
               (3, 3, 64, 4), (4, 5, 64, 4), (5, 65, 64, 4), (5, 1, 65, 4), (6, 6, 35, 4), (2, 3, 255, 4), (3, 65, 257, 4),
               (2, 1, 1025, 4), (5, 3, 1025, 4), (3, 3, 1028, 4))


def edge_key(n, C, s, dims):
    return f'edge_{n}_{C}_{s}_{dims}'


def edge_inputs(n, C, s, dims, seed=None):
    """-> (x, weight, bias, g) f32: the halves differ in mean (scale 1) and spread ([0.5, 1.5)) per channel"""
    gen = torch.Generator().manual_seed(100 + n + C + s if seed is None else seed)
    shape = (n, C) if dims == 2 else (n, C, 1, s)
    cv = (lambda v: v.view(1, C)) if dims == 2 else (lambda v: v.view(1, C, 1, 1))
    x = torch.randn(shape, generator=gen)
    half = n // 2
    x[:half] = x[:half] * cv(0.5 + torch.rand(C, generator=gen)) + cv(torch.randn(C, generator=gen))
    x[half:] = x[half:] * cv(0.5 + torch.rand(C, generator=gen)) + cv(torch.randn(C, generator=gen))
    return x, torch.rand(C, generator=gen) + 0.5, torch.randn(C, generator=gen), torch.randn(shape, generator=gen)


def dx_deviation(dx, ref, weight, g):
    """The deviation of a training-mode dx from the restatement `ref`, relative to the norm of rstd * g * (1 + alpha) *
    weight, its largest term, not to its own norm: with two or three values per half the three terms of dx cancel to
    eps / (var + eps) of their size, and a deviation relative to that residue measures the cancellation, not the
    arithmetic (where the halves are well filled the two norms agree)."""
    y = ref['y']
    n_src = ref['n_src']
    w = torch.ones_like(ref['alpha']) if weight is None else weight.double().cpu()
    t = g.double().cpu() * _cview((1 + ref['alpha']) * w, y)
    t[:n_src] *= _cview(ref['rstd'][0], y)
    t[n_src:] *= _cview(ref['rstd'][1], y)
    return ((dx.double().cpu() - ref['dx']).norm() / t.norm()).item()
