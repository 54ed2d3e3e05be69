"""GPU: the linear passes of norm_kernels.hip / mix_kernels.hip -- rgda_spatial_mix, _spatial_mix_multi, _group_mix,
_sparse_mix and the classifier forward / backward -- on every case of tests/norm_cases.py, per element against float64
references on the same stored inputs (computed on the GPU).

Bound of an output that is a sum of n products (fp32 products of a bf16 value and an fp32 weight are rounded once; the
sum is formed in fp32 in any fixed order): |err| <= (n + 1) 2^-24 sum |terms|; then the store rounds once more (2^-8 of
the value for bf16, 2^-24 for fp32).  n is the longest chain of additions the kernel's layout gives one partial
(a slice's terms, then the slices in order), not the whole term count, where that is known from the launch."""
import pytest
import torch

import norm_cases as N
from norm_cases import U, U32, cdiv

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
DEV = 'cuda'


@pytest.fixture(scope='module')
def ops():
    from regda_amd import ops
    return ops


def _gen(*key):
    import zlib
    return torch.Generator(device=DEV).manual_seed(zlib.crc32(repr(key).encode()) % 100000)


def _buf(rows, C, pad, dtype, gen=None):
    """[rows][C] view of a [rows][C + pad] buffer (NaN pad); random values if gen is given."""
    t = torch.full((rows, C + pad), float('nan'), dtype=dtype, device=DEV)[:, :C]
    if gen is not None:
        t.copy_(torch.randn(rows, C, generator=gen, device=DEV).to(dtype))
    return t


def _check(name, got, ref, bound):
    d = (got.double() - ref).abs()
    bad = int((~(d <= bound)).sum())
    assert bad == 0, '%s: %d of %d off; max |diff| %.3e' % (name, bad, got.numel(), float(d.max()))


def _store(ref, dtype):
    return (U if dtype == BF else U32) * ref.abs()


def _sparse_matrix(gen, I, J, density, zero_rows=()):
    m = torch.randn(I, J, generator=gen, device=DEV) * (torch.rand(I, J, generator=gen, device=DEV) < density)
    for i in zero_rows:
        m[i] = 0
    return m.contiguous()


@pytest.mark.parametrize('case', N.SPATIAL, ids=['%dx%dx%dx%d-pad%d-acc%d-f32%d' % c for c in N.SPATIAL])
def test_spatial_mix(ops, case):
    """out[n][i] (+)= sum_j Mx[i][j] in[n][j]: a slice sums every SL-th nonzero of the row, the SL slices are added in
    order -> chains of ceil(J / SL) + SL additions; the accumulate path adds the stored output (one more rounding)."""
    Nn, I, J, C, pad, acc, f32 = case
    gen = _gen('smix', case)
    odt = torch.float32 if f32 else BF
    inp = _buf(Nn * J, C, pad, BF, gen)
    Mx = _sparse_matrix(gen, I, J, 0.3 if J >= 256 else 0.8, zero_rows=(I - 1,))
    out = _buf(Nn * I, C, pad, odt, gen if acc else None)
    if not acc:
        out.zero_()
    old = out.double().clone()
    ops.spatial_mix(inp, Mx, out, Nn, I, J, C, accumulate=acc)
    x = inp.double().reshape(Nn, J, C)
    ref = (Mx.double() @ x).reshape(Nn * I, C)
    mag = (Mx.double().abs() @ x.abs()).reshape(Nn * I, C)
    if acc:
        ref, mag = ref + old, mag + old.abs()
    SL = N.SPATIAL_MIX_SLICES[J >= 256]
    n = cdiv(J, SL) + SL + 2
    _check('spatial_mix', out, ref, _store(ref, odt) + n * U32 * mag)


@pytest.mark.parametrize('case', N.SPATIAL_MULTI, ids=['%dx%d-%s-%d-pad%d' % (c[0], c[1], '+'.join(map(str, c[2])), c[3], c[4])
                                                      for c in N.SPATIAL_MULTI])
def test_spatial_mix_multi(ops, case):
    """out[n][i] = sum_q Mq[i] @ inq[n] (bf16 out): the 256 threads are CVB vectors x 256 / CVB slices of the staged entry
    list; every channel block of C is a pass of the same workgroup."""
    Nn, I, Js, C, pad = case
    assert sum(Js) <= N.SPATIAL_MULTI_MAX_J
    gen = _gen('smixm', case)
    ins = [_buf(Nn * J, C, pad + 8 * q, BF, gen) for q, J in enumerate(Js)]
    mats = [_sparse_matrix(gen, I, J, 0.5) for J in Js]
    out = _buf(Nn * I, C, pad, BF)
    ops.spatial_mix_multi(ins, mats, out, Nn, I, C)
    ref = sum((m.double() @ t.double().reshape(Nn, -1, C)) for m, t in zip(mats, ins)).reshape(Nn * I, C)
    mag = sum((m.double().abs() @ t.double().abs().reshape(Nn, -1, C)) for m, t in zip(mats, ins)).reshape(Nn * I, C)
    cvb = 256 if C // 8 >= 256 else 128 if C // 8 >= 128 else 64 if C // 8 >= 64 else 32
    SL = 256 // cvb
    n = cdiv(sum(Js), SL) + SL + 2
    _check('spatial_mix_multi', out, ref, _store(ref, BF) + n * U32 * mag)


@pytest.mark.parametrize('case', N.GROUP, ids=['g%d-%dx%d-%d-pad%d-in%d-out%d' % c for c in N.GROUP])
def test_group_mix(ops, case):
    """out[g][i] = sum_j W[i][j] in[g][j]: one thread walks the J terms in order (chains of J additions)."""
    G, I, J, C, pad, in32, out32 = case
    gen = _gen('gmix', case)
    idt, odt = (torch.float32 if in32 else BF), (torch.float32 if out32 else BF)
    inp = _buf(G * J, C, pad, idt, gen)
    W = torch.randn(I, J, generator=gen, device=DEV).contiguous()
    out = _buf(G * I, C, pad, odt)
    ops.group_mix(inp, W, out, G, I, J, C)
    x = inp.double().reshape(G, J, C)
    ref = (W.double() @ x).reshape(G * I, C)
    mag = (W.double().abs() @ x.abs()).reshape(G * I, C)
    _check('group_mix', out, ref, _store(ref, odt) + (J + 2) * U32 * mag)


@pytest.mark.parametrize('case', N.SPARSE, ids=['n%d-%s-%s-%d-pad%d-in%d-out%d' % (c[0], '+'.join(map(str, c[1])),
                                                                                   '+'.join(map(str, c[2])), *c[3:])
                                                for c in N.SPARSE])
def test_sparse_mix(ops, case):
    """outs[q][n][i] = sum over the CSR row of vals[k] ins[src(k)][n][col(k)]: one thread walks the row in order."""
    Nn, Js, rows, C, pad, in32, out32 = case
    gen = _gen('spmix', case)
    idt, odt = (torch.float32 if in32 else BF), (torch.float32 if out32 else BF)
    ins = [_buf(Nn * J, C, pad + 8 * q, idt, gen) for q, J in enumerate(Js)]
    I = sum(rows)
    # row i gets i % 21 entries (0 .. 20) from random sources and columns; the dense equivalent per source
    rowptr, cols, vals = [0], [], []
    dense = [torch.zeros(I, J, dtype=torch.float64) for J in Js]
    g = torch.Generator().manual_seed(len(Js) * 1000 + I)
    for i in range(I):
        for _ in range(i % 21):
            q = int(torch.randint(len(Js), (1,), generator=g))
            j = int(torch.randint(Js[q], (1,), generator=g))
            v = float(torch.randn(1, generator=g).float())
            cols.append((q << 24) | j)
            vals.append(v)
            dense[q][i, j] += v
        rowptr.append(len(cols))
    csr = (torch.tensor(rowptr, dtype=torch.int32, device=DEV), torch.tensor(cols or [0], dtype=torch.int32, device=DEV),
           torch.tensor(vals or [0.0], dtype=torch.float32, device=DEV))
    outs = [_buf(Nn * r, C, pad + 8 * q, odt) for q, r in enumerate(rows)]
    ops.sparse_mix(ins, csr, outs, Nn, C)
    ref = sum(d.to(DEV) @ t.double().reshape(Nn, -1, C) for d, t in zip(dense, ins))          # [N][I][C]
    mag = sum(d.abs().to(DEV) @ t.double().abs().reshape(Nn, -1, C) for d, t in zip(dense, ins))
    first = 0
    for q, (o, r) in enumerate(zip(outs, rows)):
        rq, mq = ref[:, first:first + r].reshape(Nn * r, C), mag[:, first:first + r].reshape(Nn * r, C)
        _check('sparse_mix out %d' % q, o, rq, _store(rq, odt) + 22 * U32 * mq)
        first += r


@pytest.mark.parametrize('case', N.CLASSIFIER, ids=['%dx%dx%d-c%d-pad%d' % c for c in N.CLASSIFIER])
def test_classifier(ops, case):
    """Forward: a lane sums its C / 512 chunks of 8 channels, the wave adds the 64 lanes in 6 steps (chains of
    C / 64 + 6 additions), then the bias.  Backward: dhidden = bf16(sum over the ncls classes), dW / db += sums over the
    rows -- 64 rows per workgroup (a row lane's share, then the row lanes in order), the workgroups' partials in 8 ordered
    slices: chains of 64 + ceil(blocks / 8) + 8 additions; dW and db are ADDED to what they held."""
    Nn, HW, C, nc, pad = case
    gen = _gen('cls', case)
    M = Nn * HW
    hid = _buf(M, C, pad, BF, gen)
    w = (torch.randn(nc, C, generator=gen, device=DEV) / C ** 0.5).contiguous()
    b = torch.randn(nc, generator=gen, device=DEV)
    logits = torch.full((Nn, nc, HW), float('nan'), device=DEV)
    ops.classifier_fwd(hid, w, b, logits, Nn, HW, C, nc)
    h = hid.double()
    ref = (h @ w.double().t() + b.double()).reshape(Nn, HW, nc).permute(0, 2, 1)
    mag = (h.abs() @ w.double().abs().t() + b.double().abs()).reshape(Nn, HW, nc).permute(0, 2, 1)
    _check('classifier logits', logits, ref, U32 * ref.abs() + (C / 64 + 10) * U32 * mag)
    gl = torch.randn(Nn, nc, HW, generator=gen, device=DEV)
    dh = _buf(M, C, pad, BF)
    dw0 = torch.randn(nc, C, generator=gen, device=DEV)
    db0 = torch.randn(nc, generator=gen, device=DEV)
    dw, db = dw0.clone(), db0.clone()
    ops.classifier_bwd(hid, w, gl, dh, dw, db, Nn, HW, C, nc)
    g = gl.double().permute(0, 2, 1).reshape(M, nc)
    rdh = g @ w.double()
    mdh = g.abs() @ w.double().abs()
    _check('classifier dhidden', dh, rdh, U * rdh.abs() + (nc + 2) * U32 * mdh)
    n = 64 + cdiv(cdiv(M, 64), 8) + 10
    rdw = dw0.double() + g.t() @ h
    mdw = dw0.double().abs() + g.abs().t() @ h.abs()
    _check('classifier dW', dw, rdw, n * U32 * mdw)
    rdb = db0.double() + g.sum(0)
    mdb = db0.double().abs() + g.abs().sum(0)
    _check('classifier db', db, rdb, n * U32 * mdb)
