"""GPU: every kernel of regda_amd/csrc/optim_kernels.hip on the cases of tests/optim_cases.py, per element, and the
model's weight-layout bookkeeping that is built on them.

Technique: every output is a view inside a larger allocation filled with a sentinel (NaN for floats, the byte 0xA5 for
bf16 and integers) and the sentinel must be intact around the view afterwards; all accesses stay inside the allocations
by construction.  The exact passes (casts, rank-order sum, layouts, pad / unpad, fill, copy, dropout mask, bf16 add) are
compared bit for bit with the references of optim_cases.py; the gradient norm and the SGD step against fp64 within the
bounds derived there (roundings counted, nothing fitted)."""
import ctypes

import numpy as np
import pytest
import torch

import optim_cases as O

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
DEV = 'cuda'
GUARD = 64          # sentinel elements on either side of a view (a multiple of 16 bytes for every dtype)


@pytest.fixture(scope='module')
def ops():
    from regda_amd import ops
    return ops


def _raw(name, *args):
    from regda_amd._lib import lib
    lib().call(name, *args, torch.cuda.current_stream().cuda_stream)


def _gen(*key):
    import zlib
    return torch.Generator(device=DEV).manual_seed(zlib.crc32(repr(key).encode()) % 100000)


def _poison(t):
    if t.dtype.is_floating_point and t.dtype != BF:
        t.fill_(float('nan'))
    else:
        t.view(torch.uint8).fill_(0xA5)


def _is_poison(t):
    if t.dtype.is_floating_point and t.dtype != BF:
        return bool(torch.isnan(t).all())
    return bool((t.view(torch.uint8) == 0xA5).all())


class Arena:
    """`view`: n elements inside a sentinel-filled allocation, `off` elements past a 16-byte boundary."""

    def __init__(self, n, dtype, off=0, tail=GUARD):
        self.full = torch.empty(GUARD + off + n + tail, dtype=dtype, device=DEV)
        _poison(self.full)
        self.lo, self.n = GUARD + off, n
        self.view = self.full[self.lo:self.lo + n]

    def intact(self):
        return _is_poison(self.full[:self.lo]) and _is_poison(self.full[self.lo + self.n:])


def _filled(values):
    a = Arena(values.numel(), values.dtype)
    a.view.copy_(values.reshape(-1))
    return a


def _check(name, got, ref, bound):
    d = (got.double() - ref).abs()
    bad = ~(d <= bound)
    n = int(bad.sum())
    if n:
        i = int(bad.flatten().nonzero()[0])
        raise AssertionError('%s: %d of %d outside the bound; first at %d: got %r ref %r bound %.3e' % (
            name, n, got.numel(), i, float(got.flatten()[i]), float(ref.flatten()[i]), float(bound.flatten()[i])))


# ---------------------------------------------------------------- rgda_sumsq
def _positive(gen, n, scale):
    """|x| in [0.5, 1.5) scale, random signs: every square is a normal fp32 number."""
    x = (torch.rand(n, generator=gen, device=DEV) + 0.5) * scale
    return x * (torch.randint(0, 2, (n,), generator=gen, device=DEV) * 2 - 1)


@pytest.mark.parametrize('n', O.SUMSQ_N)
def test_sumsq(ops, n):
    for scale in (1.0, 1e-12, 3e9):
        g = _filled(_positive(_gen('sumsq', n, scale), n, scale))
        out, ws = Arena(1, torch.float32), Arena(O.SUMSQ_CAP, torch.float32)
        ops.sumsq(g.view, out.view, ws.view)
        ref = float((g.view.double() ** 2).sum())
        got = float(out.view)
        print('sumsq n %d scale %g: rel err %.3e (bound %.3e)' % (n, scale, abs(got / ref - 1), O.sumsq_bound(n)))
        assert abs(got - ref) <= O.sumsq_bound(n) * ref, (n, scale, got, ref)
        assert out.intact() and ws.intact() and g.intact()
        assert _is_poison(ws.view[O.sumsq_blocks(n):])        # one partial per workgroup, no more


# ---------------------------------------------------------------- rgda_sgd_step
def _f32(x):
    return float(np.float32(x))


@pytest.mark.parametrize('c', O.SGD_CASES, ids=[c.name for c in O.SGD_CASES])
def test_sgd_step(ops, c):
    gen = _gen('sgd', c.name)
    n = c.n
    p = _filled(torch.randn(n, generator=gen, device=DEV))
    g = _filled(torch.randn(n, generator=gen, device=DEV) * c.gsig)
    v = _filled(torch.randn(n, generator=gen, device=DEV) * 0.3)
    if c.first:
        v.view.fill_(float('nan'))                  # the first step must not read the momentum buffer
    has_s, has_pb, has_sb = c.bufs != 'noshadow', c.bufs != 'nopb', c.bufs in ('all', 'nopb')
    s = _filled(p.view + 0.05 * torch.randn(n, generator=gen, device=DEV)) if has_s else None
    pb = Arena(n, BF) if has_pb else None
    sb = Arena(n, BF) if has_sb else None
    gn, ws = torch.zeros(1, device=DEV), torch.empty(O.SUMSQ_CAP, device=DEV)
    ops.sumsq(g.view, gn, ws)                       # the norm word the step reads is the library's own
    lr = torch.tensor([O.SGD_LR], device=DEV)
    p0, g0, v0, s0 = p.view.clone(), g.view.clone(), v.view.clone(), (s.view.clone() if has_s else None)
    ops.sgd_step(p.view, g.view, v.view, s.view if has_s else None, pb.view if has_pb else None, gn, lr, O.SGD_MOMENTUM,
                 c.wd, c.max_norm, c.gscale, c.ema, c.first, shadow_bf16=sb.view if has_sb else None)
    torch.cuda.synchronize()
    coef, rel = O.coef_fp32(float(gn), c.gscale, c.max_norm)
    if c.clip in ('inactive', 'zero'):
        assert coef == c.gscale and rel == 0.0      # the clamp is taken: coef is gscale exactly
    else:
        assert coef < c.gscale
    vn, pn, sn, Ev, Ep, Es = O.sgd_reference(p0, g.view, v0, s0, coef, rel, _f32(float(lr)), _f32(O.SGD_MOMENTUM),
                                             _f32(c.wd), _f32(c.ema), c.first)
    assert bool(torch.isfinite(v.view).all()) and bool(torch.isfinite(p.view).all())
    _check('v', v.view, vn, Ev)
    _check('p', p.view, pn, Ep)
    if has_s:
        _check('shadow', s.view, sn, Es)
        if c.ema == 0:
            assert torch.equal(s.view, p.view)      # (1 - 0) p' + 0 s: the new weights bit for bit
        else:
            assert not torch.equal(s.view, p.view)
    # the bf16 mirrors: the rounding of the fp32 values the kernel stored
    if has_pb:
        assert torch.equal(O.bf16_canon(pb.view), O.bf16_bits(p.view))
    if has_sb:
        assert torch.equal(O.bf16_canon(sb.view), O.bf16_bits(s.view))
    assert torch.equal(g.view, g0) and all(a.intact() for a in (p, g, v, s, pb, sb) if a is not None)


def test_sgd_step_refusals(ops):
    n = 8
    t = [torch.zeros(n, device=DEV) for _ in range(4)]
    gn, lr = torch.ones(1, device=DEV), torch.ones(1, device=DEV)
    with pytest.raises(ValueError):
        ops.sgd_step(t[0][:6], t[1][:6], t[2][:6], None, None, gn, lr, 0.9, 0.0, 1.0, 1.0, 0.0, True)
    args = [t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), 0, 0, 0, gn.data_ptr(), lr.data_ptr(), n, 0.9, 0.0, 1.0,
            1.0, 0.0, 1]
    _raw('rgda_sgd_step', *args)                    # the optional buffers may be absent
    for i in (0, 1, 2, 6, 7):
        bad = list(args)
        bad[i] = 0
        with pytest.raises(ValueError):
            _raw('rgda_sgd_step', *bad)
    with pytest.raises(ValueError):
        _raw('rgda_sgd_step', *(args[:8] + [0] + args[9:]))


# ---------------------------------------------------------------- casts
def _cast_source(n):
    sp = O.cast_specials(DEV)
    if n < 2 * sp.numel():
        return sp.repeat(2)[7:7 + n].clone() if n > 3 else sp[4 - n:4].clone()
    x = torch.randn(n, generator=_gen('cast', n), device=DEV)
    x[:sp.numel()] = sp
    x[-sp.numel():] = sp.flip(0)                    # the last elements are the tail lanes' (n & 3)
    return x


@pytest.mark.parametrize('n', O.CAST_N)
def test_cast_bf16(ops, n):
    src = _filled(_cast_source(n))
    dst = Arena(n, BF)
    ops.cast_bf16(src.view, dst.view)
    assert torch.equal(O.bf16_canon(dst.view), O.bf16_bits(src.view))
    assert dst.intact() and src.intact()


def test_cast_bf16_special_values(ops):
    """+-0, +-inf, NaN stays NaN, ties to even in both directions, the largest finite fp32 -> inf; every special value
    passes through a vector lane and, as the length shrinks, through each tail lane."""
    sp = O.cast_specials(DEV)
    for n in (sp.numel(), sp.numel() - 1, sp.numel() - 2, sp.numel() - 3):
        for src in (sp[:n].clone(), sp[sp.numel() - n:].clone()):
            dst = Arena(n, BF)
            ops.cast_bf16(src, dst.view)
            assert torch.equal(O.bf16_canon(dst.view), O.bf16_bits(src)) and dst.intact()
    dst = Arena(sp.numel(), BF)
    ops.cast_bf16(sp, dst.view)
    got = dict(zip(O.CAST_SPECIALS_BITS, O.bf16_canon(dst.view).tolist()))
    assert got[0x3F808000] == 0x3F80 and got[0x3F818000] == 0x3F82 and got[0x7F7FFFFF] == 0x7F80, got
    assert got[0x7FC00000] == O.BF16_NAN and got[0x80000000] == 0x8000 and got[0xFF800000] == 0xFF80, got


@pytest.mark.parametrize('n', O.CASTF32_N)
def test_cast_f32(ops, n):
    bits = torch.randint(0, 65536, (n,), generator=_gen('castf32', n), device=DEV, dtype=torch.int32)
    m = min(n, 65536)
    bits[:m] = torch.arange(65536, device=DEV, dtype=torch.int32)[65536 - m:]      # every pattern, NaN payloads included
    src = _filled(O.bf16_from_bits(bits))
    dst = Arena(n, torch.float32)
    ops.cast_f32(src.view, dst.view)
    assert torch.equal(dst.view.view(torch.int32), bits << 16)      # a widening is a shift: exact for every pattern
    assert dst.intact() and src.intact()


# ---------------------------------------------------------------- rgda_ddp_accumulate_bf16
@pytest.mark.parametrize('world,s,order', O.DDP_CASES)
def test_ddp_accumulate_bf16(ops, world, s, order):
    recv = _filled(O.ddp_input(world, s, order, DEV))
    out = Arena(s, BF)
    ops.ddp_accumulate_bf16(recv.view, world, out.view)
    ref = O.ddp_reference_bits(recv.view.view(world, s), world)
    assert torch.equal(O.bf16_canon(out.view), ref)
    if order:
        assert not torch.equal(ref, O.ddp_reference_bits(recv.view.view(world, s), world, descending=True))
    assert out.intact() and recv.intact()


def test_ddp_accumulate_bf16_refuses_ragged_shards(ops):
    recv, out = torch.zeros(2, 16, dtype=BF, device=DEV), torch.zeros(16, dtype=BF, device=DEV)
    with pytest.raises(ValueError):
        ops.ddp_accumulate_bf16(recv, 2, out[:12])
    with pytest.raises(ValueError):
        ops.ddp_accumulate_bf16(recv, 0, out)


# ---------------------------------------------------------------- rgda_weight_transpose_batched
def _up(x, m):
    return -(-x // m) * m


@pytest.mark.parametrize('name', list(O.LAYOUT_TABLES))
def test_weight_layout_tables(ops, name):
    """One launch per table.  Sources and destinations are laid out back to back inside one source arena per type and one
    destination arena, each on a 16-byte boundary plus its row's offset; the WHOLE destination arena is compared, so a
    write outside a row's destination shows as a changed sentinel or a changed neighbour."""
    rows = O.LAYOUT_TABLES[name]
    gen = _gen('layout', name)
    first, total = O.layout_first_blocks(rows)
    spos, n32, n16 = [], 0, 0
    for r in rows:
        size = r.Co * r.T * r.ld
        if r.src16:
            spos.append(n16)
            n16 += _up(size, 8) + 8
        else:
            spos.append(n32)
            n32 += _up(size, 8) + 8
    src32 = _filled(torch.randn(max(n32, 1), generator=gen, device=DEV))
    src16 = _filled(torch.randn(max(n16, 1), generator=gen, device=DEV).to(BF))
    dpos, nd = [], 0
    for r in rows:
        dpos.append(nd + r.dst_off)
        nd += _up(r.dst_off + r.Co * r.T * r.Ci, 8) + 8
    # room behind the last destination for one whole source row stride per destination row: indexing a destination with
    # a source stride (a mistake the table invites) still lands inside the allocation
    dst = Arena(nd, BF, tail=GUARD + max(r.Co * r.T * r.ld for r in rows))
    expect = O.bf16_canon(dst.full)
    table = []
    for r, f, sp, dp in zip(rows, first, spos, dpos):
        arena = src16 if r.src16 else src32
        src = arena.view[sp:sp + r.Co * r.T * r.ld].view(r.Co, r.T, r.ld)
        assert src.data_ptr() % 16 == 0 and (dst.view.data_ptr() + 2 * (dp - r.dst_off)) % 16 == 0
        table.append([src.data_ptr() + r.off * src.element_size(), dst.view.data_ptr() + 2 * dp, r.Co, r.T, r.Ci, f, r.ld,
                      r.mode | (O.LAYOUT_SRC16 if r.src16 else 0)])
        expect[dst.lo + dp:dst.lo + dp + r.Co * r.T * r.Ci] = O.layout_reference_bits(src, r).reshape(-1)
    tab = torch.tensor(table, dtype=torch.int64, device=DEV)
    ops.weight_transpose_batched(tab, len(rows), total)
    got = O.bf16_canon(dst.full)
    if not torch.equal(got, expect):
        for i, (r, dp) in enumerate(zip(rows, dpos)):
            sl = slice(dst.lo + dp, dst.lo + dp + r.Co * r.T * r.Ci)
            assert torch.equal(got[sl], expect[sl]), 'row %d %r (%s)' % (i, r, O.layout_fallback_reasons(r) or 'vec')
        raise AssertionError('a write outside every destination: %d elements changed' % int((got != expect).sum()))
    assert src32.intact() and src16.intact()


def test_weight_layout_refusals(ops):
    tab = torch.zeros(1, 8, dtype=torch.int64, device=DEV)
    for n, blocks in ((0, 1), (1, 0), (1, 2 ** 31)):
        with pytest.raises(ValueError):
            ops.weight_transpose_batched(tab, n, blocks)


# ---------------------------------------------------------------- stem pad / unpad
@pytest.mark.parametrize('R,K,Kp', O.PAD_CASES)
def test_pad_cast_and_unpad_acc(ops, R, K, Kp):
    gen = _gen('pad', R, K, Kp)
    src = _filled(torch.randn(R * K, generator=gen, device=DEV))
    dst = Arena(R * Kp, BF)
    ops.pad_cast_bf16(src.view, dst.view, R, K, Kp)
    ref = torch.zeros(R, Kp, dtype=torch.int32, device=DEV)
    ref[:, :K] = O.bf16_bits(src.view).view(R, K)
    assert torch.equal(O.bf16_canon(dst.view).view(R, Kp), ref)
    assert dst.intact() and src.intact()
    # dst[R][K] += src[R][Kp][:K]: ONE fp32 add onto a destination that is not zero
    wide = _filled(torch.randn(R * Kp, generator=gen, device=DEV))
    acc = _filled(torch.randn(R * K, generator=gen, device=DEV))
    before = acc.view.clone()
    ops.unpad_acc_f32(wide.view, acc.view, R, K, Kp)
    want = before.view(R, K) + wide.view.view(R, Kp)[:, :K]
    assert torch.equal(O.f32_canon(acc.view.view(R, K)), O.f32_canon(want)) and not torch.equal(acc.view, before)
    assert acc.intact() and wide.intact()


# ---------------------------------------------------------------- rgda_fill_zero
@pytest.mark.parametrize('nbytes', O.FILL_BYTES)
def test_fill_zero_bytes(nbytes):
    a = Arena(nbytes, torch.uint8)
    _raw('rgda_fill_zero', a.full.data_ptr() + a.lo, nbytes)
    assert bool((a.view == 0).all()) and a.intact()         # the byte after the end is untouched


@pytest.mark.parametrize('dtype,n', [('bfloat16', 8 * O.K + 3), ('int64', 2 * O.K + 1), ('uint8', 16 * O.K + 5),
                                     ('bfloat16', 3), ('int64', 1)])
def test_fill_zero_tensors(ops, dtype, n):
    a = Arena(n, getattr(torch, dtype))
    ops.fill_zero(a.view)
    assert bool((a.view.view(torch.uint8) == 0).all()) and a.intact()


def test_fill_zero_refuses_a_misaligned_pointer(ops):
    a = Arena(64, torch.uint8, off=1)
    with pytest.raises(ValueError):
        ops.fill_zero(a.view)
    assert _is_poison(a.full)
    with pytest.raises(ValueError):
        _raw('rgda_fill_zero', 0, 16)


# ---------------------------------------------------------------- rgda_copy_multi
def _copy_raw(dsts, srcs, sizes):
    n = len(sizes)
    D, S, B = (ctypes.c_void_p * n)(*dsts), (ctypes.c_void_p * n)(*srcs), (ctypes.c_size_t * n)(*sizes)
    _raw('rgda_copy_multi', n, ctypes.cast(D, ctypes.c_void_p), ctypes.cast(S, ctypes.c_void_p), ctypes.cast(B, ctypes.c_void_p))


@pytest.mark.parametrize('sizes', O.COPY_CASES, ids=['-'.join(map(str, s)) for s in O.COPY_CASES])
def test_copy_multi(ops, sizes):
    gen = _gen('copy', sizes)
    srcs = [_filled(torch.randint(0, 256, (b,), generator=gen, device=DEV, dtype=torch.uint8)) for b in sizes]
    dsts = [Arena(b, torch.uint8) for b in sizes]
    if all(sizes):
        ops.copy_multi([(d.view, s.view) for d, s in zip(dsts, srcs)])
    else:               # a zero-length job: torch gives an empty tensor no address, the entry point itself admits it
        _copy_raw([d.full.data_ptr() + d.lo for d in dsts], [s.full.data_ptr() + s.lo for s in srcs], sizes)
    for k, (d, s) in enumerate(zip(dsts, srcs)):
        assert torch.equal(d.view, s.view), 'job %d of %r' % (k, sizes)
        assert d.intact() and s.intact(), 'job %d of %r' % (k, sizes)


def test_copy_multi_refusals(ops):
    a, b = Arena(64, torch.uint8), Arena(64, torch.uint8)
    pair = (a.view[:16], b.view[:16])
    with pytest.raises(ValueError):
        ops.copy_multi([pair] * 5)
    with pytest.raises(ValueError):
        ops.copy_multi([(a.view[1:17], b.view[:16])])
    with pytest.raises(ValueError):
        ops.copy_multi([(a.view[:16], b.view[1:17])])
    with pytest.raises(ValueError):
        ops.copy_multi([pair, (a.view[16:40], b.view[16:40])])
    assert _is_poison(a.full)


# ---------------------------------------------------------------- rgda_dropout_mask
@pytest.mark.parametrize('p,seed,n', O.DROPOUT_CASES)
def test_dropout_mask(ops, p, seed, n):
    out = Arena(n, torch.float32)
    ops.dropout_mask(out.view, p, seed)
    ref = torch.from_numpy(O.dropout_reference(n, p, seed)).to(DEV)
    assert torch.equal(out.view.view(torch.int32), ref.view(torch.int32))
    assert out.intact()


def test_dropout_mask_refusals(ops):
    out = torch.zeros(8, device=DEV)
    for p in (1.0, -0.1, float('nan'), 1.5):
        with pytest.raises(ValueError):
            ops.dropout_mask(out, p, 1)


# ---------------------------------------------------------------- rgda_add_bf16
@pytest.mark.parametrize('M,C,lds', O.ADD_CASES)
def test_add_bf16(ops, M, C, lds):
    """No call site in regda_amd/models/Encoder.py aliases the output with an operand (the entry point has no caller
    there at all), so there is no aliased case."""
    gen = _gen('add', M, C)
    bufs = []
    for ld in lds[:2]:
        a = _filled(torch.randn(M * ld, generator=gen, device=DEV).to(BF))
        bufs.append(a)
    o = Arena(M * lds[2], BF)
    a, b = (x.view.view(M, ld)[:, :C] for x, ld in zip(bufs, lds))
    ops.add_bf16(a, b, o.view.view(M, lds[2])[:, :C], M, C)
    got = O.bf16_canon(o.full)
    ref = O.bf16_bits(a.float() + b.float())            # one fp32 add, one rounding
    body = torch.full((M, lds[2]), 0xA5A5, dtype=torch.int32, device=DEV)
    body[:, :C] = ref
    assert torch.equal(got[o.lo:o.lo + o.n].view(M, lds[2]), body)      # the pad columns of the output rows too
    assert o.intact() and all(x.intact() for x in bufs)
    with pytest.raises(ValueError):
        ops.add_bf16(a, b, o.view.view(M, lds[2])[:, :C], M, C + 4)


# ---------------------------------------------------------------- the model's weight-layout bookkeeping
def _build(rt, head, ncls):
    from regda_amd.models.Encoder import Deeplabv2
    cfg = dict(backbone=dict(resnet_type=rt, output_stride=16, pretrained=False), multi_layer=True, cascade=False,
               use_ppm=head == 'ppm', inchannels=2048, num_classes=ncls, is_ins_norm=True)
    if head == 'ppm':
        cfg['ppm'] = dict(num_classes=ncls, use_aux=False, fc_dim=2048)
    return Deeplabv2(cfg)


def _owner(ptr, tensors):
    for t in tensors:
        if t.data_ptr() <= ptr < t.data_ptr() + t.numel() * t.element_size():
            return t, (ptr - t.data_ptr()) // t.element_size()
    raise AssertionError('a table pointer outside every buffer of the model')


def _check_table(m, table, blocks, where):
    """Decode every row (pointer -> offset into flat_p / flat_pb, shape, leading dimension, mode) and compare its
    destination with the permuted slice of the source, bit for bit."""
    dsts = [m.flat_wt] + ([m.aspp_wz] if m.head_kind == 'aspp' else
                          [t for hw in m.head_w.values() for t in [hw['wfeat']] + hw['wz'] + hw['wzt']])
    blk = 0
    for i, (src, dst, Co, T, Ci, first, ld, mode) in enumerate(table.cpu().tolist()):
        assert first == blk, (where, i)
        blk += O.layout_blocks(Co, Ci, T)
        s, soff = _owner(src, [m.flat_pb] if mode & O.LAYOUT_SRC16 else [m.flat_p])
        assert soff + (Co * T - 1) * ld + Ci <= s.numel()
        sl = torch.as_strided(s, (Co, T, Ci), (T * ld, ld, 1), soff)
        ref = O.bf16_bits({0: sl.permute(2, 1, 0), 1: sl.permute(1, 0, 2), 2: sl}[mode & 15].float().contiguous()).reshape(-1)
        d, doff = _owner(dst, dsts)
        assert doff + Co * T * Ci <= d.numel()
        got = O.bf16_canon(d.reshape(-1)[doff:doff + Co * T * Ci])
        assert torch.equal(got, ref), '%s: row %d (Co %d T %d Ci %d ld %d mode %d) is stale' % (where, i, Co, T, Ci, ld, mode)
    assert blk == blocks, where


def _check_model(m, where, derived=True, transposes=True):
    assert torch.equal(O.bf16_canon(m.flat_pb), O.bf16_bits(m.flat_p)), where + ': bf16 mirror'
    if not derived:
        return
    stem = m.convs['encoder.resnet.conv1'].w.reshape(64, 147)
    ref = torch.zeros(64, 192, dtype=torch.int32, device=DEV)
    ref[:, :147] = O.bf16_bits(stem.contiguous())
    assert torch.equal(O.bf16_canon(m.stem_wb).view(64, 192), ref), where + ': stem_wb'
    _check_table(m, m._hw_fwd_table, m._hw_fwd_blocks, where + ' _hw_fwd_table')
    if transposes:
        _check_table(m, m._wt_table, m._wt_blocks, where + ' _wt_table')
        if m.head_kind == 'aspp':
            assert torch.equal(m.aspp_wzt.view(2048, m.aspp_zc), m.aspp_wz.view(m.aspp_zc, 2048).t()), where + ': aspp_wzt'
        else:
            _check_table(m, m._hw_bwd_table, m._hw_bwd_blocks, where + ' _hw_bwd_table')


@pytest.mark.parametrize('head,ncls', [('ppm', 6), ('ppm', 7), ('aspp', 6), ('aspp', 7)])
def test_model_weight_copies_follow_the_master(head, ncls, monkeypatch):
    from oracle import model as omodel
    from regda_amd.ssl import SSLStep
    from regda_amd.synthetic import make_batch
    rt = 'resnet17t'
    m = _build(rt, head, ncls)
    torch.cuda.synchronize()
    _check_model(m, 'constructed')
    m.load_state_dict(omodel.init_state_dict(rt, ncls, seed=8, head=head), strict=True)
    torch.cuda.synchronize()
    _check_model(m, 'loaded')
    st = SSLStep(m, torch.randn(ncls, 2048, generator=torch.Generator().manual_seed(3)), class_num=ncls, ema_decay=0.99)
    assert st.wgrad_stream is not None              # the transposed copies are rebuilt on the side stream
    torch.cuda.synchronize()
    _check_model(st.teacher, 'teacher made', transposes=False)
    assert torch.equal(st.teacher.flat_buf, m.flat_buf) and torch.equal(st.teacher.flat_nbt, m.flat_nbt)
    b = make_batch(b=2, size=64, classes=ncls, seed=3, with_soft=False)
    w0 = m.flat_p.clone()
    st.step(b['images_s'], b['label_s'], b['images_t'], None, b['regs_t'], 1e-3)
    # the next backward reads the transposed copies this step rebuilt on the side stream: it has to wait for THIS event
    ready = m._wt_ready
    assert ready is not None
    waited = []
    orig = torch.cuda.Stream.wait_event
    monkeypatch.setattr(torch.cuda.Stream, 'wait_event', lambda self, ev: (waited.append(ev), orig(self, ev))[1])
    st.step(b['images_s'], b['label_s'], b['images_t'], None, b['regs_t'], 1e-3)
    monkeypatch.undo()
    torch.cuda.synchronize()
    assert any(ev is ready for ev in waited), 'the backward did not wait for the transposed copies of the previous step'
    assert m._wt_ready is not ready
    assert not torch.equal(m.flat_p, w0)
    _check_model(m, 'after two steps')
    t = st.teacher
    _check_model(t, 'teacher after two steps', derived=False)       # rgda_sgd_step wrote its mirror
    assert not torch.equal(t.flat_p, m.flat_p)
    t.refresh_from_master(mirror_is_fresh=True)                     # as the next step's teacher forward does
    torch.cuda.synchronize()
    _check_model(t, 'teacher refreshed', transposes=False)
    assert not torch.equal(t.flat_buf, m.flat_buf)                  # the student's forward has moved on since the snapshot
    t.adopt_buffers(m)
    torch.cuda.synchronize()
    assert torch.equal(t.flat_buf, m.flat_buf) and torch.equal(t.flat_nbt, m.flat_nbt)
