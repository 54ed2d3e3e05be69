"""GPU: the stage-2 loss kernels of regda_amd/csrc/align_kernels.hip and the ASPP head kernels of aspp_kernels.hip on every
case of tests/align_cases.py, per element against the plain references there.  Flag words, sentinel columns, the ASPP
gather and the scatter must match bit for bit; the PCL loss and gradient and dbias are bounded per element by
tests/golden/head_tolerances.json, which tests/golden/derive_head_tolerances.py derives on the CPU from an fp32 oracle's own
deviation from the fp64 reference (never from a kernel's output), plus the analytic bf16 storage term 2^-8 |ref| of the
gradient.  tests/test_align_cases_cpu.py checks, without a GPU, that each case reaches the path it names and that the
references agree with the oracles."""
import json
import os

import numpy as np
import pytest
import torch

import align_cases as A

pytestmark = pytest.mark.gpu
TOL = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'head_tolerances.json')))
BF = torch.bfloat16


@pytest.fixture(scope='module')
def ops():
    from regda_amd import ops
    return ops


def cu(a):
    return torch.as_tensor(a).contiguous().cuda()


def _ids(cases):
    return [c.name for c in cases]


def _check(name, got, ref, bound):
    """Every element within its bound (a scalar or an array of the same shape); prints the largest difference."""
    d = np.atleast_1d(np.abs(np.asarray(got, np.float64) - np.asarray(ref, np.float64)))
    bound = np.broadcast_to(np.asarray(bound, np.float64), d.shape)
    off = ~(d <= bound)
    i = np.unravel_index(np.argmax(d - bound), d.shape)
    print('%s: max |diff| %.3e; tightest element: |diff| %.3e, bound %.3e' % (name, d.max(), d[i], bound[i]))
    assert not off.any(), '%s: %d of %d off; worst |diff| %.3e against bound %.3e' % (name, off.sum(), d.size, d[i], bound[i])


def _bits(t):
    return t.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


def _from_bits(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int16)).cuda().view(BF)


# ---------------------------------------------------------------- PrototypeContrastiveLoss
def _pcl_run(ops, case, x, old=None):
    """One call through ops.pcl_loss with a workspace and a gradient buffer of the test's own -> (loss, grad (b, hw, K)
    as fp32 numpy, flag word, the columns [K, lddf) as bits).  The workspace starts as 0xff bytes and the gradient, where
    it is not accumulated onto, as 7.0: the call has to clear the one and overwrite the other."""
    from regda_amd._lib import lib
    b, K, C, hw = case.b, case.K, case.C, case.h * case.w
    ld = case.lddf or K
    buf = _from_bits(np.full((b * hw, ld), A.SENTINEL_BITS, np.uint16))
    buf[:, :K] = 7.0 if old is None else cu(old.reshape(b * hw, K)).to(BF)
    ws = torch.full((lib().size('rgda_pcl_loss_workspace', C, K),), 255, dtype=torch.uint8, device='cuda')
    assert ws.numel() == A.pcl_workspace(C, K)
    loss = torch.full((1,), case.loss0, device='cuda')
    out = ops.pcl_loss(cu(x['feat']), cu(x['lab']), cu(x['protos']), case.temp, case.ignore, case.weight, loss=loss,
                       dfeat=buf[:, :K], accumulate=old is not None, ws=ws)
    assert out is loss
    flag = ops.pcl_flag(ws, C, K)
    off = A.pcl_flag_offset(C, K)
    assert flag == int(ws[off:off + 4].view(torch.int32).item())
    return float(loss.item()), buf[:, :K].float().cpu().numpy().reshape(b, hw, K), flag, _bits(buf)[:, K:]


def _grad_bound(case, ref, total=None):
    """The derived fp32 bound plus the bf16 storage term 2^-8 |stored value| per element."""
    t = TOL['pcl'][case.name]
    bound = t['grad']['bound'] + 2.0 ** -8 * np.abs(ref if total is None else total)
    if case.special == 'zero_pixel':
        p = A.DEGENERATE_PIXEL
        bound[0, p] = t['grad_row']['bound'] + 2.0 ** -8 * np.abs((ref if total is None else total)[0, p])
    return bound


@pytest.mark.parametrize('case', A.PCL_FINITE, ids=_ids(A.PCL_FINITE))
def test_pcl_loss_and_gradient(ops, case):
    x = A.pcl_inputs(case)
    loss, grad, kept, flag = A.pcl_ref(x['feat'], x['protos'], x['lab'], case.temp, case.ignore, case.weight)
    got_loss, got, got_flag, tail = _pcl_run(ops, case, x)
    assert got_flag == flag == (A.FLAG_LABEL if case.special == 'bad_labels' else 0)
    _check(case.name + ' loss', got_loss, case.loss0 + loss, TOL['pcl'][case.name]['loss']['bound'])
    _check(case.name + ' grad', got, grad, _grad_bound(case, grad))
    assert not got[~kept].any()                                  # ignored and out-of-range pixels: exactly zero
    assert (tail == A.SENTINEL_BITS).all()
    if case.lddf:                                                # the same case accumulating onto a gradient
        old = A.accumulate_old(grad, case.name)
        l2, got2, f2, tail2 = _pcl_run(ops, case, x, old)
        total = old.astype(np.float64) + grad
        _check(case.name + ' accumulate', got2, total, _grad_bound(case, grad, total))
        assert np.array_equal(got2[~kept], old[~kept]) and (tail2 == A.SENTINEL_BITS).all() and l2 == got_loss and f2 == flag
    # the loss alone (dfeat = NULL) is the same number
    only = ops.pcl_loss(cu(x['feat']), cu(x['lab']), cu(x['protos']), case.temp, case.ignore, case.weight,
                        loss=torch.full((1,), case.loss0, device='cuda'))
    assert float(only.item()) == got_loss


def test_pcl_none_kept(ops):
    case = next(c for c in A.PCL_CASES if c.name == 'none_kept')
    x = A.pcl_inputs(case)
    got_loss, got, flag, _ = _pcl_run(ops, case, x)
    print('none_kept: loss %r, max |grad| %g, flag %d' % (got_loss, np.abs(got).max(), flag))
    assert np.isnan(got_loss) and not got.any() and flag == 0


NONFINITE = [c for c in A.PCL_CASES if 'nonfinite' in c.paths]


@pytest.mark.parametrize('case', NONFINITE, ids=_ids(NONFINITE))
def test_pcl_nonfinite_feature(ops, case):
    """A NaN or Inf feature in a kept pixel: the loss is NaN for any number of such pixel blocks (before the flag bit of
    pcl_kernel, one block read 3145728.0 + the healthy sum -- 3 * 2^60 in the 2^-40 fixed point -- and sixteen or
    thirty-two wrapped the 64-bit total back to the healthy sum alone), that pixel's gradient row is non-finite, and
    every other pixel keeps its reference gradient."""
    x = A.pcl_inputs(case)
    loss, grad, kept, _ = A.pcl_ref(x['feat'], x['protos'], x['lab'], case.temp, case.ignore, case.weight)
    bad = ~np.isfinite(x['feat'].reshape(case.b, case.K, -1)).all(1)
    got_loss, got, flag, _ = _pcl_run(ops, case, x)
    print('%s: loss %r (reference %r), flag %d, %d non-finite pixels in %d blocks' %
          (case.name, got_loss, loss, flag, bad.sum(), A.cdiv(case.h * case.w, A.PX)))
    assert np.isnan(loss) and np.isnan(got_loss)
    assert flag == A.FLAG_NONFINITE
    assert not np.isfinite(got[bad]).any()
    _check(case.name + ' other rows', got[~bad], grad[~bad], (TOL['pcl'][case.name]['grad']['bound'] + 2.0 ** -8 * np.abs(grad))[~bad])
    assert not got[~kept].any()


@pytest.mark.parametrize('ref', A.PCL_REFUSALS, ids=[r[0] for r in A.PCL_REFUSALS])
def test_pcl_refusals(ops, ref):
    """Every refusal answers as the restatement predicts and before anything is launched: the loss, the gradient buffer
    and the workspace (its count / flag / total words are cleared first thing otherwise) stay as they were."""
    from regda_amd._lib import lib
    name, C, K, ld, short = ref
    b, h, w = 1, 2, 2
    feat = torch.zeros(b * 4200 * h * w, device='cuda')
    lab = torch.zeros(b, h, w, dtype=torch.int64, device='cuda')
    protos = torch.ones(17 * 4200, device='cuda')
    loss = torch.full((1,), 3.0, device='cuda')
    df = torch.full((b * h * w * 4200,), 7.0, dtype=BF, device='cuda')
    ws = torch.full((1 << 20,), 255, dtype=torch.uint8, device='cuda')
    nbytes = A.pcl_workspace(C, K) - 1 if short else ws.numel()
    rc = lib().raw('rgda_pcl_loss')(feat.data_ptr(), lab.data_ptr(), protos.data_ptr(), loss.data_ptr(),
                                    df.data_ptr(), ld or K, 0, b, K, C, h, w, -1, 8.0, 1.0, ws.data_ptr(), nbytes, ops._stream())
    torch.cuda.synchronize()
    assert rc == A.pcl_status(C, K, ld or K, nbytes) != A.OK
    assert float(loss.item()) == 3.0 and bool((ws == 255).all()) and bool((df == 7.0).all())


# ---------------------------------------------------------------- the ASPP head
def _aspp_buffer(case, bits=None):
    """A bf16 [M][ld] buffer of sentinels and its [M][zc] column slice, holding `bits` when given."""
    zc, ld, off = A.aspp_width(case)
    M = case.N * case.h * case.w
    full = np.full((M, ld), A.ASPP_SENTINEL_BITS, np.uint16)
    if bits is not None:
        full[:, off:off + zc] = bits
    buf = _from_bits(full)
    return buf, buf[:, off:off + zc]


@pytest.mark.parametrize('case', A.ASPP_CASES, ids=_ids(A.ASPP_CASES))
def test_aspp_gather(ops, case):
    x = A.aspp_inputs(case)
    N, h, w, C = case.N, case.h, case.w, case.C
    buf, z = _aspp_buffer(case, x['z'])
    o1 = torch.full((N, C, h, w), 7.0, device='cuda')
    o2 = torch.full((N, C, h, w), 7.0, device='cuda')
    ops.aspp_gather(z, [cu(b) for b in x['biases']], o1, o2, N, h, w, C, case.dils)
    r1, r2 = A.gather_ref(x['z'], x['biases'], N, h, w, C, case.dils)
    for name, got, ref in (('head 1', o1, r1), ('head 2', o2, r2)):
        g = got.cpu().numpy()
        print('%s %s: max |diff| %.3e (bit for bit)' % (case.name, name, np.abs(g.astype(np.float64) - ref).max()))
        assert np.array_equal(g.view(np.uint32), ref.view(np.uint32)), (case.name, name)
    assert not np.array_equal(r1, r2)


@pytest.mark.parametrize('case', A.ASPP_CASES, ids=_ids(A.ASPP_CASES))
def test_aspp_scatter_and_dbias(ops, case):
    x = A.aspp_inputs(case)
    N, h, w, C = case.N, case.h, case.w, case.C
    zc, ld, off = A.aspp_width(case)
    buf, dz = _aspp_buffer(case)
    dbs = [cu(b).clone() for b in x['dbias0']]
    ops.aspp_scatter(cu(x['g1']), cu(x['g2']), dz, dbs, N, h, w, C, case.dils)
    got = _bits(buf)
    ref = A.scatter_ref(x['g1'], x['g2'], N, h, w, C, case.dils, zc)
    wrong = got[:, off:off + zc] != ref
    print('%s: %d of %d elements of dz differ' % (case.name, wrong.sum(), wrong.size))
    assert not wrong.any(), np.argwhere(wrong)[:8]
    assert not got[:, off + A.aspp_columns(C):off + zc].any()                       # the pad columns
    assert (got[:, :off] == A.ASPP_SENTINEL_BITS).all() and (got[:, off + zc:] == A.ASPP_SENTINEL_BITS).all()
    r64 = A.dbias_ref(x['g1'], x['g2'], x['dbias0'])
    outs = np.stack([d.cpu().numpy() for d in dbs])
    _check(case.name + ' dbias', outs, np.stack(r64), TOL['dbias'][case.name]['bound'])
    delta = outs - np.stack(x['dbias0'])                         # the four dilations of a head add the same fp32 total
    assert not np.allclose(delta[0], delta[4])
