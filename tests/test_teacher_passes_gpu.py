"""GPU: every kernel of regda_amd/csrc/teacher_kernels.hip on every case of tests/teacher_cases.py, per element against the
plain references there.  Permutations, crops, pads, the window sums, the fp32 division, argmax and the confusion matrix
must match exactly; the dihedral scale-and-accumulate is bounded by two fp32 roundings and the resize by
tests/golden/head_tolerances.json (tests/golden/derive_head_tolerances.py: three times F.interpolate's own fp32 deviation
from the fp64 reference, never a kernel's output).  tests/test_teacher_cases_cpu.py checks, without a GPU, that each case
reaches the path it names and that the references agree with the oracles."""
import json
import os

import numpy as np
import pytest
import torch

import teacher_cases as T

pytestmark = pytest.mark.gpu
TOL = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'head_tolerances.json')))


@pytest.fixture(scope='module')
def ops():
    from regda_amd import ops
    return ops


def cu(a):
    return torch.as_tensor(a).contiguous().cuda()


def _same(name, got, ref):
    """Bit for bit (NaN in the same places)."""
    got = got.cpu().numpy() if torch.is_tensor(got) else got
    assert got.shape == ref.shape and got.dtype == ref.dtype, (name, got.shape, ref.shape, got.dtype, ref.dtype)
    wrong = ~((got == ref) | (np.isnan(got) & np.isnan(ref))) if got.dtype.kind == 'f' else got != ref
    print('%s: %d of %d elements differ' % (name, wrong.sum(), wrong.size))
    assert not wrong.any(), (name, np.argwhere(wrong)[:8])


def _check(name, got, ref, bound):
    d = np.abs(got.cpu().numpy().astype(np.float64) - np.asarray(ref, np.float64))
    bound = np.broadcast_to(np.asarray(bound, np.float64), d.shape)
    i = np.unravel_index(np.argmax(d - bound), d.shape)
    print('%s: max |diff| %.3e; tightest element: |diff| %.3e, bound %.3e' % (name, d.max(), d[i], bound[i]))
    n = int((~(d <= bound)).sum())
    assert n == 0, '%s: %d of %d off; |diff| %.3e against bound %.3e' % (name, n, d.size, d[i], bound[i])


# ---------------------------------------------------------------- dihedral
@pytest.mark.parametrize('shape', T.DIHEDRAL_SHAPES, ids=str)
def test_dihedral_all_sixteen_views(ops, shape):
    src = T.index_image(shape)
    g = cu(src)
    for f, k, ff in T.VIEWS:
        out = ops.dihedral(g, f, k, ff)
        assert tuple(out.shape) == T.dihedral_shape(*shape, k)
        _same('%s view %s' % (shape, (f, k, ff)), out, T.dihedral_ref(src, f, k, ff))


@pytest.mark.parametrize('view', T.DIHEDRAL_BIG_VIEWS, ids=str)
def test_dihedral_second_trip(ops, view):
    """More than 65535 * 256 elements, an odd rotation, H != W: the elements of the loop's second trip are the last rows."""
    src = T.index_image(T.DIHEDRAL_BIG)
    out = ops.dihedral(cu(src), *view)
    _same('big view %s' % (view,), out, T.dihedral_ref(src, *view))


@pytest.mark.parametrize('view', [(0, 0, 1), (1, 1, 1), (1, 1, 0), (0, 3, 0), (1, 2, 1)], ids=str)
def test_dihedral_scale_and_accumulate(ops, view):
    shape = T.DIHEDRAL_SHAPES[-1]
    src, old = T.dihedral_acc_inputs(shape, view)
    ref, bound = T.dihedral_acc_ref(src, old, view, T.DIHEDRAL_SCALE)
    dst = cu(old).clone()
    ops.dihedral(cu(src), *view, dst=dst, scale=T.DIHEDRAL_SCALE, accumulate=True)
    _check('scale + accumulate %s' % (view,), dst, ref, bound)
    plain = ops.dihedral(cu(src), *view, scale=T.DIHEDRAL_SCALE)                   # scale alone: one rounding, one answer
    _same('scale %s' % (view,), plain, np.float32(T.DIHEDRAL_SCALE) * T.dihedral_ref(src, *view))


# ---------------------------------------------------------------- windows
@pytest.mark.parametrize('case', T.CROP_CASES, ids=[c.name for c in T.CROP_CASES])
def test_window_crop(ops, case):
    full = T.index_image(case.shape) + 1.0                       # no zero in the image: the padding is told apart
    out = ops.window_crop(cu(full), case.y1, case.x1, case.h, case.w, case.Th, case.Tw)
    _same(case.name, out, T.crop_ref(full, case))


@pytest.mark.parametrize('case', T.ACC_CASES, ids=[c.name for c in T.ACC_CASES])
def test_window_accumulate(ops, case):
    tiles, full, count = T.acc_inputs(case)
    rf, rc = T.acc_ref(tiles, full, count, case)
    gf, gc = cu(full).clone(), cu(count).clone()
    for t, (y1, x1, h, w) in zip(tiles, case.windows):
        ops.window_accumulate(cu(t), gf, gc, y1, x1, h, w)
    _same(case.name + ' full', gf, rf)                           # inside the windows and, bit-identical, outside them
    _same(case.name + ' count', gc, rc)


@pytest.mark.parametrize('shape', T.NORM_SHAPES + [T.NORM_BIG], ids=str)
def test_window_normalise(ops, shape):
    full, count = T.norm_inputs(shape)
    g = cu(full).clone()
    ops.window_normalise(g, cu(count))
    _same('normalise %s' % (shape,), g, T.norm_ref(full, count))


# ---------------------------------------------------------------- resize, pad
@pytest.mark.parametrize('shape,size', T.RESIZE_CASES, ids=[T.resize_name(*c) for c in T.RESIZE_CASES])
def test_resize_bilinear_ac(ops, shape, size):
    x = T.resize_inputs(shape, size)
    out = ops.resize_bilinear_ac(cu(x), size)
    assert tuple(out.shape) == shape[:2] + size
    _check(T.resize_name(shape, size), out, T.resize_ref(x, size).numpy(), TOL['resize'][T.resize_name(shape, size)]['bound'])


@pytest.mark.parametrize('top,bottom', T.PAD_CASES)
def test_pad_rows(ops, top, bottom):
    x = T.index_image(T.PAD_SHAPE) + 1.0
    _same('pad (%d, %d)' % (top, bottom), ops.pad_rows(cu(x), top, bottom), T.pad_ref(x, top, bottom))


# ---------------------------------------------------------------- argmax, confusion matrix
@pytest.mark.parametrize('name,x', T.argmax_cases(), ids=[c[0] for c in T.argmax_cases()])
def test_argmax_nchw(ops, name, x):
    out = ops.argmax_nchw(cu(x))
    assert out.dtype == torch.int64
    _same(name, out, T.argmax_ref(x))


@pytest.mark.parametrize('case', T.CONF_CASES, ids=[c.name for c in T.CONF_CASES])
def test_confusion_accumulate(ops, case):
    yt, yp = T.conf_inputs(case)
    ref, flag = T.conf_ref(yt, yp, case.C)
    cm = torch.full((case.C, case.C), T.CONF_CM0, dtype=torch.int64, device='cuda')
    fl = torch.full((1,), T.CONF_FLAG0, dtype=torch.int32, device='cuda')
    if case.n == 0:                                              # an empty tensor has no pointer: n = 0 over a real buffer
        from regda_amd._lib import lib
        some = torch.full((8,), case.C, dtype=torch.int64, device='cuda')         # out of range, were it looked at
        lib().call('rgda_confusion_accumulate', some.data_ptr(), some.data_ptr(), cm.data_ptr(), fl.data_ptr(), 0, case.C,
                   ops._stream())
    else:
        ops.confusion_accumulate(cu(yt), cu(yp), cm, fl)
    _same(case.name, cm, ref)
    assert int(fl.item()) == flag


def test_confusion_refuses_65_classes(ops):
    from regda_amd._lib import lib
    y = torch.zeros(8, dtype=torch.int64, device='cuda')
    cm = torch.zeros(65, 65, dtype=torch.int64, device='cuda')
    fl = torch.zeros(1, dtype=torch.int32, device='cuda')
    rc = lib().raw('rgda_confusion_accumulate')(y.data_ptr(), y.data_ptr(), cm.data_ptr(), fl.data_ptr(), 8, 65, ops._stream())
    torch.cuda.synchronize()
    assert rc == T.confusion_status(8, 65) == T.ERR_ARG and not cm.any() and int(fl.item()) == 0
    with pytest.raises(ValueError):
        ops.confusion_accumulate(y, y, cm, fl)
