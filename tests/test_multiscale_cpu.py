"""Multi-scale sliding-window inference without a GPU: the scaled size and the resampling formula of the kernels against
scipy.ndimage.zoom and F.interpolate, the argument checks of rgda_window_gather_scaled / rgda_scale_merge (RGDA_ERR_ARG
before any launch) and of predict_multiscale, and the scales= parameter of the functions that gained it."""
import inspect

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from regda_amd import _lib
from regda_amd.utils.tools import DEFAULT_SCALES, check_scales, predict_multiscale, scaled_size

ERR_ARG = -1
CASES = [(5, 7, 1.5), (8, 8, 0.75), (9, 6, 1.25), (11, 13, 1.3), (7, 7, 1.75)]


def resize_ac_f32(x, Hs, Ws):
    """resize_ac_kernel / window_gather_scaled_kernel / scale_merge_kernel restated in NumPy, every step rounded to fp32:
    s = (in - 1) / (out - 1) in fp32 (0 for out == 1), f = s * I, truncate, clamp the upper neighbour, then
    (1-ly) * ((1-lx) * a + lx * b) + ly * ((1-lx) * c + lx * d)."""
    f32 = np.float32
    H, W = x.shape[-2:]

    def axis(n_in, n_out):
        s = f32(n_in - 1) / f32(n_out - 1) if n_out > 1 else f32(0)
        f = (s * np.arange(n_out, dtype=f32)).astype(f32)
        i0 = np.minimum(f.astype(np.int64), n_in - 1)
        i1 = i0 + (i0 < n_in - 1)
        lam = (f - i0.astype(f32)).astype(f32)
        return i0, i1, lam
    ya, yb, ly = axis(H, Hs)
    xa, xb, lx = axis(W, Ws)
    ly, lx = ly[:, None], lx[None, :]
    my, mx = f32(1) - ly, f32(1) - lx
    x = x.astype(f32)
    top = (mx * x[..., ya[:, None], xa[None, :]]).astype(f32) + (lx * x[..., ya[:, None], xb[None, :]]).astype(f32)
    bot = (mx * x[..., yb[:, None], xa[None, :]]).astype(f32) + (lx * x[..., yb[:, None], xb[None, :]]).astype(f32)
    return ((my * top.astype(f32)).astype(f32) + (ly * bot.astype(f32)).astype(f32)).astype(f32)


@pytest.mark.parametrize('H,W,s', CASES)
def test_scaled_size_is_ndimage_zooms_output_shape(H, W, s):
    from scipy import ndimage
    z = ndimage.zoom(np.zeros((1, 1, H, W), np.float32), (1.0, 1.0, s, s), order=1, prefilter=False)
    assert scaled_size(H, W, s) == z.shape[2:]


def test_scaled_size_rounds_like_python():
    assert scaled_size(7, 5, 1.5) == (10, 8)               # 10.5 -> 10, 7.5 -> 8: round half to even
    assert scaled_size(512, 512, 1.0) == (512, 512) and scaled_size(6000, 6000, 0.75) == (4500, 4500)


@pytest.mark.parametrize('H,W,s', CASES)
def test_kernel_formula_is_zoom_and_align_corners_bilinear(H, W, s):
    from scipy import ndimage
    x = np.random.default_rng(H * 100 + W).standard_normal((2, 3, H, W)).astype(np.float32)
    Hs, Ws = scaled_size(H, W, s)
    got = resize_ac_f32(x, Hs, Ws)
    assert got.dtype == np.float32 and got.shape == (2, 3, Hs, Ws)
    zoom = ndimage.zoom(x, (1.0, 1.0, s, s), order=1, prefilter=False)
    np.testing.assert_allclose(got, zoom, rtol=0, atol=1e-5)
    ref = F.interpolate(torch.from_numpy(x), size=(Hs, Ws), mode='bilinear', align_corners=True).numpy()
    np.testing.assert_allclose(got, ref, rtol=0, atol=1e-5)
    back = resize_ac_f32(got, H, W)                        # ... and back, as the probabilities come
    ref = F.interpolate(torch.from_numpy(got), size=(H, W), mode='bilinear', align_corners=True).numpy()
    np.testing.assert_allclose(back, ref, rtol=0, atol=1e-5)


@pytest.fixture(scope='module')
def L():
    try:
        return _lib.lib()
    except ImportError as e:
        pytest.skip(str(e))


P = 0x1000      # a non-null pointer that is never dereferenced: every call below is refused before any launch


def test_window_gather_scaled_refuses_bad_arguments(L):
    g = L.raw('rgda_window_gather_scaled')
    ok = dict(f32=P, u8=None, lut=None, win=P, K=2, V=1, n=1, C=3, H=600, W=600, Hs=900, Ws=900, Th=512, Tw=512, out=P)

    def call(**kw):
        a = dict(ok, **kw)
        return g(a['f32'], a['u8'], a['lut'], a['win'], a['K'], a['V'], a['n'], a['C'], a['H'], a['W'], a['Hs'], a['Ws'],
                 a['Th'], a['Tw'], a['out'], None, None)
    for bad in (dict(f32=None), dict(u8=P), dict(u8=P, lut=P), dict(f32=None, u8=P), dict(f32=None, u8=P, lut=P, C=4),
                dict(win=None), dict(out=None), dict(K=0), dict(n=0), dict(C=0), dict(H=0), dict(W=0), dict(Hs=511),
                dict(Ws=100), dict(Th=0), dict(Tw=0), dict(V=2), dict(V=0), dict(V=8, Tw=256)):
        assert call(**bad) == ERR_ARG, bad
    # the source may be smaller than the tile: only the scaled image has to hold a window
    for bad in (dict(H=100, W=100, Hs=511), dict(H=100, W=100, Ws=511)):
        assert call(**bad) == ERR_ARG, bad


def test_scale_merge_refuses_bad_arguments(L):
    m = L.raw('rgda_scale_merge')
    ok = dict(full=P, count=P, n=1, C=6, Hs=12, Ws=12, H=8, W=8, acc=P, cnt=P)

    def call(**kw):
        a = dict(ok, **kw)
        return m(a['full'], a['count'], a['n'], a['C'], a['Hs'], a['Ws'], a['H'], a['W'], a['acc'], a['cnt'], None)
    for bad in (dict(full=None), dict(count=None), dict(acc=None), dict(cnt=None), dict(n=0), dict(C=0), dict(Hs=0),
                dict(Ws=0), dict(H=0), dict(W=0), dict(n=-1)):
        assert call(**bad) == ERR_ARG, bad


def test_new_entry_points_are_in_the_plan_dispatch_table(L):
    for name, nargs in (('rgda_window_gather_scaled', 17), ('rgda_scale_merge', 11)):
        assert len(L.protos[name][1]) == nargs
        assert L.raw('rgda_plan_fn_id')(name.encode()) >= 0


def test_predict_multiscale_refuses_bad_scales_before_any_launch():
    class NeverCalled:
        num_classes = 6

        def __call__(self, x):
            raise AssertionError('the model ran')
    img = torch.zeros(1, 3, 40, 40)             # on the host: anything past the checks would fail differently
    for bad in ((), [], (0.0,), (1.0, -0.5), (1.0, 0.0), (0.01,), (float('nan'),), (float('inf'),)):
        for wb in (16, None):
            with pytest.raises(ValueError):
                predict_multiscale(NeverCalled(), img, scales=bad, window_batch=wb)
    with pytest.raises(ValueError):             # 40 x 3 at 0.1: a 4 x 0 image
        predict_multiscale(NeverCalled(), torch.zeros(1, 3, 40, 3), scales=(1.0, 0.1))
    assert check_scales(40, 40, (0.75, 1.0, 1.5)) == [(30, 30), (40, 40), (60, 60)]
    assert check_scales(7, 5, DEFAULT_SCALES)[3] == (10, 8)


def test_signatures():
    from regda_amd.gast.pseudo_generation import gener_target_pseudo
    from regda_amd.utils.eval import evaluate
    from regda_amd.utils.infer import predict_scene
    for fn in (evaluate, gener_target_pseudo, predict_scene):
        p = inspect.signature(fn).parameters
        assert p['scales'].default is None and list(p)[-1] == 'scales', fn.__name__
    p = inspect.signature(predict_multiscale).parameters
    assert list(p) == ['model', 'image', 'scales', 'tile_size', 'num_classes', 'tta', 'window_batch']
    assert p['scales'].default == (0.75, 1.0, 1.25, 1.5, 1.75, 2.0) and p['tile_size'].default == (512, 512)
    assert p['window_batch'].default == 16 and p['num_classes'].default is None and p['tta'].default is False


def test_functions_with_scales_accept_none(tmp_path):
    """scales=None reaches the code each function ran before it had the parameter: the same errors, the same empty run."""
    from regda_amd.gast.metrics import PixelMetricIgnore  # noqa: F401  (evaluate's import chain loads without a GPU)
    from regda_amd.gast.pseudo_generation import gener_target_pseudo
    from regda_amd.utils.eval import evaluate
    from regda_amd.utils.infer import predict_scene

    class Model:
        num_classes = 6

        def eval(self):
            return self
    with pytest.raises(ValueError, match='dataloader'):
        evaluate(Model(), None, is_training=True, scales=None)
    with pytest.raises(ValueError, match='uint8'):
        predict_scene(Model(), np.zeros((8, 8, 3), np.float32), None, 6, scales=None)

    class Cfg:
        NUM_CLASSES = 6
    gener_target_pseudo(Cfg, Model(), [], str(tmp_path / 'none'), scales=None)         # an empty loader: no launch
    gener_target_pseudo(Cfg, Model(), [], str(tmp_path / 'none'), window_batch=4, scales=None)
    with pytest.raises(ValueError, match='slide'):
        gener_target_pseudo(Cfg, Model(), [], str(tmp_path / 'none'), slide=False, scales=(1.0,))
