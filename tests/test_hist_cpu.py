"""No GPU: the numpy / integer restatement of the histogram matching (tests/hist_ref.py) against the textbook
np.unique / np.interp formulation and on its special cases, the host side (HistogramStyle's draws and state), and the
refusals of the three entry points, which come before any launch."""
import ctypes

import numpy as np
import pytest

import hist_ref
from hist_ref import MEAN, STD

NEW = {'rgda_hist_style': 25, 'rgda_hist_style_write_table': 7, 'rgda_hist_style_workspace': 4}


# ---- the restatement
def interp_lut(src, tgt):
    """scikit-image's match_histograms on two integer planes: {source level: matched level}"""
    sv, sc = np.unique(src.ravel(), return_counts=True)
    tv, tc = np.unique(tgt.ravel(), return_counts=True)
    got = np.interp(np.cumsum(sc) / src.size, np.cumsum(tc) / tgt.size, tv)
    return dict(zip(sv.tolist(), got.tolist()))


def test_the_restatement_is_the_unique_interp_formulation_on_random_pairs():
    rng = np.random.default_rng(7)
    worst, seen = 0.0, set()
    for trial in range(200):
        h, w = (1, 1) if trial == 0 else (40, 40) if trial == 1 else rng.integers(1, 41, 2)
        pools = []
        for _ in range(2):      # 1 to 256 occupied levels (as many as the plane has room for)
            k = 256 if trial == 1 else int(rng.integers(1, 257))
            pools.append(rng.choice(256, size=k, replace=False))
        if trial == 1:
            src, tgt = (np.concatenate([p, rng.choice(p, h * w - 256)]).reshape(h, w) for p in pools)
        else:
            src, tgt = (rng.choice(p, (h, w)) for p in pools)
        L = hist_ref.match_lut(hist_ref.histogram(src), hist_ref.histogram(tgt))
        want = interp_lut(src, tgt)
        seen.add(len(want))
        for v in range(256):
            if v in want:
                worst = max(worst, abs(L[v] - want[v]))
                assert abs(L[v] - want[v]) <= 1e-9, (trial, v, L[v], want[v])
            else:
                assert L[v] == float(v)
    print('200 pairs, 1 .. %d occupied source levels: max |L - interp| %.3e' % (max(seen), worst))
    assert min(seen) == 1 and max(seen) == 256


def test_special_cases_of_the_restatement():
    rng = np.random.default_rng(3)
    src = rng.integers(0, 256, (24, 31))
    hs = hist_ref.histogram(src)
    # a constant template: every occupied level becomes it
    L = hist_ref.match_lut(hs, hist_ref.histogram(np.full((24, 31), 77)))
    assert all(L[v] == 77.0 for v in range(256) if hs[v]) and all(L[v] == float(v) for v in range(256) if not hs[v])
    # a constant source: cs = HW, the template's top level
    tgt = rng.integers(10, 200, (24, 31))
    L = hist_ref.match_lut(hist_ref.histogram(np.full((24, 31), 5)), hist_ref.histogram(tgt))
    assert L[5] == float(tgt.max()) and all(L[v] == float(v) for v in range(256) if v != 5)
    # self-match: the identity, exactly
    assert hist_ref.match_lut(hs, hs) == [float(v) for v in range(256)]
    two = rng.choice([3, 250], (7, 9))
    assert hist_ref.match_lut(hist_ref.histogram(two), hist_ref.histogram(two)) == [float(v) for v in range(256)]
    # both end clamps: a first template level that holds more pixels than the lowest source levels (no j), and the top
    spike = np.full((24, 31), 128)
    spike.flat[-2:] = [254, 255]
    L = hist_ref.match_lut(hs, hist_ref.histogram(spike))
    lowest, top = min(v for v in range(256) if hs[v]), max(v for v in range(256) if hs[v])
    assert L[lowest] == 128.0 and L[top] == 255.0 and 128.0 <= min(L[v] for v in range(256) if hs[v])


def test_the_whole_transform_on_one_pair():
    rng = np.random.default_rng(5)
    ls, lt = rng.integers(0, 120, (2, 3, 9, 11)).astype(np.uint8), rng.integers(100, 256, (1, 3, 9, 11)).astype(np.uint8)
    xs, xt = hist_ref.tiles(ls, MEAN, STD, rng.uniform(-0.4, 0.4, ls.shape)), hist_ref.tiles(lt, hist_ref.MEAN_T, hist_ref.STD_T)
    assert np.array_equal(hist_ref.levels_of(xs, MEAN, STD), ls) and np.array_equal(hist_ref.levels_of(xt, hist_ref.MEAN_T, hist_ref.STD_T), lt)
    table = np.array([[0, 65536, 1, 0], [0, 65536, 0, 0]], np.int32)
    out, hist, lut = hist_ref.hist_ref(xs, xt, table, MEAN, STD, hist_ref.MEAN_T, hist_ref.STD_T)
    assert np.array_equal(out[1].view(np.int32), xs[1].view(np.int32)) and np.array_equal(lut[1, 0], np.arange(256.0))
    assert hist.shape == (3, 3, 256) and (hist.sum(-1) == 99).all()
    raw = out[0].astype(np.float64) * np.float32(STD)[:, None, None] + np.float32(MEAN)[:, None, None]
    assert raw.min() > 99.0 and raw.max() < 255.5           # the source sits in the template's range now
    # beta = 0 and a twin partner return the source
    zero = hist_ref.hist_ref(xs, xt, np.array([[0, 0, 1, 0], [0, 0, 1, 0]], np.int32), MEAN, STD, hist_ref.MEAN_T, hist_ref.STD_T)[0]
    twin = hist_ref.hist_ref(xs, xs, np.array([[0, 65536, 1, 0], [1, 40000, 1, 0]], np.int32))[0]
    assert np.array_equal(zero, xs) and np.array_equal(twin, xs)


# ---- the built library
def test_symbols_are_exported_declared_and_replayable():
    from regda_amd import _lib
    from regda_amd._ops import histogram
    L = _lib.lib()
    for name, nargs in NEW.items():
        assert name in L.protos and name not in L.missing
        assert len(L.protos[name][1]) == nargs
    assert L.raw('rgda_plan_fn_id')(b'rgda_hist_style') >= 0                # a row of a recorded plan
    assert L.raw('rgda_plan_fn_id')(b'rgda_hist_style_write_table') >= 0
    assert histogram.HIST_BLEND_ONE == 65536 == hist_ref.BLEND_ONE
    assert L.raw('rgda_abi_version')() == 10


def test_the_wrappers_are_reached_through_the_aug_module_and_not_through_ops():
    from regda_amd import ops
    from regda_amd._ops import histogram
    from regda_amd.aug import histogram as aug
    for name in ('hist_style', 'hist_style_workspace', 'hist_style_write_table'):
        assert getattr(aug, name) is getattr(histogram, name) and not hasattr(ops, name)
    assert aug.BLEND_ONE == histogram.HIST_BLEND_ONE


def test_workspace_query():
    from regda_amd import _lib
    size = lambda *a: _lib.lib().size('rgda_hist_style_workspace', *a)
    for n, m, h, w in ((3, 2, 33, 47), (16, 16, 512, 512), (1, 1, 1, 1), (1, 1, 4096, 4096)):
        assert size(n, m, h, w) == 256 + (n + m) * 3 * 256 * 4 + n * 3 * 256 * 4
    for shape in ((0, 1, 8, 8), (1, 0, 8, 8), (17, 1, 8, 8), (1, 17, 8, 8), (1, 1, 0, 8), (1, 1, 8, 0), (1, 1, 8, 4097),
                  (1, 1, 4097, 8), (-1, 1, 8, 8)):
        assert size(*shape) == 0, shape


def _host(n_floats=64):
    """a 16-byte aligned host buffer (kept alive by the first value) and its address"""
    buf = ctypes.create_string_buffer(4 * n_floats + 16)
    return buf, (ctypes.addressof(buf) + 15) & ~15


S_NAMES = ['img_s', 'img_t', 'out', 'table', 'ws', 'N', 'M', 'H', 'W', 'msr', 'msg', 'msb', 'ssr', 'ssg', 'ssb',
           'mtr', 'mtg', 'mtb', 'str', 'stg', 'stb', 'hist', 'lut', 'flag', 'stream']


def _style(**kw):
    from regda_amd import _lib
    bufs = [_host(4096) for _ in range(3)] + [_host(), _host(1 << 16), _host(4096)]
    s, t, o, tab, ws, aux = (b[1] for b in bufs)
    args = dict(zip(S_NAMES, (s, t, o, tab, ws, 2, 2, 8, 8, 1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 1.5, 2.5, 3.5, 4.5, 5.5, 6.5, None,
                              None, None, None)))
    named = {'src': s, 'src+': s + 64, 'tgt': t, 'tgt+': t + 64, 'table+4': tab + 4, 'ws+8': ws + 8, 'aux+2': aux + 2,
             'aux+4': aux + 4}
    for k, v in kw.items():
        args[k] = named.get(v, v) if isinstance(v, str) else v
    return _lib.lib().raw('rgda_hist_style')(*[args[k] for k in S_NAMES])


@pytest.mark.parametrize('kw,status', [
    (dict(img_s=None), -1), (dict(img_t=None), -1), (dict(out=None), -1), (dict(table=None), -1), (dict(ws=None), -1),
    (dict(table='table+4'), -1), (dict(ws='ws+8'), -1), (dict(hist='aux+2'), -1), (dict(lut='aux+4'), -1),
    (dict(N=0), -1), (dict(M=0), -1), (dict(H=0), -1), (dict(W=0), -1), (dict(N=-1), -1),
    (dict(ssr=0.0), -1), (dict(ssg=-1.0), -1), (dict(ssb=float('nan')), -1), (dict(str=0.0), -1), (dict(stg=float('inf')), -1),
    (dict(stb=float('nan')), -1), (dict(msr=float('nan')), -1), (dict(mtb=float('inf')), -1),
    (dict(out='src'), -1), (dict(out='src+'), -1), (dict(out='tgt'), -1), (dict(out='tgt+'), -1),     # in place, overlapping
    (dict(N=17), -4), (dict(M=17), -4), (dict(N=17, out=None), -1), (dict(H=4097), -4), (dict(W=4097), -4)])
def test_style_refusals_come_before_any_launch(kw, status):
    """RGDA_ERR_ARG (-1) / RGDA_ERR_UNSUPPORTED (-4): on a machine without a GPU a launch would fail with -3"""
    assert _style(**kw) == status


def _write(rows, n=None, m=2, h=64, w=64, table='t', host='h'):
    from regda_amd import _lib
    rows = np.ascontiguousarray(rows, np.int32)
    b, t = _host(256)
    tp = {'t': t, 't+4': t + 4, None: None}[table]
    hp = rows.ctypes.data if host == 'h' else None
    return _lib.lib().raw('rgda_hist_style_write_table')(tp, hp, rows.shape[0] if n is None else n, m, h, w, None)


@pytest.mark.parametrize('call,status', [
    (lambda: _write([[0, 5, 1, 0]], table=None), -1), (lambda: _write([[0, 5, 1, 0]], table='t+4'), -1),
    (lambda: _write([[0, 5, 1, 0]], host=None), -1), (lambda: _write([[0, 5, 1, 0]], n=0), -1),
    (lambda: _write([[0, 5, 1, 0]], m=0), -1), (lambda: _write([[0, 5, 1, 0]], h=0), -1), (lambda: _write([[0, 5, 1, 0]], w=0), -1),
    (lambda: _write([[2, 5, 1, 0]]), -1), (lambda: _write([[-1, 5, 1, 0]]), -1),            # a partner index >= M, or negative
    (lambda: _write([[0, 5, 1, 0], [1, 5, 1, 0], [2, 5, 0, 0]]), -1),                       # ... in a row that is off, too
    (lambda: _write([[0, -1, 1, 0]]), -1), (lambda: _write([[0, 65537, 1, 0]]), -1), (lambda: _write([[0, 65537, 0, 0]]), -1),
    (lambda: _write([[0, 5, 2, 0]]), -1), (lambda: _write([[0, 5, -1, 0]]), -1),
    (lambda: _write([[0, 5, 1, 0]] * 17), -4), (lambda: _write([[0, 5, 1, 0]], m=17), -4)])
def test_write_table_refusals_come_before_any_launch(call, status):
    assert call() == status


def test_python_wrappers_refuse_cpu_tensors():
    import torch
    from regda_amd.aug import histogram
    x = torch.zeros(2, 3, 8, 8)
    tab = torch.zeros(2, 4, dtype=torch.int32)
    with pytest.raises(RuntimeError):       # no CPU fallback
        histogram.hist_style(x, x, tab, MEAN, STD, MEAN, STD)
    with pytest.raises(RuntimeError):
        histogram.hist_style_write_table(tab, np.zeros((2, 4), np.int32), 2, (8, 8))


# ---- HistogramStyle
def test_draw_is_the_seeds_and_does_not_depend_on_the_coins():
    from regda_amd.aug.histogram import HistogramStyle
    kw = dict(blend=(0.25, 1.0), prob=0.5)
    a, b = HistogramStyle(seed=5, **kw), HistogramStyle(seed=5, **kw)
    ta = np.concatenate([a.draw(3, 4, 64, 96) for _ in range(30)])
    tb = np.concatenate([b.draw(3, 4, 64, 96) for _ in range(30)])
    assert ta.dtype == np.int32 and ta.shape == (90, 4) and np.array_equal(ta, tb)
    assert set(ta[:, 2].tolist()) == {0, 1} and set(ta[:, 0].tolist()) == {0, 1, 2, 3} and (ta[:, 3] == 0).all()
    assert 16384 <= ta[:, 1].min() < 24000 and 58000 < ta[:, 1].max() <= 65536 and 0.35 < ta[:, 2].mean() < 0.65
    # other probabilities, the same seed: other switches, the same partners and blends in the same places
    for prob, on in ((1.0, 1), (0.0, 0)):
        c = HistogramStyle(seed=5, blend=(0.25, 1.0), prob=prob)
        tc = np.concatenate([c.draw(3, 4, 64, 96) for _ in range(30)])
        assert np.array_equal(tc[:, :2], ta[:, :2]) and (tc[:, 2] == on).all()
    # one image at a time draws the same sequence as a batch
    e = HistogramStyle(seed=5, **kw)
    assert np.array_equal(np.concatenate([e.draw(1, 4, 64, 96) for _ in range(90)]), ta)
    assert not np.array_equal(HistogramStyle(seed=6, **kw).draw(3, 4, 64, 96), ta[:3])


@pytest.mark.parametrize('blend,q', [(0.0, 0), (1.0, 65536), (0.5, 32768), (0.3, 19661), ((0.75, 0.75), 49152)])
def test_blend_q_is_the_rounded_blend_times_65536(blend, q):
    from regda_amd.aug.histogram import HistogramStyle
    t = HistogramStyle(blend=blend, seed=0).draw(4, 2, 8, 8)
    assert (t[:, 1] == q).all() and (t[:, 2] == 1).all() and t[:, 0].max() <= 1
    assert HistogramStyle().blend == (0.5, 1.0) and HistogramStyle().prob == 1.0


def test_state_round_trip_continues_the_sequence():
    from regda_amd.aug.histogram import HistogramStyle
    a = HistogramStyle(blend=(0.1, 0.9), prob=0.5, seed=11)
    for _ in range(7):
        a.draw(2, 3, 64, 64)
    sd = a.state_dict()
    assert set(sd) == {'rng'}
    want = [a.draw(2, 3, 64, 64) for _ in range(5)]
    b = HistogramStyle(blend=(0.1, 0.9), prob=0.5, seed=99)
    b.load_state_dict(sd)
    assert all(np.array_equal(x, b.draw(2, 3, 64, 64)) for x in want)
    # validated first: a bad state leaves the object where it was
    c, twin = HistogramStyle(seed=3), HistogramStyle(seed=3)
    for bad in ({}, {'rng': 5}, {'rng': dict(sd['rng'], bit_generator='MT19937')},
                {'rng': dict(sd['rng'], state={'state': 'x', 'inc': 1})}):
        with pytest.raises(ValueError, match='HistogramStyle.rng'):
            c.load_state_dict(bad)
    assert np.array_equal(c.draw(4, 2, 64, 64), twin.draw(4, 2, 64, 64))


@pytest.mark.parametrize('kw', [dict(blend=-0.01), dict(blend=1.01), dict(blend=(0.5, 0.1)), dict(blend=(0.1,)),
                                dict(blend=(0.0, float('inf'))), dict(blend=float('nan')), dict(prob=1.5), dict(prob=-0.1),
                                dict(mean_s=(1.0, 2.0)), dict(std_s=(1.0, 0.0, 1.0)), dict(std_t=(1.0, float('nan'), 1.0)),
                                dict(mean_t=(1.0, 2.0, float('inf')))])
def test_constructor_refuses_bad_arguments(kw):
    from regda_amd.aug.histogram import HistogramStyle
    with pytest.raises(ValueError, match='HistogramStyle'):
        HistogramStyle(**kw)


def test_draw_refuses_what_the_kernels_do_not_serve():
    from regda_amd.aug.histogram import HistogramStyle
    f, twin = HistogramStyle(seed=1), HistogramStyle(seed=1)
    for args in ((0, 2, 64, 64), (2, 0, 64, 64), (17, 2, 64, 64), (2, 17, 64, 64), (2, 2, 4097, 64), (2, 2, 64, 0)):
        with pytest.raises(ValueError):
            f.draw(*args)
    assert np.array_equal(f.draw(2, 2, 64, 64), twin.draw(2, 2, 64, 64))        # a refused draw consumed nothing


def test_both_styles_bring_the_hook_the_steps_call():
    from regda_amd.aug.fourier import FourierStyle
    from regda_amd.aug.histogram import HistogramStyle
    for cls in (FourierStyle, HistogramStyle):
        for name in ('draw', 'workspace', 'write_table', 'apply', 'state_dict', 'load_state_dict'):
            assert callable(getattr(cls, name)), (cls, name)
