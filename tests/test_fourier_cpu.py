"""No GPU: the host side of the Fourier style transfer (FourierStyle's draws and state, the entry points' refusals, which
come before any launch), the invariants of the fp64 restatement the GPU tests compare against (tests/fourier_ref.py), and
the conditions on the GPU cases that keep its bound honest."""
import ctypes

import numpy as np
import pytest

import fourier_ref
from fourier_ref import MEAN, STD

NEW = {'rgda_fourier_style': 23, 'rgda_fourier_style_write_table': 7, 'rgda_fourier_style_workspace': 4}


def test_symbols_are_exported_declared_and_replayable():
    from regda_amd import _lib, ops
    L = _lib.lib()
    for name, nargs in NEW.items():
        assert name in L.protos and name not in L.missing
        assert len(L.protos[name][1]) == nargs
    assert L.raw('rgda_plan_fn_id')(b'rgda_fourier_style') >= 0         # a row of a recorded plan
    assert L.raw('rgda_plan_fn_id')(b'rgda_fourier_style_write_table') >= 0
    assert ops.STYLE_TABLE_COLS == 4 and ops.STYLE_MAX_B == 64 and ops.STYLE_MAX_IMAGES == 16
    assert L.raw('rgda_abi_version')() == 10


def test_workspace_is_sized_for_the_largest_b_the_tile_admits():
    from regda_amd import _lib
    size = lambda *a: _lib.lib().size('rgda_fourier_style_workspace', *a)

    def want(n, m, h, w):
        bc = min(64, (min(h, w) - 1) // 2)
        kx, ky = bc + 1, 2 * bc + 1
        up = lambda v: (v + 15) // 16 * 16
        total = 256
        for part in (kx * w, kx * h, (n + m) * 3 * kx * h, (n + m) * 3 * ky * kx, n * 3 * kx * h):
            total = up(total + 8 * part)
        return total
    for shape in ((3, 2, 40, 72), (2, 2, 33, 37), (1, 1, 132, 136), (16, 16, 512, 512), (1, 1, 1, 1)):
        assert size(*shape) == want(*shape), shape
    assert 30e6 < size(16, 16, 512, 512) < 50e6             # a few tens of MB
    for shape in ((0, 1, 8, 8), (1, 0, 8, 8), (17, 1, 8, 8), (1, 17, 8, 8), (1, 1, 0, 8), (1, 1, 8, 4097)):
        assert size(*shape) == 0, shape


def _host(n_floats=64):
    """a 16-byte aligned host buffer (kept alive by the first value) and its address"""
    buf = ctypes.create_string_buffer(4 * n_floats + 16)
    return buf, (ctypes.addressof(buf) + 15) & ~15


S_NAMES = ['img_s', 'img_t', 'out', 'table', 'ws', 'N', 'M', 'H', 'W', 'msr', 'msg', 'msb', 'ssr', 'ssg', 'ssb',
           'mtr', 'mtg', 'mtb', 'str', 'stg', 'stb', 'flag', 'stream']


def _style(**kw):
    from regda_amd import _lib
    bufs = [_host(4096) for _ in range(3)] + [_host(), _host(1 << 16)]
    s, t, o, tab, ws = (b[1] for b in bufs)
    args = dict(zip(S_NAMES, (s, t, o, tab, ws, 2, 2, 8, 8, 1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 1.5, 2.5, 3.5, 4.5, 5.5, 6.5, None,
                              None)))
    named = {'src': s, 'src+': s + 64, 'tgt': t, 'tgt+': t + 64, 'table+4': tab + 4, 'ws+8': ws + 8}
    for k, v in kw.items():
        args[k] = named.get(v, v) if isinstance(v, str) else v
    return _lib.lib().raw('rgda_fourier_style')(*[args[k] for k in S_NAMES])


@pytest.mark.parametrize('kw,status', [
    (dict(img_s=None), -1), (dict(img_t=None), -1), (dict(out=None), -1), (dict(table=None), -1), (dict(ws=None), -1),
    (dict(table='table+4'), -1), (dict(ws='ws+8'), -1),
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
    return _lib.lib().raw('rgda_fourier_style_write_table')(tp, hp, rows.shape[0] if n is None else n, m, h, w, None)


@pytest.mark.parametrize('call,status', [
    (lambda: _write([[0, 5, 1, 0]], table=None), -1), (lambda: _write([[0, 5, 1, 0]], table='t+4'), -1),
    (lambda: _write([[0, 5, 1, 0]], host=None), -1), (lambda: _write([[0, 5, 1, 0]], n=0), -1),
    (lambda: _write([[0, 5, 1, 0]], m=0), -1), (lambda: _write([[0, 5, 1, 0]], h=0), -1), (lambda: _write([[0, 5, 1, 0]], w=0), -1),
    (lambda: _write([[2, 5, 1, 0]]), -1), (lambda: _write([[-1, 5, 1, 0]]), -1),            # a partner index >= M, or negative
    (lambda: _write([[0, 5, 1, 0], [1, 5, 1, 0], [2, 5, 0, 0]]), -1),                       # ... in a row that is off, too
    (lambda: _write([[0, -1, 1, 0]]), -1), (lambda: _write([[0, 5, 2, 0]]), -1), (lambda: _write([[0, 5, -1, 0]]), -1),
    (lambda: _write([[0, 65, 1, 0]], h=512, w=512), -4),                                    # b > 64
    (lambda: _write([[0, 32, 1, 0]]), -4), (lambda: _write([[0, 20, 1, 0]], h=40, w=72), -4),       # 2b + 1 > min(H, W)
    (lambda: _write([[0, 20, 1, 0]], h=72, w=40), -4), (lambda: _write([[0, 1, 0, 0]], h=2, w=9), -4),
    (lambda: _write([[0, 5, 1, 0]] * 17), -4), (lambda: _write([[0, 5, 1, 0]], m=17), -4)])
def test_write_table_refusals_come_before_any_launch(call, status):
    assert call() == status


def test_python_wrappers_refuse_cpu_tensors():
    import torch
    from regda_amd import ops
    x = torch.zeros(2, 3, 8, 8)
    tab = torch.zeros(2, 4, dtype=torch.int32)
    with pytest.raises(RuntimeError):       # no CPU fallback
        ops.fourier_style(x, x, tab, MEAN, STD, MEAN, STD)
    with pytest.raises(RuntimeError):
        ops.fourier_style_write_table(tab, np.zeros((2, 4), np.int32), 2, (8, 8))


# ---- FourierStyle
def test_draw_is_the_seeds_and_does_not_depend_on_the_coins():
    from regda_amd.aug.fourier import FourierStyle
    kw = dict(beta=(0.0, 0.09), prob=0.5)
    a, b = FourierStyle(seed=5, **kw), FourierStyle(seed=5, **kw)
    ta = np.concatenate([a.draw(3, 4, 64, 96) for _ in range(30)])
    tb = np.concatenate([b.draw(3, 4, 64, 96) for _ in range(30)])
    assert ta.dtype == np.int32 and ta.shape == (90, 4) and np.array_equal(ta, tb)
    assert set(ta[:, 2].tolist()) == {0, 1} and set(ta[:, 0].tolist()) == {0, 1, 2, 3} and (ta[:, 3] == 0).all()
    assert ta[:, 1].min() == 0 and ta[:, 1].max() == 5 and 0.35 < ta[:, 2].mean() < 0.65       # floor(64 * 0.09) = 5
    # other probabilities, the same seed: other switches, the same partners and widths in the same places
    for prob, on in ((1.0, 1), (0.0, 0)):
        c = FourierStyle(seed=5, beta=(0.0, 0.09), prob=prob)
        tc = np.concatenate([c.draw(3, 4, 64, 96) for _ in range(30)])
        assert np.array_equal(tc[:, :2], ta[:, :2]) and (tc[:, 2] == on).all()
    # one image at a time draws the same sequence as a batch
    e = FourierStyle(seed=5, **kw)
    assert np.array_equal(np.concatenate([e.draw(1, 4, 64, 96) for _ in range(90)]), ta)
    assert not np.array_equal(FourierStyle(seed=6, **kw).draw(3, 4, 64, 96), ta[:3])


@pytest.mark.parametrize('h,w,beta,b', [(512, 512, 0.01, 5), (512, 512, 0.09, 46), (64, 64, 0.05, 3), (40, 72, 0.49, 19),
                                        (33, 37, 0.5, 16), (1024, 512, 0.125, 64), (64, 64, 0.0, 0), (100, 300, 0.0999, 9)])
def test_half_width_is_the_floor_of_the_shorter_edge_times_beta(h, w, beta, b):
    from regda_amd.aug.fourier import FourierStyle
    t = FourierStyle(beta=beta, seed=0).draw(4, 2, h, w)
    assert (t[:, 1] == b).all() and (t[:, 2] == 1).all() and t[:, 0].max() <= 1


def test_state_round_trip_continues_the_sequence():
    from regda_amd.aug.fourier import FourierStyle
    a = FourierStyle(beta=(0.01, 0.09), prob=0.5, seed=11)
    for _ in range(7):
        a.draw(2, 3, 64, 64)
    sd = a.state_dict()
    assert set(sd) == {'rng'}
    want = [a.draw(2, 3, 64, 64) for _ in range(5)]
    b = FourierStyle(beta=(0.01, 0.09), prob=0.5, seed=99)
    b.load_state_dict(sd)
    assert all(np.array_equal(x, b.draw(2, 3, 64, 64)) for x in want)
    # validated first: a bad state leaves the object where it was
    c, twin = FourierStyle(seed=3), FourierStyle(seed=3)
    for bad in ({}, {'rng': 5}, {'rng': dict(sd['rng'], bit_generator='MT19937')},
                {'rng': dict(sd['rng'], state={'state': 'x', 'inc': 1})}):
        with pytest.raises(ValueError, match='FourierStyle.rng'):
            c.load_state_dict(bad)
    assert np.array_equal(c.draw(4, 2, 64, 64), twin.draw(4, 2, 64, 64))


@pytest.mark.parametrize('kw', [dict(beta=-0.01), dict(beta=(0.05, 0.01)), dict(beta=(0.01,)), dict(beta=(0.0, float('inf'))),
                                dict(beta=float('nan')), dict(prob=1.5), dict(prob=-0.1), dict(mean_s=(1.0, 2.0)),
                                dict(std_s=(1.0, 0.0, 1.0)), dict(std_t=(1.0, float('nan'), 1.0)), dict(mean_t=(1.0, 2.0, float('inf')))])
def test_constructor_refuses_bad_arguments(kw):
    from regda_amd.aug.fourier import FourierStyle
    with pytest.raises(ValueError):
        FourierStyle(**kw)


def test_draw_refuses_what_the_kernels_do_not_serve():
    from regda_amd.aug.fourier import FourierStyle
    f = FourierStyle(beta=(0.0, 0.13), seed=1)
    assert f.draw(2, 2, 512, 492).shape == (2, 4)       # floor(492 * 0.13) = 63
    twin = FourierStyle(beta=(0.0, 0.13), seed=1)
    twin.draw(2, 2, 512, 492)
    for args in ((2, 2, 512, 512), (0, 2, 64, 64), (2, 0, 64, 64), (17, 2, 64, 64), (2, 17, 64, 64)):   # floor(512 * 0.13) = 66
        with pytest.raises(ValueError):
            f.draw(*args)
    with pytest.raises(ValueError):                     # 2 * 4 + 1 > 8
        FourierStyle(beta=0.5, seed=1).draw(1, 1, 8, 9)
    assert np.array_equal(f.draw(2, 2, 64, 64), twin.draw(2, 2, 64, 64))        # a refused draw consumed nothing


def test_the_steps_take_style_and_source_needs_the_target():
    """(the constructors are reached with a model only on the GPU: tests/test_fourier_step_gpu.py)"""
    import inspect
    from regda_amd.step import FusedStep
    assert inspect.signature(FusedStep.__init__).parameters['style'].default is None
    assert callable(FusedStep._style_source) and callable(FusedStep.style_flag_value)


# ---- the restatement's own invariants
def _pair(h, w, seed, same_norm=True):
    from test_fourier_gpu import tiles
    rng = np.random.default_rng(seed)
    norm = (MEAN, STD, MEAN, STD) if same_norm else (MEAN, STD, fourier_ref.MEAN_T, fourier_ref.STD_T)
    return tiles(rng, (2, 3, h, w), *norm[:2]), tiles(rng, (2, 3, h, w), *norm[2:]), norm


@pytest.mark.parametrize('h,w', [(12, 16), (13, 11), (9, 20)])
def test_the_window_is_the_published_one_of_the_shifted_spectrum(h, w):
    for b in (0, 1, 4):
        m = np.fft.fftshift(fourier_ref.window(h, w, b))
        ch, cw = h // 2, w // 2
        want = np.zeros((h, w), bool)
        want[ch - b:ch + b + 1, cw - b:cw + b + 1] = True
        assert np.array_equal(m, want) and m.sum() == (2 * b + 1) ** 2


@pytest.mark.parametrize('h,w', [(16, 24), (15, 9)])
def test_b_zero_is_the_mean_shift_and_a_twin_target_returns_the_source(h, w):
    xs, xt, norm = _pair(h, w, 3, same_norm=False)
    table = np.array([[1, 0, 1, 0], [0, 0, 0, 0]], np.int32)
    out = fourier_ref.fourier_ref(xs, xt, table, *norm)
    S = xs[0].astype(np.float64) * fourier_ref.f64(norm[1]) + fourier_ref.f64(norm[0])
    T = xt[1].astype(np.float64) * fourier_ref.f64(norm[3]) + fourier_ref.f64(norm[2])
    shift = T.mean((1, 2), keepdims=True) - S.mean((1, 2), keepdims=True)
    assert np.abs((out[0] * fourier_ref.f64(norm[1]) + fourier_ref.f64(norm[0])) - (S + shift)).max() < 1e-9
    assert np.abs(shift).max() > 1.0 and np.array_equal(out[1], xs[1].astype(np.float64))       # the off row as it is
    for b in (0, 2, (min(h, w) - 1) // 2):
        twin = fourier_ref.fourier_ref(xs, xs, np.array([[0, b, 1, 0], [1, b, 1, 0]], np.int32))
        assert np.abs(twin - xs).max() < 1e-12


def test_a_zero_bin_of_the_source_takes_phase_zero():
    S = np.full((8, 8), 100.0)              # every bin but DC is exactly 0
    T = np.full((8, 8), 50.0) + 8.0 * np.cos(2 * np.pi * np.arange(8) / 8)[None, :]      # |F_T(0, +-1)| = 8 * 64 / 2
    raw, imag = fourier_ref.swap(S, T, 1)
    assert imag < 1e-12 and np.abs(raw - T).max() < 1e-9        # amplitude 256 at phase 0 on both bins: T's own cosine


def test_the_pruned_form_equals_the_full_fft_on_every_gpu_case():
    from test_fourier_gpu import CASES, case
    for name in sorted(CASES):
        xs, xt, table, norm, want, _ = case(name)
        ms, ss, mt, st = (fourier_ref.f64(v) for v in norm)
        for n in np.flatnonzero(table[:, 2]):
            S, T = xs[n].astype(np.float64) * ss + ms, xt[table[n, 0]].astype(np.float64) * st + mt
            for ch in range(3):
                got = fourier_ref.pruned(S[ch], T[ch], int(table[n, 1]))
                assert np.abs(got - (want[n, ch] * ss[ch] + ms[ch])).max() < 1e-9, (name, n, ch)


def test_the_gpu_cases_are_well_conditioned_and_their_bound_is_tight_and_holds_for_float32():
    """Checked here so that the bound cannot hide a failure on the GPU: |F_T| / |F_S| <= 256 on every swapped bin, the bound
    at most 0.05 grey levels at every element, and a float32 numpy evaluation of the kernel's form, in its order of
    summation, inside the bound at every element."""
    from test_fourier_gpu import CASES, case
    for name in sorted(CASES):
        xs, xt, table, norm, want, err = case(name)
        rho = fourier_ref.conditioning(xs, xt, table, *norm)
        grey = fourier_ref.f64(norm[1])
        ms32, ss32 = (np.asarray(v, np.float32)[:, None, None] for v in norm[:2])
        mt32, st32 = (np.asarray(v, np.float32)[:, None, None] for v in norm[2:])
        worst = 0.0
        for n in np.flatnonzero(table[:, 2]):
            S, T = xs[n] * ss32 + ms32, xt[table[n, 0]] * st32 + mt32
            assert S.dtype == np.float32
            for ch in range(3):
                raw = fourier_ref.pruned(S[ch], T[ch], int(table[n, 1]), dtype=np.float32)
                assert raw.dtype == np.float32
                got = (raw - ms32[ch]) / ss32[ch]
                d = np.abs(got.astype(np.float64) - want[n, ch])
                worst = max(worst, float((d / err[n, ch]).max()))
                assert (d <= err[n, ch]).all(), (name, n, ch, float((d / err[n, ch]).max()))
        on = table[:, 2] == 1
        print('%s: max |F_T| / |F_S| %.1f, bound %.2e .. %.2e grey, float32 |d| / bound up to %.3f'
              % (name, rho, (err[on] * grey).min(), (err[on] * grey).max(), worst))
        assert rho <= 256.0, name
        assert (err[on] > 0).all() and (err[on] * grey).max() <= 0.05, name
        assert (err[~on] == 0).all()
