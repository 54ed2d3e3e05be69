"""No GPU: the host side of the strong augmentation (StrongAugment's draws and state, the entry points' refusals, which
come before any launch) and the invariants of the fp64 restatement the GPU tests compare against (tests/strong_ref.py)."""
import ctypes

import numpy as np
import pytest

import strong_ref

NEW = {'rgda_strong_augment': 15, 'rgda_strong_write_table': 6, 'rgda_strong_augment_workspace': 1}


def test_symbols_are_exported_declared_and_replayable():
    from regda_amd import _lib, ops
    L = _lib.lib()
    for name, nargs in NEW.items():
        assert name in L.protos and name not in L.missing
        assert len(L.protos[name][1]) == nargs
    assert L.raw('rgda_plan_fn_id')(b'rgda_strong_augment') >= 0        # a row of a recorded plan
    assert L.size('rgda_strong_augment_workspace', 5) == 5 * 128 and L.size('rgda_strong_augment_workspace', 0) == 0
    assert ops.STRONG_TABLE_COLS == 8 and ops.STRONG_MAX_RADIUS == 12
    assert L.raw('rgda_abi_version')() == 10


def _host(n_floats=64):
    """a 16-byte aligned host buffer (kept alive by the first value) and its address"""
    buf = ctypes.create_string_buffer(4 * n_floats + 16)
    return buf, (ctypes.addressof(buf) + 15) & ~15


A_NAMES = ['img_in', 'img_out', 'table', 'ws', 'N', 'H', 'W', 'mr', 'mg', 'mb', 'sr', 'sg', 'sb', 'flag', 'stream']


def _augment(**kw):
    from regda_amd import _lib
    b1, f = _host(4096)
    b2, g = _host(4096)
    b3, t = _host()
    b4, w = _host()
    args = dict(zip(A_NAMES, (f, g, t, w, 2, 8, 8, 1.0, 2.0, 3.0, 4.0, 5.0, 6.0, None, None)))
    for k, v in kw.items():
        args[k] = {'in': f, 'in+': f + 64, 'table+4': t + 4, 'ws+4': w + 4}.get(v, v) if isinstance(v, str) else v
    return _lib.lib().raw('rgda_strong_augment')(*[args[k] for k in A_NAMES])


@pytest.mark.parametrize('kw,status', [
    (dict(img_in=None), -1), (dict(img_out=None), -1), (dict(table=None), -1), (dict(ws=None), -1),
    (dict(table='table+4'), -1), (dict(ws='ws+4'), -1), (dict(N=0), -1), (dict(H=0), -1), (dict(W=0), -1),
    (dict(sr=0.0), -1), (dict(sg=-1.0), -1), (dict(sb=float('nan')), -1),
    (dict(img_out='in'), -1), (dict(img_out='in+'), -1),         # in place, and overlapping
    (dict(N=65536, img_out=None), -1), (dict(N=65536), -4), (dict(H=1 << 16, W=1 << 15), -4)])
def test_augment_refusals_come_before_any_launch(kw, status):
    """RGDA_ERR_ARG (-1) / RGDA_ERR_UNSUPPORTED (-4): on a machine without a GPU a launch would fail with -3"""
    assert _augment(**kw) == status


def _write(rows, n=None, h=64, w=64, table='t', host='h'):
    from regda_amd import _lib
    rows = np.ascontiguousarray(rows, np.float32)
    b, t = _host(256)
    tp = {'t': t, 't+4': t + 4, None: None}[table]
    hp = rows.ctypes.data if host == 'h' else None
    return _lib.lib().raw('rgda_strong_write_table')(tp, hp, rows.shape[0] if n is None else n, h, w, None)


GOOD = [1.1, 0.9, 1.2, 0.3, 1.0, 3, 0, 0]


def _row(**kw):
    r = list(GOOD)
    for k, v in kw.items():
        r[['fb', 'fc', 'fs', 'theta', 'sigma', 'flags'].index(k)] = v
    return [r]


@pytest.mark.parametrize('call,status', [
    (lambda: _write(_row(), table=None), -1), (lambda: _write(_row(), table='t+4'), -1),
    (lambda: _write(_row(), host=None), -1), (lambda: _write(_row(), n=0), -1), (lambda: _write(_row(), h=0), -1),
    (lambda: _write(_row(fb=float('nan'))), -1), (lambda: _write(_row(theta=float('inf'))), -1),
    (lambda: _write(_row(fs=-0.1)), -1), (lambda: _write(_row(flags=4)), -1), (lambda: _write(_row(flags=1.5)), -1),
    (lambda: _write(_row(sigma=float('nan'), flags=0)), -1),
    (lambda: _write(_row(sigma=0.0)), -4), (lambda: _write(_row(sigma=-1.0)), -4), (lambda: _write(_row(sigma=4.5)), -4),
    (lambda: _write(_row(sigma=4.0), h=12), -4), (lambda: _write(_row(sigma=4.0), w=12), -4),
    (lambda: _write(_row(sigma=1.15), h=4), -4),
    (lambda: _write([GOOD] * 17), -4)])
def test_write_table_refusals_come_before_any_launch(call, status):
    assert call() == status


def test_python_wrappers_refuse_cpu_tensors_and_bad_arguments():
    import torch
    from regda_amd import ops
    x = torch.zeros(2, 3, 8, 8)
    tab = torch.zeros(2, 8)
    with pytest.raises(RuntimeError):       # no CPU fallback
        ops.strong_augment(x, tab, strong_ref.MEAN, strong_ref.STD)
    with pytest.raises(RuntimeError):
        ops.strong_write_table(tab, np.zeros((2, 8), np.float32), (8, 8))


def test_draw_is_the_seeds_and_does_not_depend_on_the_coins():
    from regda_amd.aug.strong import BLUR, JITTER, StrongAugment
    a, b = StrongAugment(seed=5), StrongAugment(seed=5)
    ta, tb = np.concatenate([a.draw(3) for _ in range(30)]), np.concatenate([b.draw(3) for _ in range(30)])
    assert ta.dtype == np.float32 and ta.shape == (90, 8) and np.array_equal(ta, tb)
    assert set(ta[:, 5].tolist()) == {0.0, 1.0, 2.0, 3.0}            # every combination of the two bits occurs
    assert (ta[:, 6:] == 0).all()
    # other probabilities, the same seed: other flags, the same values in the same places
    c = StrongAugment(jitter_prob=1.0, blur_prob=0.0, seed=5)
    tc = np.concatenate([c.draw(3) for _ in range(30)])
    assert np.array_equal(tc[:, :5], ta[:, :5]) and (tc[:, 5] == JITTER).all()
    d = StrongAugment(jitter_prob=0.0, blur_prob=1.0, seed=5)
    assert (np.concatenate([d.draw(5) for _ in range(18)])[:, 5] == BLUR).all()
    # one image at a time draws the same sequence as a batch
    e = StrongAugment(seed=5)
    assert np.array_equal(np.concatenate([e.draw(1) for _ in range(90)]), ta)
    assert not np.array_equal(StrongAugment(seed=6).draw(3), ta[:3])


def test_table_layout_and_ranges():
    from regda_amd.aug.strong import StrongAugment
    s = StrongAugment(jitter_prob=0.5, brightness=0.4, contrast=0.3, saturation=0.1, hue=0.1, blur_prob=0.5,
                      sigma=(0.5, 2.0), seed=1)
    t = np.concatenate([s.draw(4) for _ in range(100)])
    for col, (lo, hi) in enumerate([(0.6, 1.4), (0.7, 1.3), (0.9, 1.1), (-0.2 * np.pi, 0.2 * np.pi), (0.5, 2.0)]):
        assert t[:, col].min() >= np.float32(lo) and t[:, col].max() <= np.float32(hi), col
        assert t[:, col].max() - t[:, col].min() > 0.8 * (hi - lo), col
    assert 0.4 < (t[:, 5].astype(int) & 1).mean() < 0.6 and 0.4 < (t[:, 5].astype(int) >> 1).mean() < 0.6
    # a switched-off range is neutral
    n = StrongAugment(brightness=0, contrast=0, saturation=0, hue=0, seed=2).draw(6)
    assert (n[:, :3] == 1).all() and (n[:, 3] == 0).all()


def test_state_round_trip_continues_the_sequence():
    from regda_amd.aug.strong import StrongAugment
    a = StrongAugment(seed=11)
    for _ in range(7):
        a.draw(2)
    sd = a.state_dict()
    assert set(sd) == {'rng'}
    want = [a.draw(2) for _ in range(5)]
    b = StrongAugment(seed=99)
    b.load_state_dict(sd)
    assert all(np.array_equal(x, b.draw(2)) for x in want)
    # validated first: a bad state leaves the object where it was
    c = StrongAugment(seed=3)
    twin = StrongAugment(seed=3)
    for bad in ({}, {'rng': 5}, {'rng': dict(sd['rng'], bit_generator='MT19937')},
                {'rng': dict(sd['rng'], state={'state': 'x', 'inc': 1})}):
        with pytest.raises(ValueError, match='StrongAugment.rng'):
            c.load_state_dict(bad)
    assert np.array_equal(c.draw(4), twin.draw(4))


@pytest.mark.parametrize('kw', [dict(jitter_prob=1.5), dict(blur_prob=-0.1), dict(brightness=1.2), dict(contrast=-0.1),
                                dict(saturation=2.0), dict(hue=0.6), dict(sigma=(0.0, 1.0)), dict(sigma=(1.0, 0.5)),
                                dict(sigma=(0.5, 4.5)), dict(sigma=(1.0,)), dict(mean=(1.0, 2.0)), dict(std=(1.0, 0.0, 1.0)),
                                dict(std=(1.0, float('nan'), 1.0))])
def test_constructor_refuses_bad_arguments(kw):
    from regda_amd.aug.strong import StrongAugment
    with pytest.raises(ValueError):
        StrongAugment(**kw)
    with pytest.raises(ValueError):
        StrongAugment().draw(0)


def test_the_other_steps_refuse_strong():
    from regda_amd.align import AlignStep
    from regda_amd.aug.strong import StrongAugment
    from regda_amd.source import SourceStep
    with pytest.raises(NotImplementedError, match='SSL step'):
        AlignStep(None, None, strong=StrongAugment(seed=1))
    with pytest.raises(NotImplementedError, match='SSL step'):
        SourceStep(None, strong=StrongAugment(seed=1))


# ---- the restatement's own invariants
def _tiles(n, h, w, seed):
    rng = np.random.default_rng(seed)
    raw = rng.uniform(0, 255, (n, 3, h, w))
    mean, std = np.asarray(strong_ref.MEAN)[:, None, None], np.asarray(strong_ref.STD)[:, None, None]
    return ((raw - mean) / std).astype(np.float32)


def test_neutral_factors_without_blur_change_an_image_by_rounding_only():
    x = _tiles(2, 9, 11, 0)
    table = np.array([[1, 1, 1, 0, 1.0, 1, 0, 0], [1, 1, 1, 0, 1.0, 0, 0, 0]], np.float32)
    out, err = strong_ref.strong_ref(x, table, bound=True)
    assert np.array_equal(out[1], x[1].astype(np.float64)) and (err[1] == 0).all()
    assert np.abs(out[0] - x[0]).max() < 1e-5       # fp32 mean / std against the doubles the tiles were made with
    assert (err[0] > 0).all() and err[0].max() < 21 * 2.0 ** -24 * 1.01 * 255 / 57.0 + 1e-12


def test_blur_preserves_a_constant_image_and_sums_to_one():
    for sigma in (0.15, 1.15, 4.0):
        R = strong_ref.radius(sigma)
        assert R == {0.15: 1, 1.15: 4, 4.0: 12}[sigma]
        t = strong_ref.taps(sigma, R)
        assert t.shape == (2 * R + 1,) and abs(t.sum() - 1) < 1e-15 and np.array_equal(t, t[::-1])
        u = np.full((3, 13, 17), 0.37)
        assert np.abs(strong_ref.blur(u, sigma) - 0.37).max() < 1e-15
    # reflection without the edge pixel, by hand: a row 0 1 2 3, R = 1, taps (a, b, a)
    idx = strong_ref.reflect_index(4, 1)
    assert idx.tolist() == [[1, 0, 1], [0, 1, 2], [1, 2, 3], [2, 3, 2]]
    a, b, _ = strong_ref.taps(0.3, 1)
    u = np.tile(np.arange(4.0), (3, 4, 1))
    got = strong_ref.blur(u, 0.3)[0, 0]
    assert np.allclose(got, [2 * a, 1.0, 2.0, 3 * b + 4 * a], atol=1e-15)


def test_hue_by_theta_then_minus_theta_is_the_identity_on_unclamped_values():
    rng = np.random.default_rng(3)
    u = rng.uniform(-0.5, 1.5, (3, 5, 7))
    for theta in (0.05, -0.3, 2.0):
        there, _ = strong_ref.jitter_steps(u, 1.0, 1.0, 1.0, theta, clamp=False)
        back, _ = strong_ref.jitter_steps(there, 1.0, 1.0, 1.0, -theta, clamp=False)
        assert np.abs(back - u).max() < 1e-14 and np.abs(there - u).max() > 1e-3
        # the grey value (Y) is kept: only the chroma turns
        assert np.abs((there * strong_ref.GREY[:, None, None]).sum(0) - (u * strong_ref.GREY[:, None, None]).sum(0)).max() < 1e-14
    assert np.allclose(strong_ref.hue_matrix(0.0), np.eye(3), atol=1e-15)


def test_every_clamp_binds_at_both_ends_in_the_gpu_cases():
    """The inputs tests/test_strong_gpu.py compares on: in every jittered image each of the four clamps (after brightness,
    contrast, saturation, hue) cuts values below 0 and values above 1 somewhere in the case set, on at least 1 % of the
    elements of some image, so a kernel that left one clamp out, or one end of it, would differ there."""
    from test_strong_gpu import CASES, case
    mean = np.asarray(strong_ref.MEAN, np.float32).astype(np.float64)[:, None, None]
    std = np.asarray(strong_ref.STD, np.float32).astype(np.float64)[:, None, None]
    best = np.zeros((4, 2))
    for name in sorted(CASES):
        x, table, _, _ = case(name)
        for n in np.flatnonzero(table[:, 5].astype(int) & 1):
            pre = []
            strong_ref.jitter_steps((x[n].astype(np.float64) * std + mean) / 255.0, *table[n, :4].astype(np.float64), pre=pre)
            assert len(pre) == 4
            share = np.array([[(a < -1e-3).mean(), (a > 1.0 + 1e-3).mean()] for a in pre])
            print(name, n, np.round(100 * share, 2).tolist())
            best = np.maximum(best, share)
    assert (best > 0.01).all(), best
