"""CPU: the in-step cross-domain mix (rgda_domain_mix_table, rgda_mix_select_classes, rgda_mix_write_table,
DomainMix.draw_step): the ABI's exports and argument errors through raw calls, the draws, and the select rule's numpy
restatement (tests/mix_select_ref.py) on hand-worked cases."""
import ctypes

import numpy as np
import pytest

import mix_select_ref

NEW = {'rgda_domain_mix_table': 15, 'rgda_mix_select_classes': 11, 'rgda_mix_write_table': 11}


def test_symbols_are_exported_declared_and_replayable():
    from regda_amd import _lib, ops
    L = _lib.lib()
    ids = set()
    for name, nargs in NEW.items():
        assert name in L.protos and name not in L.missing
        assert len(L.protos[name][1]) == nargs
        fid = L.raw('rgda_plan_fn_id')(name.encode())
        assert 0 <= fid < L.raw('rgda_plan_fn_count')()
        ids.add(fid)
    assert len(ids) == len(NEW)
    assert L.protos['rgda_mix_write_table'][1][5] is ctypes.c_uint32
    assert L.raw('rgda_abi_version')() == 10
    hdr = open(_lib.HEADER_PATH).read()
    assert '#define RGDA_MIX_TABLE_COLS %d' % ops.MIX_TABLE_COLS in hdr
    assert '#define RGDA_MIX_WRITE_MAX_IMAGES %d' % ops.MIX_WRITE_MAX_IMAGES in hdr
    assert ops.MIX_TABLE_COLS == mix_select_ref.TABLE_COLS


def _host16():
    buf = ctypes.create_string_buffer(80)
    f = ctypes.addressof(buf)       # a host address: never dereferenced, every call below returns before a launch
    return buf, f + (-f) % 16


def _raw(name, names, pointers, good, kw):
    from regda_amd import _lib
    a = dict(good, **kw)
    return _lib.lib().raw(name)(*[(a[k] or None) if k in pointers else a[k] for k in names])


T_NAMES = ['img_s', 'label_s', 'img_in', 'img_out', 'label_t', 'soft_t', 'table', 'N', 'C', 'H', 'W', 'mode', 'ignore_label',
           'flag', 'stream']
T_PTRS = T_NAMES[:7] + ['flag', 'stream']


@pytest.mark.parametrize('kw', [
    dict(table=0), dict(table='misaligned'), dict(C=0), dict(C=33), dict(img_out=0), dict(img_in=0), dict(img_s=0),
    dict(label_s=0), dict(N=0), dict(H=0), dict(W=-1), dict(mode=2), dict(mode=-1),
], ids=repr)
def test_table_mix_refusals_without_a_gpu(kw):
    buf, f = _host16()
    if kw.get('table') == 'misaligned':
        kw = dict(table=f + 4)
    good = dict(zip(T_NAMES, (f, f, f, f, f, 0, f, 2, 6, 24, 20, 0, -1, 0, None)))
    assert _raw('rgda_domain_mix_table', T_NAMES, T_PTRS, good, kw) == -1


def test_table_mix_with_nothing_to_write_returns_ok_without_a_launch():
    buf, f = _host16()
    good = dict(zip(T_NAMES, (f, f, 0, 0, 0, 0, f, 2, 6, 24, 20, 0, -1, 0, None)))
    assert _raw('rgda_domain_mix_table', T_NAMES, T_PTRS, good, {}) == 0


S_NAMES = ['label_s', 'ranks', 'table', 'ws', 'N', 'C', 'H', 'W', 'ignore_label', 'flag', 'stream']
S_PTRS = S_NAMES[:4] + ['flag', 'stream']


@pytest.mark.parametrize('kw', [
    dict(label_s=0), dict(ranks=0), dict(table=0), dict(table='misaligned'), dict(ws=0), dict(C=0), dict(C=33), dict(N=0),
    dict(H=0), dict(W=0),
], ids=repr)
def test_select_refusals_without_a_gpu(kw):
    buf, f = _host16()
    if kw.get('table') == 'misaligned':
        kw = dict(table=f + 8)
    good = dict(zip(S_NAMES, (f, f, f, f, 2, 6, 24, 20, -1, 0, None)))
    assert _raw('rgda_mix_select_classes', S_NAMES, S_PTRS, good, kw) == -1


W_NAMES = ['table', 'ranks', 'ranks_host', 'N', 'C', 'class_bits', 'y0', 'y1', 'x0', 'x1', 'stream']
W_PTRS = W_NAMES[:3] + ['stream']


@pytest.mark.parametrize('kw,status', [
    (dict(table=0), -1), (dict(table='misaligned'), -1), (dict(C=0), -1), (dict(C=33), -1), (dict(N=0), -1),
    (dict(class_bits=1 << 6), -1), (dict(C=31, class_bits=1 << 31), -1), (dict(y0=-1), -1), (dict(y0=3, y1=2), -1),
    (dict(x0=-1), -1), (dict(x0=5, x1=4), -1), (dict(ranks='f'), -1), (dict(ranks_host='f'), -1),
    (dict(N=17), -4), (dict(N=17, ranks='f', ranks_host='f'), -4), (dict(N=1 << 20), -4),
], ids=repr)
def test_write_table_refusals_without_a_gpu(kw, status):
    """RGDA_ERR_ARG (-1), and RGDA_ERR_UNSUPPORTED (-4) for more images than the argument block holds."""
    from regda_amd import ops
    assert ops.MIX_WRITE_MAX_IMAGES == 16
    buf, f = _host16()
    kw = {k: (f + 4 if v == 'misaligned' else f if v == 'f' else v) for k, v in kw.items()}
    good = dict(zip(W_NAMES, (f, 0, 0, 2, 6, 0b101, 0, 0, 0, 0, None)))
    assert _raw('rgda_mix_write_table', W_NAMES, W_PTRS, good, kw) == status


def test_python_wrappers_refuse_cpu_tensors():
    import torch
    from regda_amd import ops
    x = torch.zeros(1, 3, 4, 4)
    lab = torch.zeros(1, 4, 4, dtype=torch.int64)
    tab = torch.zeros(1, 8, dtype=torch.int32)
    with pytest.raises(RuntimeError):       # no CPU fallback
        ops.domain_mix_table(x, lab, tab, ops.MIX_CLASS, images_in=x, images_out=x.clone())
    with pytest.raises(RuntimeError):
        ops.mix_select_classes(lab, torch.zeros(1, 6, dtype=torch.uint8), tab)
    with pytest.raises(RuntimeError):
        ops.mix_write_table(tab, 6)


# ---------------------------------------------------------------------------------------------------------------- draws
def test_dacs_rows_are_permutations_and_the_sequence_is_the_seeds():
    from regda_amd.aug.mix import DomainMix
    d1, d2 = DomainMix('dacs', 7, prob=0.7, seed=5), DomainMix('dacs', 7, prob=0.7, seed=5)
    s1 = [d1.draw_step(3, 64, 48) for _ in range(40)]
    s2 = [d2.draw_step(3, 64, 48) for _ in range(40)]
    assert any(d is None for d in s1) and any(d is not None for d in s1)
    for a, b in zip(s1, s2):
        assert (a is None) == (b is None)
        if a is None:
            continue
        assert a[0] == 'ranks' and a[1].dtype == np.uint8 and a[1].shape == (3, 7)
        assert np.array_equal(a[1], b[1])
        for row in a[1]:
            assert sorted(row.tolist()) == list(range(7))
    drawn = [a[1] for a in s1 if a is not None]
    assert any(not np.array_equal(drawn[0], x) for x in drawn[1:])          # the draws differ from batch to batch
    assert any(not np.array_equal(x[0], x[1]) for x in drawn)               # and from image to image
    other = [DomainMix('dacs', 7, prob=0.7, seed=6).draw_step(3, 64, 48) for _ in range(40)]
    assert [x is None for x in other] != [x is None for x in s1] or \
        any(not np.array_equal(a[1], b[1]) for a, b in zip(s1, other) if a is not None and b is not None)
    assert all(DomainMix('dacs', 6, prob=0.0, seed=1).draw_step(2, 8, 8) is None for _ in range(20))
    with pytest.raises(ValueError):
        DomainMix('dacs', 6, seed=1).draw(8, 8)         # the labels live on the device: a step's draw only


def test_dacs_state_round_trip_continues_the_sequence():
    from regda_amd.aug.mix import DomainMix
    a = DomainMix('dacs', 6, prob=0.8, seed=11)
    for _ in range(7):
        a.draw_step(2, 32, 32)
    sd = a.state_dict()
    assert set(sd) == {'rng'}                   # the generator is the only state, as for the other kinds
    b = DomainMix('dacs', 6, prob=0.8, seed=99)
    b.load_state_dict(sd)
    for _ in range(20):
        x, y = a.draw_step(2, 32, 32), b.draw_step(2, 32, 32)
        assert (x is None) == (y is None) and (x is None or np.array_equal(x[1], y[1]))


@pytest.mark.parametrize('kind', ['class', 'box'])
def test_class_and_box_step_draws_are_those_of_draw(kind):
    from regda_amd.aug.mix import DomainMix
    a, b = DomainMix(kind, 6, prob=0.7, seed=5), DomainMix(kind, 6, prob=0.7, seed=5)
    s1 = [a.draw(64, 48) for _ in range(40)]
    s2 = [b.draw_step(4, 64, 48) for _ in range(40)]
    assert s1 == s2 and any(d is None for d in s1) and any(d is not None for d in s1)


# ---------------------------------------------------------------------------------------------------------------- rule
def test_select_rule_on_hand_worked_cases():
    sel = mix_select_ref.select_classes
    ig = np.full((1, 2, 3), -1, np.int64)
    perm = np.array([[3, 0, 5, 1, 4, 2]], np.uint8)
    # P = 0: nothing
    bits, flag = sel(ig, perm)
    assert bits.tolist() == [0] and bits.dtype == np.uint32 and flag == 0
    # P = 1: (1 + 1) // 2 = 1, the class itself
    one = ig.copy()
    one[0, 1, 2] = 4
    assert sel(one, perm)[0].tolist() == [1 << 4]
    # P = 3 (classes 0, 2, 5 with ranks 3, 5, 2): two classes, those of rank 2 and 3
    three = np.array([[[0, 2, 5], [-1, 0, 0]]], np.int64)
    assert sel(three, perm)[0].tolist() == [(1 << 5) | (1 << 0)]
    # P = 2: one class, the smaller rank (class 1, rank 0, against class 3, rank 1)
    assert sel(np.array([[[1, 3, 3]]], np.int64), perm)[0].tolist() == [1 << 1]
    # P = C = 16: the eight classes of ranks 0..7
    r16 = np.array([[(5 * c + 3) % 16 for c in range(16)]], np.uint8)
    all16 = np.arange(16, dtype=np.int64).reshape(1, 4, 4)
    bits, flag = sel(all16, r16)
    want = sum(1 << c for c in range(16) if r16[0][c] < 8)
    assert bits.tolist() == [want] and bin(want).count('1') == 8 and flag == 0
    # per image, and the flag for a label that is neither a class nor the ignore label
    two = np.concatenate([three, np.array([[[1, 3, 3], [9, -1, -1]]], np.int64)])
    bits, flag = sel(two, np.concatenate([perm, perm]))
    assert bits.tolist() == [(1 << 5) | 1, 1 << 1] and flag == 1
    # ranks at or above C select nothing: the batch a step does not mix
    assert sel(three, np.full((1, 6), 255, np.uint8))[0].tolist() == [0]
    assert mix_select_ref.classes_of(0b100101, 6) == [0, 2, 5]
    assert mix_select_ref.table_rows(2, 5, (1, 2, 3, 4)).tolist() == [[5, 1, 2, 3, 4, 0, 0, 0]] * 2
