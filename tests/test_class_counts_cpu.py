"""Class counts 6 <= C <= 16 without a GPU: the CPU oracle against the reference-minted goldens at 8, 11 and 16 classes
(tests/golden/make_cn_goldens.py -> cn.npz), the label table of a 16-class config, and the refusals of counts outside
the range -- at the entry points, where the class count is checked before any memory is touched, and in the steps'
shape checks."""
import ctypes
import os
import sys
import types

import numpy as np
import pytest
import torch

from oracle import labels as olab

HERE = os.path.dirname(os.path.abspath(__file__))
COUNTS = (8, 11, 16)


@pytest.fixture(scope='module')
def cn():
    return np.load(os.path.join(HERE, 'golden', 'cn.npz'))


@pytest.mark.parametrize('C', COUNTS)
def test_oracle_pseudo_selection_and_homogenizer_match_the_reference(cn, C):
    p = f'c{C}_'
    for i in range(int(cn[p + 'ps_n'])):
        s = cn[f'{p}ps_in{i}']
        assert s.shape[1] == C
        assert np.array_equal(olab.pseudo_selection(s, 0.8, 0.6, -1), cn[f'{p}ps_out{i}'].astype(np.int64)), i
    for i in range(int(cn[p + 'lrh_n'])):
        got = olab.homogenize(cn[f'{p}lrh_lab{i}'].astype(np.int64), cn[f'{p}lrh_reg{i}'].astype(np.int64),
                              float(cn[f'{p}lrh_pct{i}']), C, -1)
        assert np.array_equal(got, cn[f'{p}lrh_out{i}'].astype(np.int64)), i


@pytest.mark.parametrize('C', COUNTS)
def test_oracle_downscale_matches_the_reference(cn, C):
    sys.path.insert(0, os.path.join(HERE, 'golden'))
    from make_cn_goldens import checksum, downscale_big_input
    lab = downscale_big_input(C)
    assert checksum(lab) == cn[f'c{C}_ds_big_sum']
    want = cn[f'c{C}_ds_big_out'].astype(np.int64).reshape(8, 32, 32)
    got = np.asarray(olab.downscale_label(lab, 16, C, -1, 0.75)).reshape(8, 32, 32)
    assert np.array_equal(got, want)
    # the hand-set cells of image 0, row 0 (make_cn_goldens.downscale_big_input): exactly 0.75 kept, 191/256 and the
    # 128 / 128 ties dropped by min_ratio, the highest class kept at 200/256, 256/256 and exactly 0.75
    assert list(want[0, 0, :10]) == [2, -1, -1, -1, C - 1, C - 1, C - 1, -1, -1, -1]
    # below min_ratio 0.5 the tie rule decides: the class tied with ignore wins (strict >, ignore last)
    got = np.asarray(olab.downscale_label(lab[:1, :16, :16 * 10], 16, C, -1, 0.5)).reshape(10)
    assert got[2] == 3 and got[8] == C - 1


def test_label_table_of_a_sixteen_class_config():
    from regda_amd import aug
    assert aug.label_config(types.SimpleNamespace(NUM_CLASSES=16, LABEL_OFFSET=-1, IGNORE_LABEL=-1)) == \
        dict(offset=-1, num_class=16, ignore_label=-1)
    base = _cfg('st.regda.2rural')                 # a real task config's data pipelines, with a 16-class label surface
    cfg = types.SimpleNamespace(NUM_CLASSES=16, LABEL_OFFSET=-1, IGNORE_LABEL=-1,
                                TARGET_DATA_CONFIG=base.TARGET_DATA_CONFIG, SOURCE_DATA_CONFIG=base.SOURCE_DATA_CONFIG)
    tabs = [aug.from_config(dc, **aug.label_config(cfg)).label_table()
            for dc in (cfg.TARGET_DATA_CONFIG, cfg.SOURCE_DATA_CONFIG)]
    expect = torch.full((256,), -1, dtype=torch.int32)
    expect[1:17] = torch.arange(16, dtype=torch.int32)
    for tab in tabs:
        assert torch.equal(tab, expect)             # 0 -> -1, 1..16 -> 0..15, >= 17 -> -1


def _cfg(name):
    from regda_amd.utils.tools import import_config
    return import_config(name, create=False, copy=False)


def _host():
    """An aligned host address and a buffer that keeps it alive: handed only with a refused class count, where every
    entry point below returns before it reads or launches anything."""
    buf = ctypes.create_string_buffer(256)
    a = ctypes.addressof(buf)
    return buf, a + (-a) % 16


@pytest.mark.parametrize('C', [5, 17])
def test_entry_points_refuse_counts_outside_6_to_16(C):
    from regda_amd import _lib
    L = _lib.lib()
    buf, f = _host()
    calls = [
        ('rgda_teacher_probs', (f, f, f, 1, C, 2, 2, 4, 4, None)),
        ('rgda_classifier_fwd', (f, 8, f, f, f, 1, 4, 8, C, None)),
        ('rgda_classifier_bwd', (f, 8, f, f, f, 8, f, f, 1, 4, 8, C, None, 0, None)),
        ('rgda_proto_stats', (f, f, f, 1, 8, C, 2, 2, 16, -1, 0.75, f, 1 << 20, None)),
        ('rgda_pseudo_lrh', (f, f, f, f, 1, 16, C, 0.8, 0.6, -1, 0.5, 16, f, 1 << 20, None)),
        ('rgda_label_refine', (f, f, f, f, f, f, 1, 8, C, 2, 2, 4, 4, 2.0, f, 1 << 20, None)),
        ('rgda_upsample_ce', (f, f, f, None, f, None, None, 1, C, 2, 2, 4, 4, -1, f, 1 << 20, None)),
        ('rgda_pcl_loss', (f, f, f, f, None, 0, 0, 1, 8, C, 2, 2, -1, 8.0, 1.0, f, 1 << 20, None)),
    ]
    for name, args in calls:
        with pytest.raises(ValueError, match='not supported'):
            L.call(name, *args)
    del buf


def test_step_checks_name_the_limits():
    from regda_amd import ops
    for c in (6, 7, 8, 11, 16):
        ops.check_class_count(c)
        ops.check_step_shape(c, 2048, 512, 512)
    for c in (5, 17):
        with pytest.raises(ValueError, match='6 <= class_num <= 16'):
            ops.check_class_count(c, 'SSLStep')
    # 1024 x 1024 tiles: the fused upsample + loss row pass serves up to 15 classes
    ops.check_step_shape(15, 2048, 1024, 1024)
    with pytest.raises(ValueError, match='W <= 1008'):
        ops.check_step_shape(16, 2048, 1024, 1024)
    ops.check_step_shape(16, 2048, 1008, 1008)
    # the prototypes of 16 classes fit the LDS up to 2048 channels
    with pytest.raises(ValueError, match='prototype'):
        ops.check_step_shape(16, 4096, 512, 512)


def test_step_checks_use_the_librarys_lds_budgets():
    """check_step_shape asks the library (rgda_class_lds / _limit) for the LDS of the class-dependent layouts; pin those
    answers at the boundaries the kernels refuse at: the loss row pass at 16 classes (W = 1008 served, 1024 not), the
    PCL and label_refine prototypes at 16 classes (K = 2048 served, 4096 not), and 6 / 7 classes at K = 4096."""
    from regda_amd import _lib
    L = _lib.lib()
    row, pcl, ref = 0, 1, 2
    lim_row, lim = L.size('rgda_class_lds_limit', row), L.size('rgda_class_lds_limit', pcl)
    assert lim_row == 150 * 1024 and lim == 160 * 1024 == L.size('rgda_class_lds_limit', ref)
    assert L.size('rgda_class_lds', row, 16, 63, 1008) <= lim_row < L.size('rgda_class_lds', row, 16, 64, 1024)
    assert L.size('rgda_class_lds', row, 15, 64, 1024) <= lim_row
    assert L.size('rgda_class_lds', row, 6, 32, 512) == (4 * 6 * 32 + 2 * 6 * 512 + 2 * 512) * 4
    for which in (pcl, ref):
        assert L.size('rgda_class_lds', which, 16, 2048, 0) <= lim < L.size('rgda_class_lds', which, 16, 4096, 0)
        for c in (6, 7):
            assert L.size('rgda_class_lds', which, c, 4096, 0) <= lim
    assert L.size('rgda_class_lds', 3, 16, 2048, 0) == 0


@pytest.mark.parametrize('C', COUNTS)
def test_oracle_label_refine_and_pcl_match_the_reference(cn, C):
    """oracle.labelpath's label_refine (with and without superpixels) and PrototypeContrastiveLoss against the
    reference-minted cases of cn.npz: the oracle the GPU tests compare with is itself pinned at these counts."""
    from oracle import labelpath as opath
    p = f'c{C}_'
    t = lambda k: torch.from_numpy(cn[p + k])
    out = opath.label_refine(t('rf_feat'), t('rf_protos'), [t('rf_p1'), t('rf_p2')], t('rf_soft'))
    np.testing.assert_allclose(out.numpy(), cn[p + 'rf_out'], rtol=1e-5, atol=1e-6)
    H = cn[p + 'rf_sup'].shape[-1]
    sup = t('rf_sup').long().reshape(-1, 1, H, H)
    out = opath.label_refine(t('rf_feat'), t('rf_protos'), [t('rf_p1'), t('rf_p2')], t('rf_soft'), True, 'all', 2.0,
                             label_t_sup=sup)
    np.testing.assert_allclose(out.numpy(), cn[p + 'rf_out_sup'], rtol=1e-5, atol=1e-6)
    f = t('pcl_feat').clone().requires_grad_(True)
    loss = opath.prototype_contrastive_loss(t('pcl_protos'), f, t('pcl_lab').long(), 8.0, -1)
    loss.backward()
    assert loss.item() == pytest.approx(float(cn[p + 'pcl_loss']), rel=1e-5)
    np.testing.assert_allclose(f.grad.numpy(), cn[p + 'pcl_gfeat'], rtol=1e-4, atol=1e-7)
