"""The LoveDA tasks' configuration surface (the reference's configs/st/regda/2rural.py, 2urban.py and
configs/ToRURAL.py / ToURBAN.py), their label table and the evaluation's ignore list -- CPU only."""
import json
import os

import pytest
import torch

from regda_amd.utils.tools import import_config

LOVEDA_MEAN = (73.53223948, 80.01710095, 74.59297778)
LOVEDA_STD = (41.5113661, 35.66528876, 33.75830885)
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


def _cfg(name):
    return import_config(name, create=False, copy=False)


@pytest.mark.parametrize('target,src', [('rural', 'Urban'), ('urban', 'Rural')])
def test_loveda_config_surface(target, src):
    cfg = _cfg('st.regda.2' + target)
    for attr in ('MODEL IGNORE_LABEL MOMENTUM NUM_CLASSES SNAPSHOT_DIR WEIGHT_DECAY LEARNING_RATE STAGE1_STEPS '
                 'STAGE2_STEPS STAGE3_STEPS NUM_STEPS PREHEAT_STEPS POWER EVAL_EVERY GENE_EVERY MULTI_LAYER IGNORE_BG '
                 'PSEUDO_SELECT CUTOFF_TOP CUTOFF_LOW TARGET_DATA_CONFIG SOURCE_DATA_CONFIG EVAL_DATA_CONFIG '
                 'PSEUDO_DATA_CONFIG TEST_DATA_CONFIG TARGET_SET target_dir DATASETS').split():
        assert hasattr(cfg, attr), attr
    assert cfg.MODEL == 'ResNet' and cfg.NUM_CLASSES == 7 and cfg.IGNORE_LABEL == -1
    assert cfg.MULTI_LAYER is True and cfg.IGNORE_BG is True and cfg.PSEUDO_SELECT is True
    assert cfg.DATASETS == 'LoveDA' and cfg.TARGET_SET == target.capitalize()
    assert cfg.SNAPSHOT_DIR == './log/regda/2' + target
    assert (cfg.STAGE1_STEPS, cfg.STAGE2_STEPS, cfg.STAGE3_STEPS) == (4000, 6000, 6000)
    assert (cfg.CUTOFF_TOP, cfg.CUTOFF_LOW, cfg.LEARNING_RATE, cfg.POWER) == (0.8, 0.6, 1e-2, 0.9)
    assert cfg.MEAN == LOVEDA_MEAN and cfg.STD == LOVEDA_STD
    tgt = target.capitalize()
    assert cfg.target_dir['image_dir'] == ['data/LoveDA/Val/%s/images_png' % tgt]
    assert cfg.SOURCE_DATA_CONFIG['image_dir'] == ['data/LoveDA/Train/%s/images_png' % src]
    assert cfg.SOURCE_DATA_CONFIG['mask_dir'] == ['data/LoveDA/Train/%s/masks_png' % src]
    assert cfg.EVAL_DATA_CONFIG['mask_dir'] == ['data/LoveDA/Train/%s/masks_png' % tgt]
    assert cfg.TEST_DATA_CONFIG['image_dir'] == ['data/LoveDA/Test/%s/images_png' % tgt]
    t = cfg.TARGET_DATA_CONFIG
    assert t['mask_dir'] == [None] and t['label_type'] == 'prob' and t['read_sup'] is True and t['batch_size'] == 8
    for dc in (cfg.SOURCE_DATA_CONFIG, cfg.EVAL_DATA_CONFIG, cfg.PSEUDO_DATA_CONFIG, cfg.TEST_DATA_CONFIG, t):
        norm = [x[1] for x in dc['transforms'] if x[0] == 'Normalize']
        assert len(norm) == 1 and norm[0]['mean'] == LOVEDA_MEAN and norm[0]['std'] == LOVEDA_STD


@pytest.mark.parametrize('target', ['rural', 'urban'])
def test_loveda_target_pipeline_has_no_clamp(target):
    from regda_amd import aug
    from regda_amd.aug import augmentation
    cfg = _cfg('st.regda.2' + target)
    p = aug.from_config(cfg.TARGET_DATA_CONFIG, **aug.label_config(cfg))
    assert isinstance(p, augmentation.Compose)
    norms = [t for t in p.transforms if isinstance(t, augmentation.Normalize)]
    assert len(norms) == 1 and norms[0].clamp is False
    tab = norms[0].table()
    mean = torch.tensor(LOVEDA_MEAN, dtype=torch.float32).view(3, 1)
    std = torch.tensor(LOVEDA_STD, dtype=torch.float32).view(3, 1)
    assert torch.equal(tab, (torch.arange(256, dtype=torch.float32).expand(3, 256) - mean) / std)
    assert float(tab.max()) > 1.0               # a clamp(max=1) would have cut these
    # the ISPRS target pipelines keep theirs
    isprs = _cfg('st.regda.2potsdam')
    pi = aug.from_config(isprs.TARGET_DATA_CONFIG, **aug.label_config(isprs))
    assert [t.clamp for t in pi.transforms if isinstance(t, augmentation.Normalize)] == [True]


@pytest.mark.parametrize('target', ['rural', 'urban'])
def test_loveda_label_table(target):
    from regda_amd import aug
    cfg = _cfg('st.regda.2' + target)
    assert aug.label_config(cfg) == dict(offset=-1, num_class=7, ignore_label=-1)
    expect = torch.full((256,), -1, dtype=torch.int32)
    expect[1:8] = torch.arange(7, dtype=torch.int32)
    for dc in (cfg.TARGET_DATA_CONFIG, cfg.SOURCE_DATA_CONFIG):
        tab = aug.from_config(dc, **aug.label_config(cfg)).label_table()
        assert torch.equal(tab, expect)              # 0 -> -1, 1..7 -> 0..6, >= 8 -> -1
    # the ISPRS configs set none of the names: IsprsDA's table (0, 6, -1)
    isprs = _cfg('st.regda.2vaihingen')
    assert aug.label_config(isprs) == dict(offset=0, num_class=6, ignore_label=-1)


def test_evaluate_ignore_list(monkeypatch):
    from regda_amd.utils import eval as ev
    seen = []

    class Metric:
        def __init__(self, n, class_names=None, logdir=None, logger=None, ignore_labels=()):
            seen.append((n, list(ignore_labels)))

        def summary_all(self):
            return None

    class Model:
        num_classes = 7

        def eval(self):
            return self
    monkeypatch.setattr(ev, 'PixelMetricIgnore', Metric)
    for name, expect in (('st.regda.2rural', (7, [])), ('st.regda.2urban', (7, [])), ('st.regda.2potsdam', (7, [0]))):
        seen.clear()
        ev.evaluate(Model(), _cfg(name), is_training=True, dataloader=[])
        assert seen == [expect], name


def test_isprs_configs_unchanged():
    """The two ISPRS modules come out exactly as before the LoveDA tasks were added (snapshot of their surface)."""
    with open(os.path.join(GOLD, 'isprs_config_surface.json')) as f:
        snap = json.load(f)
    for name in ('st.regda.2potsdam', 'st.regda.2vaihingen'):
        m = _cfg(name)
        got = repr(sorted((k, v) for k, v in vars(m).items() if (k.isupper() and k != 'SNAPSHOT_DIR') or k == 'target_dir'))
        assert got == snap[name], name
        assert m.SNAPSHOT_DIR.startswith('./log/regda/' + name.split('.')[-1])     # (other tests append a postfix)
        assert not hasattr(m, 'NUM_CLASSES') and not hasattr(m, 'LABEL_OFFSET') and m.MODEL == 'ResNet101'
