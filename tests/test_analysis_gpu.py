"""GPU: the pseudo-label analysis.  rgda_pseudo_analysis's integer tables EQUAL to the numpy restatement
(tests/analysis_ref.py) for every input kind, class count and shape, on both load routes; PseudoLabelAnalysis.summary()
against the reference's own loop (tests/golden/pseudo_analysis.npz); the fold's order, determinism, the flag word, and
the three ways in (tensors, files, the gener_target_pseudo hook).

Bounds (tests/test_analysis_cpu.py derives them): integer lists equal, acc_list rtol 5e-7, diffi_list rtol 1e-5 against
the reference; against the restatement everything is equal: the tables are integers and both sides form the fp64
quotients from the same integers with correctly rounded divisions, in the same image order."""
import functools
import math
import os
import types

import numpy as np
import pytest
import torch

import analysis_ref as ar

pytestmark = pytest.mark.gpu

SEED = 20
CASES = [(kind,) + s for s in ar.shapes() for kind in ar.KINDS]
LISTS = ('acc_list', 'diffi_list', 'cnt_true_list', 'cnt_used_list')


@functools.lru_cache(maxsize=None)
def _case(kind, b, C, H, W):
    soft, gt = ar.inputs(kind, b, C, H, W, SEED)
    return soft, gt, ar.analyse(soft, gt)


def _edges(C, R=ar.R):
    from regda_amd.gast.pseudo_generation import entropy_bin_edges
    _, lo, hi = entropy_bin_edges(C, R)
    return torch.from_numpy(lo).cuda(), torch.from_numpy(hi).cuda()


def _tables(soft, gt):
    from regda_amd import ops
    b, C = soft.shape[:2]
    lo, hi = _edges(C)
    t = ops.pseudo_analysis(soft, gt, lo, hi, ar.TOP, ar.LOW, ar.IGNORE)
    used, hit, inbin, d24, flag = ops.analysis_views(t, b, C, ar.R)
    return dict(used=used.cpu().numpy(), hit=hit.cpu().numpy(), inbin=inbin.cpu().numpy(), diff24=d24.cpu().numpy(),
                flag=int(flag.item()))


def _assert_tables(got, want):
    for k in ('used', 'hit', 'inbin', 'diff24'):
        assert np.array_equal(got[k], want[k]), k
    assert got['flag'] == want['flag']


def _assert_summaries_equal(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), k


@pytest.mark.parametrize('kind,b,C,H,W', CASES)
def test_tables_equal_the_restatement(kind, b, C, H, W):
    soft, gt, want = _case(kind, b, C, H, W)
    got = _tables(torch.from_numpy(soft).cuda(), torch.from_numpy(gt).cuda())
    _assert_tables(got, want)
    assert got['inbin'].sum() == (0 if kind == 'uniform' else b * H * W)        # one bin per pixel: no gap, no overlap
    if kind == 'zeros':
        assert got['inbin'][:, ar.R].min() > 0


def test_tables_on_a_view_that_starts_4_bytes_into_its_buffer():
    """H * W % 4 == 0 but the planes are not 16-byte aligned: the scalar loads of both passes (the analysis kernel's
    scalar route, the maximum pass kept off its 16-byte loads by its chunk) at a shape the vector route serves."""
    soft, gt, want = _case('softmax', 3, 6, 96, 100)
    buf = torch.zeros(soft.size + 1, dtype=torch.float32, device='cuda')
    view = buf[1:].view(soft.shape)
    view.copy_(torch.from_numpy(soft))
    assert view.data_ptr() % 16 == 4 and view.is_contiguous()
    _assert_tables(_tables(view, torch.from_numpy(gt).cuda()), want)


def test_workgroups_that_take_more_than_one_step():
    """64 images of 96 x 100: the launch's workgroups are shared among the images, 8 per image for the 10 steps of one, so
    the first two workgroups of every image go round their loop twice.  Tables and the folded summary of the 64 images."""
    from regda_amd.gast.pseudo_generation import PseudoLabelAnalysis
    soft, gt = ar.inputs('softmax', 64, 6, 96, 100, SEED)
    want = ar.analyse(soft, gt)
    s, g = torch.from_numpy(soft).cuda(), torch.from_numpy(gt).cuda()
    _assert_tables(_tables(s, g), want)
    a = PseudoLabelAnalysis(6)
    a.update(s, g)
    _assert_summaries_equal(a.summary(), ar.summary(ar.fold(ar.new_state(6), want), 6))


@pytest.mark.parametrize('kind,b,C,H,W', CASES)
def test_summary_matches_the_reference_loop(gold, kind, b, C, H, W):
    from regda_amd.gast.pseudo_generation import PseudoLabelAnalysis
    soft, gt, tables = _case(kind, b, C, H, W)
    a = PseudoLabelAnalysis(C)
    a.update(torch.from_numpy(soft).cuda(), torch.from_numpy(gt).cuda())
    got = a.summary()
    g = gold('pseudo_analysis.npz')
    want = {k: g[f'{kind}/c{C}/{H}x{W}/{k}'] for k in LISTS}
    assert np.array_equal(got['cnt_true_list'], want['cnt_true_list'])
    assert np.array_equal(got['cnt_used_list'], want['cnt_used_list'])
    np.testing.assert_allclose(got['acc_list'], want['acc_list'], rtol=5e-7)
    np.testing.assert_allclose(got['diffi_list'], want['diffi_list'], rtol=1e-5)
    _assert_summaries_equal(got, ar.summary(ar.fold(ar.new_state(C), tables), C))


def test_two_updates_equal_one_on_the_concatenated_batch_and_resume():
    from regda_amd.gast.pseudo_generation import PseudoLabelAnalysis
    soft, gt, _ = _case('softmax', 3, 6, 96, 100)
    s, g = torch.from_numpy(soft).cuda(), torch.from_numpy(gt).cuda()
    one, two, resumed = PseudoLabelAnalysis(6), PseudoLabelAnalysis(6), PseudoLabelAnalysis(6)
    one.update(s, g)
    two.update(s[:1], g[:1])
    sd = two.state_dict()
    two.update(s[1:], g[1:])
    assert torch.equal(one._state, two._state)          # the integers and the f64 sums: the same image order
    assert one.summary()['images'] == 3
    resumed.load_state_dict(sd)
    resumed.update(s[1:], g[1:])
    assert torch.equal(one._state, resumed._state)
    again = PseudoLabelAnalysis(6)                      # two runs: the same bits
    again.update(s, g)
    assert torch.equal(one._state, again._state)
    one.reset()
    assert not one._state.any() and one.summary()['images'] == 0


@pytest.mark.parametrize('bit', (0, 1))
def test_flag_bits_and_the_summary_refusal(bit):
    from regda_amd.gast.pseudo_generation import PseudoLabelAnalysis
    soft, gt, _ = _case('softmax', 2, 6, 33, 45)
    soft, gt = soft.copy(), gt.copy()
    if bit == 0:
        soft[1, 2, 5, 7] = 1.5
    else:
        gt[1, 5, 7] = 6
    got = _tables(torch.from_numpy(soft).cuda(), torch.from_numpy(gt).cuda())
    assert got['flag'] == 1 << bit
    if bit == 1:        # the pixel is skipped, the others are counted as they were
        want = ar.analyse(soft, gt)
        _assert_tables(got, want)
        assert got['inbin'].sum() == soft.shape[0] * 33 * 45 - 1
    a = PseudoLabelAnalysis(6)
    a.update(torch.from_numpy(soft).cuda(), torch.from_numpy(gt).cuda())
    with pytest.raises(ValueError, match=f'bit {bit}'):
        a.summary()


def test_range_static_on_device_maps_matches_the_reference_on_one_bin(gold):
    from regda_amd import ops
    from regda_amd.gast.pseudo_generation import range_static
    kind, C, H, W, img, i = 'softmax', 6, 33, 45, 0, 7          # make_analysis_goldens.ONE_BIN
    soft, gt, _ = _case(kind, 2, C, H, W)
    s, g = torch.from_numpy(soft[img:img + 1]).cuda(), torch.from_numpy(gt[img:img + 1]).cuda()
    pseudo = ops.pseudo_select(s, 0.8, 0.6, -1)
    pseudo[pseudo == -1] = C
    entropy = torch.sum(-s * torch.log(s), dim=1)
    diff = torch.from_numpy(ar.difficulty(soft[img:img + 1], gt[img:img + 1])).cuda()
    step = math.log(C) / 100
    got = [float(r) for r in range_static(entropy, diff, pseudo, g, 1.0 * i * step, 1.0 * i * step + step, C)]
    want = gold('pseudo_analysis.npz')['one_bin/result']
    assert got[0] == want[0] and got[1] == want[1]
    np.testing.assert_allclose(got[2:], want[2:], rtol=1e-5)


def _write_labels(label_dir, names, gt):
    from PIL import Image
    os.makedirs(label_dir, exist_ok=True)
    for name, g in zip(names, gt):
        Image.fromarray((g + 1).astype(np.uint8)).save(os.path.join(label_dir, name))       # 0 = ignored


def test_file_route_and_the_gener_target_pseudo_hook(tmp_path):
    from regda_amd.gast.pseudo_generation import PseudoLabelAnalysis, analysis_pseudo_labels, gener_target_pseudo
    soft, gt, tables = _case('softmax', 2, 6, 33, 45)
    names = ['tile_0.png', 'tile_1.png']
    probs = {float(i): torch.from_numpy(soft[i:i + 1]) for i in range(2)}

    class Model:
        num_classes = 6

        def eval(self):
            return self

        def __call__(self, x):          # the tile's index travels in the image
            return probs[float(x[0, 0, 0, 0])].cuda()

    loader = [(torch.full((1, 3, 33, 45), float(i)), {'fname': [names[i]], 'cls': torch.from_numpy(gt[i:i + 1])}) for i in range(2)]
    cfg = types.SimpleNamespace(NUM_CLASSES=6)
    hook = PseudoLabelAnalysis(6)
    gener_target_pseudo(cfg, Model(), loader, str(tmp_path / 'with'), slide=False, save_prob=True, size=(33, 45), analysis=hook)
    gener_target_pseudo(cfg, Model(), loader, str(tmp_path / 'without'), slide=False, save_prob=True, size=(33, 45))
    for i, n in enumerate(names):       # the hook changes nothing of what is written
        a = torch.load(tmp_path / 'with' / (n + '.pt'), weights_only=True)
        assert torch.equal(a, torch.load(tmp_path / 'without' / (n + '.pt'), weights_only=True))
        assert torch.equal(a, torch.from_numpy(soft[i]))
    _write_labels(str(tmp_path / 'labels'), names, gt)
    files = analysis_pseudo_labels(str(tmp_path / 'labels'), str(tmp_path / 'with'), n_classes=6, label_offset=1)
    _assert_summaries_equal(files, hook.summary())
    _assert_summaries_equal(files, ar.summary(ar.fold(ar.new_state(6), tables), 6))
    with pytest.raises(KeyError, match='cls'):
        gener_target_pseudo(cfg, Model(), [(loader[0][0], {'fname': [names[0]]})], str(tmp_path / 'nogt'), slide=False,
                            save_prob=True, size=(33, 45), analysis=PseudoLabelAnalysis(6))
