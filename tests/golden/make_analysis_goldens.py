"""Mint tests/golden/pseudo_analysis.npz from the reference's OWN analysis_pseudo_labels and range_static
(regda/gast/pseudo_generation.py:158-235), imported behind the same stubs as make_goldens.py.  No reference source is
copied: its function runs as it is.

Run in the build container only (needs the reference checkout):  python tests/golden/make_analysis_goldens.py
Data only, and outputs only: the inputs are tests/analysis_ref.py's seeded makers (inputs(kind, b, C, H, W, SEED)).
Per case <kind>/c<C>/<H>x<W>/: acc_list, diffi_list, cnt_true_list, cnt_used_list (f64 [100]): what the reference's
function hands to its three figures at the end of its loop.  What is replaced around it, in its module's namespace:
`glob` lists one name per image of the batch, `cv2.imread` and `torch.load` hand out that image's ground truth and soft
label from the maker's arrays, `Tensor.cuda` is the identity (_refstubs), `tqdm` the identity, and show_tradeoff /
plot_noise_rate / plot_cnt are collectors.  one_bin/result: the reference's range_static on one bin of one image, on maps
built here from the contract (oracle selection, analysis_ref's entropy order and difficulty)."""
import math
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_goldens as mg  # noqa: E402,F401  (installs the stubs, imports the reference)

from regda.gast import pseudo_generation as rpg  # noqa: E402

from oracle import labels as olab  # noqa: E402

import analysis_ref as ar  # noqa: E402

SEED = 20
ONE_BIN = ('softmax', 6, 33, 45, 0, 7)      # kind, C, H, W, image, bin


def run_reference(soft, gt):
    """The reference's analysis_pseudo_labels over the images of one batch -> the lists its figures receive."""
    n = soft.shape[0]
    files = {f'/labels/{i:03d}.png': gt[i] for i in range(n)}
    files.update({f'/pseudo/{i:03d}.pt': torch.from_numpy(soft[i].copy()) for i in range(n)})
    got = {}

    def tradeoff(unce, diffi, cnt_used_list, *a, **k):
        got['tradeoff'] = (list(unce), list(diffi), np.array(cnt_used_list))

    def noise_rate(x, acc_list, diffi_list, num_classes=6, **k):
        got.update(x=list(x), acc_list=np.array([float(v) for v in acc_list]),
                   diffi_list=np.array([float(v) for v in diffi_list]), n_classes=num_classes)

    def cnt(x, y1, y2):
        got.update(cnt_true_list=np.array(y1, dtype=np.float64), cnt_used_list=np.array(y2, dtype=np.float64))

    saved = {k: getattr(rpg, k, None) for k in ('glob', 'cv2', 'tqdm', 'show_tradeoff', 'plot_noise_rate', 'plot_cnt')}
    torch_load = torch.load
    try:
        rpg.glob = lambda pattern: [f for f in files if f.startswith(os.path.dirname(pattern)) and f.endswith(pattern[-3:])][::-1]
        rpg.cv2 = types.SimpleNamespace(IMREAD_UNCHANGED=-1, imread=lambda path, flag: files[path].copy())
        rpg.tqdm = lambda it: it
        rpg.show_tradeoff, rpg.plot_noise_rate, rpg.plot_cnt = tradeoff, noise_rate, cnt
        torch.load = lambda path, map_location=None: files[path].clone()
        rpg.analysis_pseudo_labels(label_dir='/labels', pseudo_dir='/pseudo', ignore_label=-1, n_classes=soft.shape[1])
    finally:
        torch.load = torch_load
        for k, v in saved.items():
            setattr(rpg, k, v)
    assert got['n_classes'] == soft.shape[1] and got['x'] == ar.edges(soft.shape[1])[0]
    assert got['tradeoff'][1] == list(got['diffi_list'][:50]) and np.array_equal(got['tradeoff'][2], got['cnt_used_list'][:50])
    return {k: got[k] for k in ('acc_list', 'diffi_list', 'cnt_true_list', 'cnt_used_list')}


def mint():
    out = {}
    for b, C, H, W in ar.shapes():
        for kind in ar.KINDS:
            soft, gt = ar.inputs(kind, b, C, H, W, SEED)
            got = run_reference(soft, gt)
            for k, v in got.items():
                out[f'{kind}/c{C}/{H}x{W}/{k}'] = v
            print(kind, C, H, W, 'used', int(got['cnt_used_list'].sum()), 'true', int(got['cnt_true_list'].sum()),
                  'bins hit', int((got['diffi_list'] != 0).sum()))
    kind, C, H, W, img, i = ONE_BIN
    soft, gt = ar.inputs(kind, 2, C, H, W, SEED)
    soft, gt = soft[img:img + 1], gt[img:img + 1]
    pseudo = olab.pseudo_selection(soft, ar.TOP, ar.LOW, -1)
    pseudo[pseudo == -1] = C
    entropy = torch.from_numpy(ar.entropy64(soft).astype(np.float32))
    step = math.log(C) / ar.R
    res = rpg.range_static(entropy, torch.from_numpy(ar.difficulty(soft, gt)), torch.from_numpy(pseudo), torch.from_numpy(gt),
                           1.0 * i * step, 1.0 * i * step + step, C)
    out['one_bin/result'] = np.array([float(r) for r in res])
    path = os.path.join(HERE, 'pseudo_analysis.npz')
    np.savez_compressed(path, **out)
    print('pseudo_analysis.npz', os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    mint()
