"""Mint whiten.npz from the reference's OWN ClassWareWhitening (imported behind the stubs of _refstubs.py, on the CPU).

Run where the reference checkout exists only:
    python tests/golden/make_whiten_goldens.py
Data only: inputs, the reference's loss and its autograd gradient with respect to `feats`.

Cases (features on a grid of 1/32, stored as int8; labels int8 with -1 = ignored):
    k64g1_c6    (2, 64, 8, 12), groups 1, 6 classes: class 5 has no pixel, class 4 exactly one, 15 % ignored
    k64g2_c7    (2, 64, 8, 12), groups 2, 7 classes: class 2 has no pixel, class 6 exactly one
    k256g4_c16  (2, 256, 8, 12), groups 4, 16 classes: class 9 has no pixel, class 15 exactly one
    hand        the 6 x 4 example of the reference's __main__ (k = 4, class_ids [1, 2], groups 1), for which the
                reference prints 12.4375; stored under hand_* as float32 features"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _refstubs  # noqa: E402

_refstubs.install()

from regda.gast.class_ware_whiten import ClassWareWhitening  # noqa: E402


def labels_for(rng, shape, C, empty, single, ignored=0.15):
    """blocky labels over the classes other than `empty` and `single`, some pixels ignored, one pixel of `single`"""
    b, h, w = shape
    pool = np.array([c for c in range(C) if c not in (empty, single)])
    cells = pool[rng.integers(0, len(pool), (b, h // 2, w // 2))]
    lab = np.repeat(np.repeat(cells, 2, 1), 2, 2)
    noise = rng.random(shape) < 0.3
    lab = np.where(noise, pool[rng.integers(0, len(pool), shape)], lab)
    lab = np.where(rng.random(shape) < ignored, -1, lab)
    lab[b - 1, h // 2, w // 3] = single
    assert (lab == empty).sum() == 0 and (lab == single).sum() == 1
    return lab.astype(np.int8)


def main():
    rng = np.random.default_rng(20230331)
    out = {}
    names = []
    for name, k, groups, C, empty, single, scale in (('k64g1_c6', 64, 1, 6, 5, 4, 1.0), ('k64g2_c7', 64, 2, 7, 2, 6, 1.25),
                                                     ('k256g4_c16', 256, 4, 16, 9, 15, 0.75)):
        shape = (2, k, 8, 12)
        q = np.clip(np.round(rng.standard_normal(shape) * 32.0 * 0.8), -127, 127).astype(np.int8)
        lab = labels_for(rng, (2, 8, 12), C, empty, single)
        feats = (torch.from_numpy(q.astype(np.float32) / 32.0) * scale).requires_grad_(True)
        crit = ClassWareWhitening(class_ids=range(C), groups=groups)
        loss = crit(feats, torch.from_numpy(lab.astype(np.int64)))
        loss.backward()
        names.append(name)
        out.update({name + '_q': q, name + '_scale': np.float32(scale), name + '_lab': lab, name + '_C': np.int32(C),
                    name + '_groups': np.int32(groups), name + '_loss': loss.detach().numpy(),
                    name + '_grad': feats.grad.numpy()})
    # the demo inputs of the reference's class_ware_whiten.py __main__ (the 6 x 4 matrix and its mask): values only
    a = [[2, 1, 3, 0], [5, 6, 7, 8], [1, 2, 3, 4], [2, 3, 4, 5], [0, 1, 0, 1], [5, 1, 3, 1]]
    fe = torch.tensor(a, dtype=torch.float32).reshape(1, 1, 6, 4).permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    mi = torch.tensor([1, 0, 0, 1, 0, 0], dtype=torch.int64).reshape(1, 1, 6)
    loss = ClassWareWhitening(class_ids=[1, 2], groups=1)(fe, mi)
    loss.backward()
    assert abs(loss.item() - 12.4375) < 1e-5, loss.item()
    out.update(hand_feats=fe.detach().numpy(), hand_lab=mi.numpy().astype(np.int8), hand_class_ids=np.array([1, 2], np.int32),
               hand_loss=loss.detach().numpy(), hand_grad=fe.grad.numpy())
    out['names'] = np.array(names)
    np.savez_compressed(os.path.join(HERE, 'whiten.npz'), **out)
    print('wrote whiten.npz', {k: getattr(v, 'shape', None) for k, v in out.items()})


if __name__ == '__main__':
    main()
