"""Mint tests/golden/gdp.npz from the reference's OWN GDPLoss (regda/gast/balance.py:218-303, through
regda/utils/tools.py: loss_calc) and Aligner.get_prototype_weight_4pixel (regda/gast/alignment.py:267-281), imported
behind the same stubs as make_goldens.py.

Run in the build container only (needs the reference checkout):  python tests/golden/make_gdp_goldens.py
Data only: inputs and the reference's outputs.  Per class count C in (6, 7) the file holds one set of base inputs
`c<C>/...` -- logits p1, p2 (2, C, 5, 7), labels (2, 37, 300) with ignored pixels, features (2, 64, 5, 7), prototypes
(C, 64) -- and the reference's prototype weights `c<C>/pw` of those labels.  Each case `<name>/...` stores what it
changes of the base inputs, and per call k (suffix '' / '1') the loss, both logit gradients, acc_sum, bins_weight and
the balancer's frequencies.  Label pixels whose |p_y - 1| lies within 1e-4 of a bin edge in either head are ignored
(as make_loss_goldens.py does for GHM), so that two correct implementations bin every pixel alike."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_goldens as mg  # noqa: E402  (installs the stubs, imports the reference)

from regda.gast.alignment import Aligner  # noqa: E402
from regda.gast.balance import GDPLoss  # noqa: E402
from regda.utils.tools import loss_calc  # noqa: E402

import loss_ref  # noqa: E402

B, h, w, H, W, K = 2, 5, 7, 37, 300, 64

# name, class count, GDPLoss options, input options, calls
CASES = [
    ('plain6', 6, {}, {}, 1),
    ('plain7', 7, {}, {}, 1),
    ('cb6', 6, dict(class_balance=True), {}, 1),
    ('cb7', 7, dict(class_balance=True), {}, 1),
    ('pr6', 6, dict(prototype_refine=True), {}, 1),
    ('pr7', 7, dict(prototype_refine=True), {}, 1),
    ('both6', 6, dict(class_balance=True, prototype_refine=True), {}, 1),
    ('both7', 7, dict(class_balance=True, prototype_refine=True), {}, 1),
    ('mom0', 6, dict(momentum=0.0), {}, 1),
    ('state', 7, dict(class_balance=True, prototype_refine=True), {}, 2),
    ('ignored', 6, {}, dict(all_ignored=True), 1),
    ('oneclass', 7, {}, dict(one_class=3), 1),
    ('saturated', 6, {}, dict(saturate=True), 1),
    ('single', 7, dict(class_balance=True), dict(single=True), 1),
]


def drop_near_edges(lab, preds):
    for p in preds:
        near = loss_ref.near_boundary('ghm', loss_ref.up(p, (H, W)), lab, eps=1e-4).reshape(lab.shape)
        lab = torch.where(near, torch.full_like(lab, -1), lab)
    return lab


def base_inputs(C):
    rng = np.random.default_rng(9100 + C)
    f32 = lambda *s: torch.from_numpy(rng.standard_normal(s).astype(np.float32))
    p1, p2 = f32(B, C, h, w) * 2, f32(B, C, h, w) * 2
    lab = torch.from_numpy(rng.integers(0, C, (B, H, W)))
    lab = torch.where(torch.from_numpy(rng.random((B, H, W)) < 0.15), torch.full_like(lab, -1), lab)
    lab = drop_near_edges(lab, (p1, p2))
    protos, feat = f32(C, K), f32(B, K, h, w)
    feat[0, :, 1, 2] = protos[2] + 0.05 * f32(K)        # one pixel close to a prototype: a large similarity
    al = Aligner(logger=mg._Log(), feat_channels=K, class_num=C, ignore_label=-1, decay=0.996, resume=None)
    al.prototypes = protos.clone()
    pw = al.get_prototype_weight_4pixel(feat, lab, temp=2.0)
    return dict(p1=p1, p2=p2, lab=lab, feat=feat, protos=protos, pw=pw)


def mint():
    out = {}
    base = {C: base_inputs(C) for C in (6, 7)}
    for C, d in base.items():
        for k, v in d.items():
            out[f'c{C}/{k}'] = v.numpy().astype(np.int8) if k == 'lab' else v.numpy()
    for name, C, opts, inp, calls in CASES:
        d = base[C]
        p1, p2, lab = d['p1'].clone(), d['p2'].clone(), d['lab'].clone()
        rec = {}
        if inp.get('all_ignored'):
            lab = torch.full_like(lab, -1)
        if inp.get('one_class') is not None:
            # one class everywhere and logits that agree with it: g falls into the lowest bins (and, symmetrised, the
            # highest), the bins between stay empty
            lab = torch.where(lab >= 0, torch.full_like(lab, inp['one_class']), lab)
            p1[:, inp['one_class']] += 12.0
            p2[:, inp['one_class']] += 12.0
        if inp.get('saturate'):
            # logits of +-40 in a block: p_y rounds to 1 there (g == 0 exactly: counted in bin 0, bucket 0, weight 0)
            p1[0, :, :2, :3] = -40.0
            p2[0, :, :2, :3] = -40.0
            p1[0, 2, :2, :3] = 40.0
            p2[0, 2, :2, :3] = 40.0
            lab[0, :9, :90] = 2
        if inp:
            lab = drop_near_edges(lab, (p1, p2))
            rec.update(p1=p1.numpy(), p2=p2.numpy(), lab=lab.numpy().astype(np.int8))
        fn = GDPLoss(bins=30, class_num=C, ignore_label=-1, temp=0.5, **opts)
        if opts.get('prototype_refine'):
            fn.set_prototype_weight_4pixel(d['pw'])
        for k in range(calls):
            q1, q2 = p1.clone().requires_grad_(True), p2.clone().requires_grad_(True)
            if inp.get('single'):
                loss = loss_calc(q1, lab, fn, multi=False)
            else:
                loss = loss_calc([q1, q2], lab, fn, multi=True)
            loss.backward()
            sfx = '' if k == 0 else str(k)
            rec.update({'loss' + sfx: loss.detach().numpy(), 'g1' + sfx: q1.grad.numpy(),
                        'acc' + sfx: fn.acc_sum.detach().numpy().copy(),
                        'bw' + sfx: fn.bins_weight.detach().numpy().copy(),
                        'freq' + sfx: fn.class_balancer.freq.numpy().copy()})
            if not inp.get('single'):
                rec['g2' + sfx] = q2.grad.numpy()
        if inp.get('saturate'):
            g = loss_ref.ghm_g(loss_ref.up(p1, (H, W)), lab)
            assert int((g == 0).sum()) > 0, 'the saturated case must hold pixels with g == 0 exactly'
        for k, v in rec.items():
            out[f'{name}/{k}'] = v
        print(name, float(rec['loss']))
    np.savez_compressed(os.path.join(HERE, 'gdp.npz'), **out)
    print('gdp.npz', os.path.getsize(os.path.join(HERE, 'gdp.npz')), 'bytes')


if __name__ == '__main__':
    mint()
