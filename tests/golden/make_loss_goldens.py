"""Mint tests/golden/losses.npz from the reference's OWN loss classes (regda/gast/balance.py: OhemCrossEntropy,
FocalLoss, GHMLoss, UPSLoss, UVEMLoss, ClassBalance; regda/utils/tools.py: loss_calc; balance.py: loss_calc_uvem),
imported behind the same stubs as make_goldens.py.

Run in the build container only (needs the reference checkout):  python tests/golden/make_loss_goldens.py
Data only: inputs and the reference's outputs.  Each case `<name>` stores its inputs (p1, p2 at 8 x 8, labels at 32 x 32
with ignored pixels, the soft label where the loss reads one), the loss, both gradients and the state that follows
(`freq` of a ClassBalance, `acc` of GHMLoss).  The inputs are redrawn until no decision value lies within 1e-4 of a
boundary (tests/loss_ref.near_boundary), except where a case is about that boundary."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_goldens as mg  # noqa: E402,F401  (installs the stubs, imports the reference)

from regda.gast.balance import (ClassBalance, FocalLoss, GHMLoss, OhemCrossEntropy, UPSLoss, UVEMLoss,  # noqa: E402
                                loss_calc_uvem)
from regda.utils.tools import loss_calc  # noqa: E402

import loss_ref  # noqa: E402

B, C, h, H = 2, 6, 8, 32
F0 = np.array([0.4, 0.25, 0.1, 0.1, 0.1, 0.05], np.float32)     # a skewed ClassBalance start, so the weights differ


def draw(rng, kind, confident=False, all_ignored=False, saturate=False, zeros=0.0, onehot=False):
    p1 = torch.from_numpy((rng.standard_normal((B, C, h, h)) * 2).astype(np.float32))
    p2 = torch.from_numpy((rng.standard_normal((B, C, h, h)) * 2).astype(np.float32))
    lab = torch.from_numpy(rng.integers(0, C, (B, H, H)))
    if confident:
        # two close heads and labels = their prediction almost everywhere: few losses above -log(0.7), the top-k branch
        base = torch.from_numpy((rng.standard_normal((B, C, h, h)) * 24).astype(np.float32))
        p1 = base + torch.from_numpy((rng.standard_normal((B, C, h, h)) * 0.2).astype(np.float32))
        p2 = base + torch.from_numpy((rng.standard_normal((B, C, h, h)) * 0.2).astype(np.float32))
        lab = loss_ref.up(base, (H, H)).argmax(1)
        flip = torch.from_numpy(rng.random((B, H, H)) < 0.03)
        lab = torch.where(flip, (lab + 1) % C, lab)
    if saturate:
        # a block of logits so large that p_y rounds to 1 (g = 0: counted in bin 0, weight 0)
        p1[0, :, :3, :3] = 0.0
        p2[0, :, :3, :3] = 0.0
        p1[0, 2, :3, :3] = 60.0
        p2[0, 2, :3, :3] = 60.0
        lab[0, :9, :9] = 2
    ign = torch.from_numpy(rng.random((B, H, H)) < 0.15)
    lab = torch.where(ign, torch.full_like(lab, -1), lab)
    if all_ignored:
        lab = torch.full_like(lab, -1)
    soft = None
    if kind in ('ups', 'uvem'):
        soft = torch.softmax(torch.from_numpy((rng.standard_normal((B, C, H, H)) * 3).astype(np.float32)), 1)
        if zeros:
            # exact zeros in the soft label: u = NaN, neither gated nor counted
            z = torch.from_numpy(rng.random((B, 1, H, H)) < zeros)
            hot = torch.nn.functional.one_hot(lab.clamp(min=0), C).permute(0, 3, 1, 2).float()
            soft = torch.where(z, hot, soft)
        if onehot:
            soft = torch.nn.functional.one_hot(lab.clamp(min=0), C).permute(0, 3, 1, 2).float()
    return p1, p2, lab, soft


def clean(kind, p1, p2, lab, soft, eps=1e-4):
    """no decision value within eps of a boundary, in either head (tests/loss_ref.near_boundary)"""
    for p in (p1, p2):
        pf = loss_ref.up(p, (H, H))
        if bool(loss_ref.near_boundary(kind, pf, lab, soft, eps=eps).any()):
            return False
    return True


CASES = [
    # name, kind, draw options, --bcs / --bct balancer, calls (GHM: two consecutive loss_calc calls)
    ('ohem', 'ohem', {}, False),
    ('ohem_topk', 'ohem', dict(confident=True), False),
    ('ohem_bal', 'ohem', {}, True),
    ('ohem_ignored', 'ohem', dict(all_ignored=True), False),
    ('focal', 'focal', {}, False),
    ('ghm', 'ghm', dict(saturate=True), False),
    ('ups', 'ups', {}, False),
    ('ups_bal', 'ups', {}, True),
    ('uvem', 'uvem', {}, False),
    ('uvem_bal', 'uvem', {}, True),
    ('uvem_zeros', 'uvem', dict(zeros=0.1), False),
    ('ups_zeros', 'ups', dict(zeros=0.1), False),
    ('uvem_onehot', 'uvem', dict(onehot=True), False),
]


def ref_loss(kind, balancer, ghm):
    if kind == 'ohem':
        return OhemCrossEntropy(ignore_label=-1, class_balancer=balancer)
    if kind == 'focal':
        return FocalLoss(gamma=2.0, reduction='mean', ignore_label=-1)
    if kind == 'ghm':
        return ghm
    if kind == 'ups':
        return UPSLoss(threshold=0.7, class_balancer=balancer, class_num=C, ignore_label=-1)
    return UVEMLoss(m=0.2, threshold=0.7, gamma=4.0, class_balancer=balancer, class_num=C, ignore_label=-1)


def mint():
    out = {}
    for ci, (name, kind, opts, bal) in enumerate(CASES):
        rng = np.random.default_rng(7000 + ci)
        deliberate = opts.get('all_ignored') or opts.get('zeros') or opts.get('onehot')
        for _ in range(200):
            p1, p2, lab, soft = draw(rng, kind, **opts)
            if kind == 'ghm':
                # 30 edges: about one pixel in a hundred lies near one; those pixels are ignored instead
                for p in (p1, p2):
                    near = loss_ref.near_boundary(kind, loss_ref.up(p, (H, H)), lab, eps=1e-4).reshape(lab.shape)
                    lab = torch.where(near, torch.full_like(lab, -1), lab)
            if deliberate or clean(kind, p1, p2, lab, soft):
                break
        else:
            raise RuntimeError(f'{name}: no draw without boundary values')
        balancer = None
        if bal:
            balancer = ClassBalance(class_num=C, ignore_label=-1, decay=0.9, temperature=2.0)
            balancer.freq = torch.from_numpy(F0.copy())
        ghm = GHMLoss(bins=30, momentum=0.99, ignore_label=-1) if kind == 'ghm' else None
        fn = ref_loss(kind, balancer, ghm)
        calls = 2 if kind == 'ghm' else 1
        rec = {'p1': p1.numpy(), 'p2': p2.numpy(), 'lab': lab.numpy().astype(np.int8)}
        if soft is not None:
            rec['soft'] = soft.numpy()
        for k in range(calls):
            q1, q2 = p1.clone().requires_grad_(True), p2.clone().requires_grad_(True)
            if kind in ('ups', 'uvem'):
                loss = loss_calc_uvem([q1, q2], lab, soft, fn, multi=True)
            else:
                loss = loss_calc([q1, q2], lab, fn, multi=True)
            loss.backward()
            sfx = '' if k == 0 else str(k)
            rec.update({'loss' + sfx: loss.detach().numpy(), 'g1' + sfx: q1.grad.numpy(), 'g2' + sfx: q2.grad.numpy()})
            if ghm is not None:
                rec['acc' + sfx] = ghm.acc_sum.numpy().copy()
        if balancer is not None:
            rec['freq'] = balancer.freq.numpy().copy()
        for k, v in rec.items():
            out[f'{name}/{k}'] = v
        print(name, float(rec['loss']))
    np.savez_compressed(os.path.join(HERE, 'losses.npz'), **out)


if __name__ == '__main__':
    mint()
