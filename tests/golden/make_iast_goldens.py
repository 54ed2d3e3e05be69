"""Mint tests/golden/iast.npz from the reference's OWN entropyloss, kldloss, ias_thresh and generate_pseudo
(regda/utils/tools.py:323-398), imported behind the same stubs as make_goldens.py.

Run in the build container only (needs the reference checkout):  python tests/golden/make_iast_goldens.py
Data only: inputs and the reference's outputs.
  reg/c<C>/logits (2, C, 9, 11) f64 (the fp32 cases read it rounded), reg/c<C>/w_<kind> (2, 1, 9, 11) for the weight
  kinds bin (0 / 1), frac (fractions, some 0), zero (all 0: the reference's 0 / 0) and neg (one negative entry); per
  case reg/c<C>/<kind>/{ent,kld}_{loss,grad}{32,64}: the loss and its autograd gradient in fp32 and fp64.
  sel/c<C>/probs (3, 2, C, H, W): three consecutive batches of probabilities; sel/c<C>/{tmp (3, C) f32: ias_thresh per
  batch, thresh (3, C) f64: cls_thresh after each batch, labels (3, 2, H, W) uint8, names (3, 2): the file names}; sel/alpha, beta, gamma.
The labels are what the reference's generate_pseudo itself handed to imsave: its loop runs here as it is, with a stub
model that returns the batches, imsave replaced by a collector, tqdm by the identity and er.viz / the (undefined)
`palette` global by no-ops.  The thresholds, which that loop does not expose, come from the selector restated in
tests/iast_ref.py with the reference's own ias_thresh called as its threshold step; its labels are asserted equal to the
collected ones."""
import os
import sys
import tempfile
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_goldens as mg  # noqa: E402,F401  (installs the stubs, imports the reference)

from regda.utils import tools as rtools  # noqa: E402

import iast_ref  # noqa: E402

CLASSES = (6, 7, 16)
B, H, W = 2, 9, 11
ALPHA, BETA, GAMMA = 0.2, 0.9, 8.0
SEL = {6: (16, 20), 16: (12, 10)}       # class count -> (H, W) of the selector batches


def weights(rng, kind):
    if kind == 'bin':
        return (rng.random((B, 1, H, W)) < 0.4).astype(np.float64)
    if kind == 'frac':
        w = rng.random((B, 1, H, W))
        w[rng.random((B, 1, H, W)) < 0.3] = 0.0
        return w
    if kind == 'zero':
        return np.zeros((B, 1, H, W))
    w = weights(rng, 'frac')
    w[1, 0, 4, 5] = -0.75
    return w


def mint_reg(out):
    for C in CLASSES:
        rng = np.random.default_rng(7300 + C)
        z = rng.standard_normal((B, C, H, W)) * 2.5
        z[0, :, 0, 0] = 0.0                 # a uniform pixel
        z[0, 1, 0, 1] = 120.0               # a saturated pixel: the other probabilities underflow
        out[f'reg/c{C}/logits'] = z
        for kind in ('bin', 'frac', 'zero', 'neg'):
            w = weights(rng, kind).astype(np.float32).astype(np.float64)     # stored as f32: exact in both precisions
            out[f'reg/c{C}/w_{kind}'] = w.astype(np.float32)
            for name, fn in (('ent', rtools.entropyloss), ('kld', rtools.kldloss)):
                for bits, dt in ((32, torch.float32), (64, torch.float64)):
                    x = torch.from_numpy(z).to(dt).requires_grad_(True)
                    loss = fn(x, torch.from_numpy(w).to(dt))
                    loss.backward()
                    out[f'reg/c{C}/{kind}/{name}_loss{bits}'] = loss.detach().numpy()
                    out[f'reg/c{C}/{kind}/{name}_grad{bits}'] = x.grad.numpy()
                print(C, kind, name, float(loss))


class _Model:
    def __init__(self, batches):
        self.batches, self.i = batches, 0

    def eval(self):
        return self

    def __call__(self, image):
        self.i += 1
        return torch.from_numpy(self.batches[self.i - 1])


def mint_sel(out):
    saved = []
    rtools.imsave = lambda path, arr: saved.append((os.path.basename(path), np.array(arr)))
    rtools.tqdm = lambda it: it
    rtools.er = types.SimpleNamespace(viz=types.SimpleNamespace(VisualizeSegmm=lambda *a, **k: (lambda *b, **c: None)))
    rtools.palette = None
    out['sel/alpha'], out['sel/beta'], out['sel/gamma'] = np.float64(ALPHA), np.float64(BETA), np.float64(GAMMA)
    for C, (h, w) in SEL.items():
        # confidences sharpen from batch to batch, so the thresholds keep moving
        probs = np.stack([iast_ref.selector_inputs('softmax', B, C, h, w, seed=50 + 10 * C + k) ** (1 + k)
                          for k in range(3)])
        probs = (probs / probs.sum(2, keepdims=True)).astype(np.float32)
        probs[1, 0, 2] = 0.0                # class 2 wins nowhere in one image
        names = [[f'c{C}_b{k}_{i}.png' for i in range(B)] for k in range(3)]
        loader = [(torch.zeros(B, 3, h, w), {'fname': names[k]}) for k in range(3)]
        del saved[:]
        with tempfile.TemporaryDirectory() as save_dir:      # the reference creates save_dir/pred; nothing is written there
            pred_dir = rtools.generate_pseudo(_Model(probs), loader, save_dir, n_class=C, logger=mg._Log(),
                                              pseudo_dict=dict(pl_alpha=ALPHA, pl_beta=BETA, pl_gamma=GAMMA))
            assert pred_dir == os.path.join(save_dir, 'pred') and [s[0] for s in saved] == sum(names, [])
        labels = np.stack([s[1] for s in saved]).reshape(3, B, h, w)
        assert labels.dtype == np.uint8
        # the thresholds: the restated selector with the reference's own ias_thresh as its threshold step (it takes the
        # per-class lists, the running threshold in front, and the running thresholds again as its weights)
        def ref_thresholds(prepend, confs):
            return rtools.ias_thresh({c: [prepend[c]] + list(confs[c]) for c in range(C)}, C, ALPHA, w=prepend, gamma=GAMMA)
        sel = iast_ref.Selector(C, ALPHA, BETA, GAMMA, thresholds=ref_thresholds)
        tmp, thresh = [], []
        for k in range(3):
            lab = sel.update(probs[k])
            assert np.array_equal(lab, labels[k]), (C, k)
            tmp.append(sel.tmp.copy())
            thresh.append(sel.cls_thresh.copy())
        out[f'sel/c{C}/probs'], out[f'sel/c{C}/labels'] = probs, labels
        out[f'sel/c{C}/names'] = np.array(names)
        out[f'sel/c{C}/tmp'], out[f'sel/c{C}/thresh'] = np.stack(tmp), np.stack(thresh)
        print('sel', C, np.stack(thresh)[-1], 'ignored', float((labels == 0).mean()))


def mint():
    out = {}
    mint_reg(out)
    mint_sel(out)
    path = os.path.join(HERE, 'iast.npz')
    np.savez_compressed(path, **out)
    print('iast.npz', os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    mint()
