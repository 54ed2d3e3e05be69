"""Mint pixel_contrast.npz from the reference's OWN PixelContrastLoss (regda/gast/contrastive.py), on the CPU in fp32.

Run where the reference checkout exists only:
    python tests/golden/make_pixel_contrast_goldens.py
The reference calls `.cuda()` on the tensors it creates: `torch.Tensor.cuda` is made a no-op here (as _refstubs.py does
for its modules), which touches no arithmetic.  `torch.randperm` is wrapped to record every draw; the reference's own
`_hard_anchor_sampling` is run a second time, reseeded, on a feature map that holds the pixel index, which yields the
pixels it selected.
Data only: per case the seed, the inputs (features on a grid of 1/8 as int8 and their scale; labels and predictions as
int8), the recorded draws, the selected pixels, the loss and the reference's autograd gradient at the selected rows
(view-major; every other row of the gradient is checked to be zero).  Also prints the reference's fp32 noise against the
float64 restatement (tests/pixel_contrast_ref.py), which tests/test_pixel_contrast_cpu.py quotes.

Cases (features: unit normal on the grid, times the scale; C = 7 classes):
    b2_k64_16x16_live   labels 64 x 64 (ratio 4, the label pixels the downscale does not read hold another class), two
                        classes of 120 feature pixels per image, label rows 0 to 3 ignored (4 rows of the 64 x 64 label map: the
                        first row, 16 pixels, of the 16 x 16 feature map), 30 % of the predictions
                        flipped, features x 0.1: live exponentials.  A = 4, n_view = 100, N = 400
    b2_k64_16x16_sat    the same with features x 1: every off-diagonal exponential underflows
    b3_k96_16x16_live   labels 32 x 32, features x 0.05; class 1 in images 0 and 1, class 2 in images 1 and 2, a class of
                        90 pixels that does not qualify: A = 5, positives cross anchors
    b3_k64_16x32        four classes of 128 pixels per image, 40 % flipped: A = 12, n_view = 85 = 42 hard + 43 easy,
                        N = 1020; h != w
    b2_k64_few_easy     a class with 20 easy pixels (contrastive.py:85-87)
    b2_k64_few_hard     a class with 20 hard pixels (contrastive.py:88-90)
    b2_k64_hard0        a class without hard pixels: randperm(0)
    b2_k64_absent       image 1 has no class of more than 100 pixels"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import _refstubs  # noqa: E402  (only for the location of the reference checkout)

sys.path.insert(0, _refstubs.REF)
torch.Tensor.cuda = lambda self, *a, **k: self

from pixel_contrast_ref import (NAMES, contrast_restated, pixel_rows, sampling_restated, view_major)  # noqa: E402
from regda.gast.contrastive import PixelContrastLoss  # noqa: E402

C = 7


def bands(h, w, spec):
    """one image's feature-resolution label: `spec` = [(class, pixels)], filled in raster order; the rest ignored"""
    lab = torch.full((h * w,), -1, dtype=torch.int64)
    o = 0
    for c, n in spec:
        lab[o:o + n] = c
        o += n
    assert o <= h * w
    return lab.view(h, w)


def flipped(lab, gen, hard):
    """predictions: per class of `hard` = {class: number of hard pixels} (default 30 %), that many pixels, drawn
    without replacement, get the next class"""
    pred = lab.clone().view(-1)
    for c in torch.unique(lab).tolist():
        if c < 0:
            continue
        idx = (lab.view(-1) == c).nonzero().view(-1)
        n = hard.get(c, int(round(0.3 * idx.numel()))) if isinstance(hard, dict) else int(round(hard * idx.numel()))
        pick = idx[torch.randperm(idx.numel(), generator=gen)[:n]]
        pred[pick] = (c + 1) % C
    return pred.view(lab.shape)


def upscale(lab, ratio):
    """feature-resolution labels -> (h ratio, w ratio): the pixels the nearest downscale reads hold the label, every
    other pixel the next class, so a wrong source position shows"""
    big = ((lab + 1) % C).repeat_interleave(ratio, 0).repeat_interleave(ratio, 1)
    big[::ratio, ::ratio] = lab
    return big


# name -> (k, h, w, label ratio, feature scale, per image the band spec, hard counts or fraction)
SPECS = {
    'b2_k64_16x16_live': (64, 16, 16, 4, 0.1, [[(-1, 16), (0, 120), (1, 120)], [(-1, 16), (2, 120), (3, 120)]], 0.3),
    'b2_k64_16x16_sat': (64, 16, 16, 4, 1.0, [[(-1, 16), (0, 120), (1, 120)], [(-1, 16), (2, 120), (3, 120)]], 0.3),
    'b3_k96_16x16_live': (96, 16, 16, 2, 0.05, [[(0, 128), (1, 128)], [(1, 128), (2, 128)], [(2, 150), (3, 90)]], 0.3),
    'b3_k64_16x32': (64, 16, 32, 1, 0.1, [[(0, 128), (1, 128), (2, 128), (3, 128)], [(1, 128), (2, 128), (3, 128), (4, 128)],
                                         [(2, 128), (3, 128), (4, 128), (5, 128)]], 0.4),
    'b2_k64_few_easy': (64, 16, 16, 1, 0.1, [[(0, 120), (1, 120)], [(5, 60), (6, 60)]], {0: 100}),
    'b2_k64_few_hard': (64, 16, 16, 1, 0.1, [[(0, 120), (1, 120)], [(5, 60), (6, 60)]], {0: 20}),
    'b2_k64_hard0': (64, 16, 16, 1, 0.1, [[(0, 120), (1, 120)], [(5, 60), (6, 60)]], {0: 0}),
    'b2_k64_absent': (64, 16, 16, 1, 0.1, [[(2, 130), (4, 110)], [(0, 100), (1, 100), (3, 40)]], 0.3),
}


def main():
    out, names = {}, []
    noise_l, noise_g = 0.0, 0.0
    for n, name in enumerate(NAMES):
        k, h, w, ratio, scale, spec, hard = SPECS[name]
        seed = 20230331 + (0 if name.endswith('_sat') else n)          # the saturated case shares the live case's inputs
        gen = torch.Generator().manual_seed(seed)
        b = len(spec)
        q = torch.clamp(torch.round(torch.randn(b, k, h, w, generator=gen) * 8.0), -127, 127)
        down = torch.stack([bands(h, w, s) for s in spec])
        predict = torch.stack([flipped(down[i], gen, hard) for i in range(b)])
        labels = torch.stack([upscale(down[i], ratio) for i in range(b)])
        feats = (q / 8.0 * scale).requires_grad_(True)

        perms = []
        real = torch.randperm

        def recording(*a, **kw):
            p = real(*a, **kw)
            perms.append(p.clone())
            return p
        ref = PixelContrastLoss()
        torch.randperm = recording
        try:
            torch.manual_seed(seed)
            loss = ref(feats, labels, predict)
            loss.backward()
            drawn = list(perms)
            # the pixels it selected: its own sampling, reseeded, on a map that holds the pixel index
            torch.manual_seed(seed)
            idx = torch.arange(h * w, dtype=torch.float32).view(1, -1, 1).expand(b, -1, -1)
            X_, y_ = ref._hard_anchor_sampling(idx, down.view(b, -1), predict.view(b, -1))
        finally:
            torch.randperm = real
        sel = X_[:, :, 0].long()
        classes = y_.long()
        rsel, anchors, n_view = sampling_restated(labels, predict, (h, w), drawn)
        assert torch.equal(rsel, sel) and [a[1] for a in anchors] == classes.tolist(), name
        rows, cls = view_major(sel, anchors, h * w)
        assert rows.unique().numel() == rows.numel()
        g = pixel_rows(feats.grad)
        other = torch.ones(g.shape[0], dtype=torch.bool)
        other[rows] = False
        assert not g[other].any(), name
        rl, rg = contrast_restated(pixel_rows(feats.detach())[rows], cls)
        nl = abs(loss.item() - rl.item()) / abs(rl.item())
        ng = ((g[rows].double() - rg).norm() / rg.norm()).item()
        noise_l, noise_g = max(noise_l, nl), max(noise_g, ng)
        print(f'{name}: A {len(anchors)} n_view {n_view} N {rows.numel()} hard_keep {[a[2] for a in anchors]} loss {loss.item():.6g} '
              f'fp32 noise against float64: loss {nl:.3g} grad {ng:.3g}')
        names.append(name)
        out.update({name + '_seed': np.int64(seed), name + '_scale': np.float64(scale),
                    name + '_sel': sel.numpy().astype(np.int16), name + '_classes': classes.numpy().astype(np.int8),
                    name + '_loss': loss.detach().numpy(), name + '_grad': g[rows].numpy()})
        if name.endswith('_sat'):         # same seed: the same grid values, labels, predictions and draws as the live case
            live = name[:-4] + '_live'
            assert all(torch.equal(a, b) for a, b in zip(drawn, live_drawn)) and np.array_equal(out[live + '_q'], q.numpy())
            out[name + '_like'] = np.array(live)
        else:
            live_drawn = drawn
            out.update({name + '_q': q.numpy().astype(np.int8), name + '_labels': labels.numpy().astype(np.int8),
                        name + '_predict': predict.numpy().astype(np.int8),
                        name + '_perms': (torch.cat(drawn) if drawn else torch.zeros(0)).numpy().astype(np.int16),
                        name + '_perm_lens': np.array([p.numel() for p in drawn], np.int32)})
    out['names'] = np.array(names)
    path = os.path.join(HERE, 'pixel_contrast.npz')
    np.savez_compressed(path, **out)
    print('reference fp32 noise (largest over the cases): loss', noise_l, 'grad', noise_g)
    print('wrote pixel_contrast.npz', os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
