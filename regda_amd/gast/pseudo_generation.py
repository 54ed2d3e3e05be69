"""pseudo_selection, gener_target_pseudo and the pseudo-label analysis -- mirror of regda/gast/pseudo_generation.py:59-235
(the matplotlib figures are left to the caller)."""
import glob
import math
import os

import numpy as np

import torch

from .. import ops


def pseudo_selection(mask, cutoff_top=0.8, cutoff_low=0.6, return_type='ndarray', ignore_label=-1):
    """soft (b,c,h,w) probabilities -> hard labels (b,h,w) int64; same arguments, asserts and
    return types as the reference."""
    assert return_type in ['ndarray', 'tensor']
    ret = ops.pseudo_select(mask, cutoff_top, cutoff_low, ignore_label, check=True)
    if return_type == 'ndarray':
        return ret.cpu().numpy()
    return ret


def range_static(entropy, difficulty, pseudo, gt, v_fr=0.0, v_to=1.0, n_classes=6):
    """One entropy bin of the analysis, for callers with their own maps (pseudo_generation.py:224-235), in plain torch
    ops on whatever device the maps live on: entropy / difficulty float, pseudo / gt int, all of one shape, ignored pseudo
    labels = n_classes -> (cnt_true, cnt_used, acc, diffi) as 0-d tensors.  A pixel is outside the bin where
    entropy < v_fr or entropy >= v_to (so a NaN entropy is inside every bin, except for diffi's pixel count)."""
    outside = (entropy < v_fr) | (entropy >= v_to)
    kept = torch.where(outside, torch.full_like(pseudo, n_classes), pseudo)
    cnt_true = (kept == gt).sum()
    cnt_used = (kept != n_classes).sum()
    acc = 1.0 * cnt_true / (cnt_used + 1e-7)
    inside = (entropy >= v_fr) & (entropy < v_to)
    diffi = 1.0 * torch.where(outside, torch.zeros_like(difficulty), difficulty).sum() / (inside.sum() + 1e-7)
    return cnt_true, cnt_used, acc, diffi


def entropy_bin_edges(n_classes, range_cnt):
    """-> (x, lo, hi): the bin origins as Python floats and the f32 edges the reference's comparisons see
    (pseudo_generation.py:168, :196-197: a float32 tensor is compared with a Python scalar in float32)."""
    step = math.log(n_classes) / range_cnt
    x = [i * step for i in range(range_cnt)]
    lo = np.array([1.0 * i * step for i in range(range_cnt)], dtype=np.float32)
    hi = np.array([1.0 * i * step + step for i in range(range_cnt)], dtype=np.float32)
    return x, lo, hi


class PseudoLabelAnalysis:
    """The tables behind the UVEM parameters (analysis_pseudo_labels, pseudo_generation.py:158-221): every pixel is binned
    by the entropy of its soft label; per bin, how many pseudo labels are used, how many of them are right and how hard
    the pixels are.  update() takes device tensors and makes no host sync: one pass over the soft labels
    (rgda_pseudo_analysis) and a fold into a running state on the device (rgda_pseudo_analysis_fold); summary() reads
    the state back once."""

    def __init__(self, n_classes=6, ignore_label=-1, cutoff_top=0.8, cutoff_low=0.6, range_cnt=100):
        ops.check_class_count(n_classes, 'PseudoLabelAnalysis')
        if not 1 <= int(range_cnt) <= ops.ANALYSIS_MAX_BINS:
            raise ValueError(f'PseudoLabelAnalysis: range_cnt {range_cnt}; the kernels serve 1 .. {ops.ANALYSIS_MAX_BINS} bins')
        self.n_classes, self.ignore_label, self.range_cnt = int(n_classes), int(ignore_label), int(range_cnt)
        self.cutoff_top, self.cutoff_low = float(cutoff_top), float(cutoff_low)
        self.x, self._lo, self._hi = entropy_bin_edges(self.n_classes, self.range_cnt)
        self._dev = self._state = self._tables = None

    def _on(self, device):
        if self._dev is None:
            self._dev = (torch.from_numpy(self._lo).to(device), torch.from_numpy(self._hi).to(device))
            pending, self._state = self._state, ops.pseudo_analysis_state(self.n_classes, self.range_cnt, device)
            if pending is not None:         # a state loaded before the first update
                self._state.copy_(pending)
        return self._dev

    def update(self, soft, gt):
        """soft f32 (b, C, H, W) probabilities, gt int64 (b, H, W) with ignore_label where there is no ground truth."""
        if soft.dim() != 4 or soft.shape[1] != self.n_classes:
            raise ValueError(f'PseudoLabelAnalysis.update: soft {tuple(soft.shape)} is not (b, {self.n_classes}, H, W)')
        lo, hi = self._on(soft.device)
        self._tables = ops.pseudo_analysis(soft, gt, lo, hi, self.cutoff_top, self.cutoff_low, self.ignore_label,
                                           tables=self._tables)
        ops.pseudo_analysis_fold(self._tables, soft.shape[0], self.n_classes, self.range_cnt, self._state)

    def reset(self):
        if self._state is not None:
            self._state.zero_()

    def _host_state(self):
        if self._state is None:
            return torch.zeros(ops.lib().size('rgda_pseudo_analysis_fold_workspace', self.n_classes, self.range_cnt),
                               dtype=torch.uint8)
        return self._state.cpu()

    def summary(self):
        """One readback -> dict: the reference's x, acc_list, diffi_list, cnt_true_list, cnt_used_list (:200-211; the two
        counts as int64), and used / true int64 [R][C] (the counts per pseudo class), in_bin int64 [R], nan_pixels (the
        pixels with a NaN entropy: in every bin's counts and difficulty, in no bin's in_bin), images.  ValueError if an
        input was outside the contract."""
        R = self.range_cnt
        v = {k: t.numpy() for k, t in ops.pseudo_analysis_state_views(self._host_state(), self.n_classes, R).items()}
        flag = int(v['flag'][0])
        if flag & 1:
            raise ValueError('PseudoLabelAnalysis: flag bit 0: a probability is outside [0, 1] or not finite')
        if flag & 2:
            raise ValueError(f'PseudoLabelAnalysis: flag bit 1: a ground-truth label is outside [0, {self.n_classes}) and is '
                             f'not ignore_label={self.ignore_label}')
        used = v['total_used'][:R] + v['total_used'][R]
        true = v['total_hit'][:R] + v['total_hit'][R]
        return dict(x=list(self.x), acc_list=list(v['acc_sum'] / (v['acc_cnt'] + 1e-7)),
                    diffi_list=list(v['diffi_sum'] / (v['diffi_cnt'] + 1e-7)), cnt_true_list=true.sum(1),
                    cnt_used_list=used.sum(1), used=used, true=true, in_bin=v['total_inbin'][:R].copy(),
                    nan_pixels=int(v['total_inbin'][R]), images=int(v['images'][0]))

    def state_dict(self):
        return dict(n_classes=self.n_classes, ignore_label=self.ignore_label, cutoff_top=self.cutoff_top,
                    cutoff_low=self.cutoff_low, range_cnt=self.range_cnt, state=self._host_state().clone())

    def load_state_dict(self, sd):
        for k in ('n_classes', 'ignore_label', 'cutoff_top', 'cutoff_low', 'range_cnt'):
            if sd[k] != getattr(self, k):
                raise ValueError(f'PseudoLabelAnalysis.load_state_dict: {k} is {sd[k]} in the state, {getattr(self, k)} here')
        state = torch.as_tensor(sd['state'], dtype=torch.uint8)
        if self._state is not None and state.numel() == self._state.numel():
            self._state.copy_(state)
        elif self._state is None and state.numel() == self._host_state().numel():
            self._state = state.clone()         # moved to the device by the first update
        else:
            raise ValueError('PseudoLabelAnalysis.load_state_dict: the state has the wrong size')


def analysis_pseudo_labels(label_dir='data/IsprsDA/Vaihingen/ann_dir/train', pseudo_dir='log/GAST/2vaihingen/pseudo_label_1000',
                           ignore_label=-1, n_classes=6, label_offset=0):
    """The reference's loop over a directory of ground-truth `*.png` and one of soft labels `*.pt` ((C, h, w) f32, as
    gener_target_pseudo(save_prob=True) writes them), both sorted, equal counts asserted (pseudo_generation.py:158-211)
    -> PseudoLabelAnalysis.summary().  label_offset is subtracted from the decoded PNG (an image cannot hold -1: labels
    stored as class + 1 with 0 = ignored take label_offset=1).  Plotting is left to the caller."""
    from PIL import Image
    labels = sorted(glob.glob(os.path.join(label_dir, '*.png')))
    pseudos = sorted(glob.glob(os.path.join(pseudo_dir, '*.pt')))
    assert len(labels) == len(pseudos)
    analysis = PseudoLabelAnalysis(n_classes, ignore_label)
    for lbl, pt in zip(labels, pseudos):
        gt = torch.from_numpy(np.asarray(Image.open(lbl)).astype(np.int64) - label_offset).unsqueeze(0).cuda()
        cls = torch.load(pt, map_location='cpu', weights_only=True).unsqueeze(0).cuda()
        analysis.update(cls, gt)
    return analysis.summary()


def gener_target_pseudo(_cfg, model, pseudo_loader, save_pseudo_label_path, slide=True, save_prob=False,
                        size=(1024, 1024), ignore_label=-1, window_batch=None, analysis=None, scales=None):
    """Teacher pass over the target set (pseudo_generation.py:96-153): eval-mode sliding-window + 8-view TTA
    inference per tile.  `save_prob=True` writes the soft labels the SSL loader reads back -- a (C, h, w) fp32 CPU tensor
    `torch.save`d as `<fname>.pt` (pseudo_generation.py:135-136, basedata.py:86).  `save_prob=False` writes the HARD
    labels as the reference does (pseudo_generation.py:143-150): pseudo_selection (or, with `_cfg.PSEUDO_SELECT` false,
    the argmax) of the tile's probabilities, + 1, reshaped to `size`, as a single-channel uint8 image named `<fname>` --
    the reference hands that array to cv2.imwrite; here Pillow writes it (the container's bytes differ, the decoded
    pixels are the same array).  The colour visualisations (VisualizeSegmm) are not reproduced.
    window_batch=K (with slide): consecutive tiles of one shape are grouped until they hold K windows, which go through
    the model K x 8 views at a time (pre_slide(window_batch=K)); the files are written per tile, in loader order.
    scales (with slide): multi-scale testing -- the probabilities are predict_multiscale(tta=True)'s over `scales`, per
    tile, or per group with window_batch=K.
    analysis: a PseudoLabelAnalysis.  Every tile's probabilities, as they are written (with save_prob=True: resized to
    `size`), go to analysis.update together with the tile's ground truth ret_gt['cls'] (int, (b, H, W) at the same size),
    while they are still on the device; analysis.summary() afterwards is what analysis_pseudo_labels gives over the
    written files.  None: nothing of this runs."""
    from ..utils.tools import check_window_batch, pre_slide, predict_multiscale, window_groups
    if analysis is not None and not isinstance(analysis, PseudoLabelAnalysis):
        # (the parameter sits before `scales`: a `scales` passed by position must not be taken for it)
        raise TypeError(f'gener_target_pseudo: analysis= takes a PseudoLabelAnalysis, got {type(analysis).__name__}')
    if scales is not None and not slide:
        raise ValueError('gener_target_pseudo: scales= is multi-scale sliding-window inference and needs slide=True')
    model.eval()
    os.makedirs(save_pseudo_label_path, exist_ok=True)
    num_classes = getattr(_cfg, 'NUM_CLASSES', None) or model.num_classes

    def analyse(probs, ret_gt):
        if 'cls' not in ret_gt:
            raise KeyError("gener_target_pseudo(analysis=): the loader's ret_gt must carry the ground truth as ret_gt['cls']")
        analysis.update(probs, torch.as_tensor(ret_gt['cls']).to(probs.device, torch.int64).reshape(probs.shape[0], *probs.shape[-2:]))

    def write(cls, ret_gt):
        if save_prob:
            out = ops.resize_bilinear_ac(cls, size) if tuple(cls.shape[-2:]) != tuple(size) else cls
            if analysis is not None:
                analyse(out, ret_gt)
            torch.save(out.squeeze(dim=0).cpu(), os.path.join(save_pseudo_label_path, ret_gt['fname'][0] + '.pt'))
        else:
            if analysis is not None:
                analyse(cls, ret_gt)
            if _cfg.PSEUDO_SELECT:                # required attribute, as in the reference (:144)
                lab = pseudo_selection(cls, ignore_label=ignore_label)      # the reference's call: default cut-offs, ndarray (:145)
            else:
                lab = ops.argmax_nchw(cls).cpu().numpy()
            from PIL import Image
            arr = (np.asarray(lab) + 1).reshape(*size).astype(np.uint8)      # -1 .. C-1  ->  0 .. C  (:149-150)
            # (a uint8 2-D array is mode 'L' by itself; the `mode=` argument is deprecated in Pillow >= 11.3)
            Image.fromarray(arr).save(os.path.join(save_pseudo_label_path, ret_gt['fname'][0]))

    with torch.no_grad():
        if slide and window_batch is not None:
            check_window_batch(window_batch, tta=True)
            for group in window_groups(pseudo_loader, tta=True, window_batch=window_batch):
                img = torch.cat([ret for ret, _ in group]).cuda()
                if scales is not None:
                    cls = predict_multiscale(model, img, scales, num_classes=num_classes, tta=True, window_batch=window_batch)
                else:
                    cls = pre_slide(model, img, num_classes=num_classes, tta=True, window_batch=window_batch)
                off = 0
                for ret, ret_gt in group:
                    b = ret.shape[0]
                    write(cls[off:off + b], ret_gt)
                    off += b
            return
        for ret, ret_gt in pseudo_loader:
            ret = ret.cuda()
            if scales is not None:
                cls = predict_multiscale(model, ret, scales, num_classes=num_classes, tta=True, window_batch=None)
            else:
                cls = pre_slide(model, ret, num_classes=num_classes, tta=True) if slide else model(ret)
            write(cls, ret_gt)
