"""loss_calc / learning-rate schedule / config import / sliding-window + TTA + multi-scale inference / IAST
self-training (adaptive pseudo-labels, entropy and KLD regularisers) -- mirror of
regda/utils/tools.py:51-97,108-129,132-152,173-207,240-260,323-398."""
import importlib
import os
import shutil
from math import ceil

import numpy as np
import torch
import torch.nn.functional as tnf

from .. import ops


def import_config(config_name, prefix='configs', copy=True, create=True, postfix=''):
    """Load the UPPER_CASE config module `<prefix>.<config_name>` (e.g. 'st.regda.2potsdam'), append `postfix` to its
    SNAPSHOT_DIR, optionally create that directory and drop a copy of the module there as config.py
    (same contract as tools.py:173-181)."""
    module = importlib.import_module(f'{prefix}.{config_name}')
    module.SNAPSHOT_DIR = module.SNAPSHOT_DIR + postfix
    if create:
        os.makedirs(module.SNAPSHOT_DIR, exist_ok=True)
    if copy:
        shutil.copy(os.path.abspath(module.__file__), os.path.join(module.SNAPSHOT_DIR, 'config.py'))
    return module


def learning_rate_at(i_iter, base_lr, warmup_iter, max_iter, power):
    """The one schedule of the st.regda.* runs (tools.py:184-207): linear warm-up from 0 over `warmup_iter`
    iterations, then polynomial decay base * (1 - it / max_iter) ** power.  Plain Python floats, like the reference."""
    it = float(i_iter)
    if i_iter < warmup_iter:
        return base_lr * (it / warmup_iter)
    return base_lr * (1 - it / max_iter) ** power


def lr_poly(base_lr, i_iter, max_iter, power):
    """Decay branch alone (tools.py:184-185)."""
    return learning_rate_at(i_iter, base_lr, 0, max_iter, power)


def lr_warmup(base_lr, i_iter, warmup_iter):
    """Warm-up branch alone (tools.py:188-189); not clamped past `warmup_iter`, like the reference."""
    return base_lr * (float(i_iter) / warmup_iter)


def adjust_learning_rate(optimizer, i_iter, cfg):
    """Set the lr of `optimizer` for iteration `i_iter` from cfg.{LEARNING_RATE, PREHEAT_STEPS, NUM_STEPS, POWER};
    a second parameter group, when present, runs at ten times the rate (tools.py:191-207).  Returns the lr."""
    lr = learning_rate_at(i_iter, cfg.LEARNING_RATE, cfg.PREHEAT_STEPS, cfg.NUM_STEPS, cfg.POWER)
    for group, mult in zip(optimizer.param_groups[:2], (1, 10)):
        group['lr'] = lr * mult
    return lr


def loss_calc(pred, label, loss_fn, multi=False):
    """Cross entropy for segmentation (tools.py:240-260).  With the fused CrossEntropy of
    regda_amd.gast.balance the upsample and both heads run in one kernel."""
    if multi is True:
        if hasattr(loss_fn, 'forward_multi') and len(pred) == 2:
            return loss_fn.forward_multi(pred, label.long())
        loss, num = 0, 0
        for p in pred:
            if p.size()[-2:] != label.size()[-2:] and not hasattr(loss_fn, 'forward_multi'):
                p = tnf.interpolate(p, size=label.size()[-2:], mode='bilinear', align_corners=True)
            loss += loss_fn(p, label.long())
            num += 1
        return loss / num
    if pred.size()[-2:] != label.size()[-2:] and not hasattr(loss_fn, 'forward_multi'):
        pred = tnf.interpolate(pred, size=label.size()[-2:], mode='bilinear', align_corners=True)
    return loss_fn(pred, label.long())


# ----------------------------------------------------------------------------- teacher inference
def pad_image(img, target_size):
    """"Pad an image up to the target size" -- literally what tools.py:51-58 computes:
    `tnf.pad(img, (0, 0, rows_missing, cols_missing))`, i.e. the ROW dimension gets rows_missing zeros on top and
    cols_missing at the bottom (negative = crop) and the width is untouched.  A no-op for windows that already have
    the tile size, which is every case where the image is at least as large as the tile."""
    rows_missing = target_size[0] - img.shape[2]
    cols_missing = target_size[1] - img.shape[3]
    if rows_missing == 0 and cols_missing == 0:
        return img
    return ops.pad_rows(img.contiguous().float(), rows_missing, cols_missing)


def tta_predict(model, img):
    """8-view test-time augmentation (tools.py:132-152; ttach 0.0.3 Compose([HorizontalFlip(), Rotate90(0/90/180/
    270)]), merge = mean).  The reference runs eight batch-1 forwards; the views are independent and the model is in
    eval mode (running BatchNorm statistics, per-sample InstanceNorm and pooling), so they go through the network
    as ONE batch of eight -- same arithmetic per view, one eighth of the launches.  Square tiles only when batched
    (rot90 of a non-square tile changes its shape): other shapes fall back to one forward per view."""
    if img.shape[0] != 1:
        raise ValueError('tta_predict averages over dim 0 like the reference: batch size must be 1')
    img = img.contiguous().float()
    views = [(f, k) for f in (False, True) for k in (0, 1, 2, 3)]
    _, c, h, w = img.shape
    out = None
    if h == w:
        batch = torch.empty(len(views), c, h, w, device=img.device)
        for i, (f, k) in enumerate(views):
            ops.dihedral(img, f, k, True, dst=batch[i:i + 1])
        pred = model(batch)
        for i, (f, k) in enumerate(views):
            out = ops.dihedral(pred[i:i + 1].contiguous(), f, (4 - k) % 4, False, dst=out, scale=1.0 / len(views),
                               accumulate=out is not None)
        return out
    for f, k in views:
        pred = model(ops.dihedral(img, f, k, True))
        out = ops.dihedral(pred.contiguous(), f, (4 - k) % 4, False, dst=out, scale=1.0 / len(views),
                           accumulate=out is not None)
    return out


def window_list(H, W, tile_size=(512, 512)):
    """The windows pre_slide visits on an H x W image, in its order: a list of (y1, x1, h, w) -- exactly the arithmetic
    of tools.py:61-97 (stride ceil(tile[0] / 2) on both axes; edge windows shifted back inside the image; none at all
    when the image is much smaller than the tile)."""
    stride = ceil(tile_size[0] * (1 - 1 / 2))
    tile_rows = int(ceil((H - tile_size[0]) / stride) + 1)
    tile_cols = int(ceil((W - tile_size[1]) / stride) + 1)
    out = []
    for row in range(tile_rows):
        for col in range(tile_cols):
            x1, y1 = int(col * stride), int(row * stride)
            x2, y2 = min(x1 + tile_size[1], W), min(y1 + tile_size[0], H)
            x1, y1 = max(int(x2 - tile_size[1]), 0), max(int(y2 - tile_size[0]), 0)
            out.append((y1, x1, y2 - y1, x2 - x1))
    return out


# one forward of the batched route stays below 2^27 input pixels: the widest activations (the stem's and layer 1's
# outputs, the upsampled probabilities) hold at most 16 values per input pixel, so their offsets stay below 2^31
MAX_WINDOW_PIXELS = 1 << 27


def batched_slide_supported(shape, tile_size=(512, 512), tta=False):
    """True where pre_slide(window_batch=K) runs the batched route for an image batch of `shape` (n, c, H, W) or (H, W):
    the image is at least the tile in both dimensions (so every window is a whole tile) and, with TTA, the tile is
    square (rot90 keeps its shape).  Otherwise pre_slide takes the per-window path."""
    H, W = shape[-2:]
    th, tw = tile_size
    return H >= th and W >= tw and (not tta or th == tw)


def check_window_batch(window_batch, tile_size=(512, 512), tta=False):
    k = int(window_batch)
    if k != window_batch or k < 1:
        raise ValueError('window_batch must be a positive int, got %r' % (window_batch,))
    if k * (8 if tta else 1) * tile_size[0] * tile_size[1] > MAX_WINDOW_PIXELS:
        raise ValueError('window_batch=%d: %d windows x %d views of %dx%d pixels per forward exceed %d pixels' %
                         (k, k, 8 if tta else 1, tile_size[0], tile_size[1], MAX_WINDOW_PIXELS))
    return k


def slide_accumulate(model, image, num_classes, tile_size=(512, 512), tta=False, window_batch=16, lut=None,
                     scaled_size=None):
    """The batched window loop without the final division: -> (full (n, C, H, W), count (n, 1, H, W)) as pre_slide holds
    them before rgda_window_normalise.  image: f32 (n, c, H, W), or uint8 (n, H, W, 3) with `lut` (f32 [3][256] device
    table), on the GPU; batched_slide_supported must hold.  Windows are taken image by image in pre_slide's order,
    `window_batch` of them (x 8 views with tta) per forward.
    scaled_size=(Hs, Ws): the same loop over ops.resize_bilinear_ac(normalised image, (Hs, Ws)), which is never stored
    (rgda_window_gather_scaled makes each window from the source); full and count are then Hs x Ws."""
    K = check_window_batch(window_batch, tile_size, tta)
    if image.dtype == torch.uint8:
        n, H, W, _ = image.shape
    else:
        n, _, H, W = image.shape
    if scaled_size is not None:
        H, W = scaled_size
    th, tw = tile_size
    assert batched_slide_supported((H, W), tile_size, tta)
    views = 8 if tta else 1
    rows = [(i, y1, x1) for i in range(n) for (y1, x1, _, _) in window_list(H, W, tile_size)]
    table = torch.tensor(rows, dtype=torch.int32).to(image.device, non_blocking=True)
    full = torch.zeros(n, num_classes, H, W, device=image.device)
    count = torch.zeros(n, 1, H, W, device=image.device)
    for s in range(0, len(rows), K):
        chunk = rows[s:s + K]
        wins = table[s:s + len(chunk)]
        if scaled_size is None:
            batch = ops.window_gather(image, wins, tile_size, views, lut=lut)
        else:
            batch = ops.window_gather_scaled(image, wins, tile_size, scaled_size, views, lut=lut)
        pred = model(batch)
        r0 = min(i * H + y1 for i, y1, _ in chunk)
        r1 = max(i * H + y1 + th for i, y1, _ in chunk)
        ops.window_scatter(pred.contiguous(), wins, full, count, (r0, r1 - r0), views)
    return full, count


def pre_slide(model, image, num_classes=7, tile_size=(512, 512), tta=False, window_batch=None):
    """Sliding-window inference with overlap 1/2 (tools.py:61-97); returns the visit-count average (n, C, H, W).
    window_batch=K: the windows of all n images go through the model K at a time (K x 8 views with tta), gathered and
    scattered by one launch each (rgda_window_gather / _scatter); every value is placed and summed as the per-window
    loop places and sums it.  Images smaller than the tile (and non-square tiles with tta) take the per-window path."""
    image = image.contiguous().float()
    if window_batch is not None:
        check_window_batch(window_batch, tile_size, tta)
        if batched_slide_supported(image.shape, tile_size, tta):
            full, count = slide_accumulate(model, image, num_classes, tile_size, tta, window_batch)
            ops.window_finish(full, count)
            return full
    n, c, H, W = image.shape
    full_probs = torch.zeros(n, num_classes, H, W, device=image.device)
    count = torch.zeros(n, 1, H, W, device=image.device)
    for y1, x1, h, w in window_list(H, W, tile_size):
        img = image if (h, w) == (H, W) else ops.window_crop(image, y1, x1, h, w, h, w)
        padded_img = pad_image(img, tile_size)
        padded = tta_predict(model, padded_img) if tta else model(padded_img)
        ops.window_accumulate(padded.contiguous(), full_probs, count, y1, x1, h, w)
    ops.window_normalise(full_probs, count)
    return full_probs


# ----------------------------------------------------------------------------- multi-scale testing (tools.py:108-129)
DEFAULT_SCALES = (0.75, 1.0, 1.25, 1.5, 1.75, 2.0)


def scaled_size(H, W, s):
    """The size ndimage.zoom(image, (1, 1, s, s)) gives an H x W image (tools.py:122): Python's round of H * s, W * s."""
    return int(round(H * s)), int(round(W * s))


def check_scales(H, W, scales):
    """-> [(Hs, Ws)] of `scales` for an H x W image; ValueError for no scale, a scale that is not a positive finite number
    and a scale whose image has no pixels."""
    scales = [float(s) for s in scales]
    if not scales:
        raise ValueError('multi-scale inference needs at least one scale')
    sizes = []
    for s in scales:
        if not (0 < s < float('inf')):
            raise ValueError('scales must be positive, got %r' % (s,))
        hs, ws = scaled_size(H, W, s)
        if hs < 1 or ws < 1:
            raise ValueError('scale %r of a %dx%d image has no pixels' % (s, H, W))
        sizes.append((hs, ws))
    return sizes


def multiscale_accumulate(model, image, num_classes, scales, tile_size=(512, 512), tta=False, window_batch=16, lut=None):
    """The sum over `scales` of the sliding-window probabilities of the rescaled image, each brought back to H x W:
    -> (acc (n, C, H, W), cnt (n, 1, H, W) = len(scales)); ops.window_finish(acc, cnt) is the mean.  image as for
    slide_accumulate (f32 NCHW, or uint8 NHWC with `lut`).  Per scale, in the given order, the windows of the Hs x Ws
    image go through the model exactly as slide_accumulate would take them from it (rgda_window_gather_scaled builds them
    from the source), and rgda_scale_merge divides by the visit count, resizes back and adds in one pass; the scale's
    n * (C + 1) * Hs * Ws * 4 bytes are released before the next scale.  A scaled image smaller than the tile (or a
    non-square tile with tta) is materialised and takes pre_slide's per-window path."""
    check_window_batch(window_batch, tile_size, tta)
    if image.dtype == torch.uint8:
        n, H, W, _ = image.shape
    else:
        n, _, H, W = image.shape
    sizes = check_scales(H, W, scales)
    acc = torch.zeros(n, num_classes, H, W, device=image.device)
    cnt = torch.zeros(n, 1, H, W, device=image.device)
    x = None
    for size in sizes:
        if batched_slide_supported(size, tile_size, tta):
            full_s, count_s = slide_accumulate(model, image, num_classes, tile_size, tta, window_batch, lut=lut,
                                               scaled_size=size)
            ops.scale_merge(full_s, count_s, acc, cnt)
            del full_s, count_s
            continue
        if x is None:
            x = image
            if image.dtype == torch.uint8:      # the normalised image through the identity element of rgda_augment_tiles
                x = ops.augment_tiles(image, torch.zeros(n, 4, dtype=torch.int32), lut, (H, W))['image']
        xs = ops.resize_bilinear_ac(x, size)
        if tta and n > 1:                       # tta_predict takes one image
            probs = torch.cat([pre_slide(model, xs[i:i + 1], num_classes, tile_size, True) for i in range(n)])
        else:
            probs = pre_slide(model, xs, num_classes, tile_size, tta)
        acc += ops.resize_bilinear_ac(probs, (H, W))
        cnt += 1
    return acc, cnt


def predict_multiscale(model, image, scales=DEFAULT_SCALES, tile_size=(512, 512), num_classes=None, tta=False,
                       window_batch=16):
    """Multi-scale testing (tools.py:108-129): the mean over `scales` of the class probabilities of the image resampled
    by each scale, brought back to the image's size; (n, C, H, W).  Kept from the reference: the default scales, the
    resampling of the image (ndimage.zoom(order=1, prefilter=False), which is align_corners=True bilinear to
    scaled_size(H, W, s)), the align_corners=True resize of the probabilities and the mean.
    The reference's function cannot run: it adds the (1, C, H, W) prediction in place into a (1, 1, H, W) accumulator,
    which raises for C > 1.  Beyond mending that, this one differs in three ways: the image is resampled on the GPU, not by
    scipy on the host; each scaled image goes through pre_slide's windows of `tile_size` (with `tta` through the 8 views)
    instead of one whole-image forward, which a scene does not fit; and the probabilities come back to the image's size,
    where the reference resizes them to `tile_size`.  The division by len(scales) is IEEE (rgda_window_finish).
    num_classes: model.num_classes when None.  window_batch=K: K windows per forward (multiscale_accumulate);
    None: the composition resize_bilinear_ac -> pre_slide -> resize_bilinear_ac per scale."""
    n, _, H, W = image.shape
    scales = tuple(scales)
    sizes = check_scales(H, W, scales)
    if num_classes is None:
        num_classes = model.num_classes
    image = image.contiguous().float()
    if window_batch is not None:
        acc, cnt = multiscale_accumulate(model, image, num_classes, scales, tile_size, tta, window_batch)
        ops.window_finish(acc, cnt)
        return acc
    acc = torch.zeros(n, num_classes, H, W, device=image.device)
    for size in sizes:
        probs = pre_slide(model, ops.resize_bilinear_ac(image, size), num_classes, tile_size, tta)
        acc += ops.resize_bilinear_ac(probs, (H, W))
    ops.window_normalise(acc, torch.full((n, 1, H, W), float(len(sizes)), device=image.device))
    return acc


def window_groups(loader, tile_size=(512, 512), tta=False, window_batch=16):
    """Consecutive loader items (image (b, c, H, W), meta) in groups for the batched route: items of one shape are
    collected until they hold at least `window_batch` windows (the last group of a shape may hold fewer).  An item the
    batched route does not serve (batched_slide_supported) comes as a group of its own.  Yields lists of items, in
    loader order."""
    group, shape, nwin = [], None, 0
    for item in loader:
        shp = tuple(item[0].shape)
        if group and shp != shape:
            yield group
            group, nwin = [], 0
        if not batched_slide_supported(shp, tile_size, tta):
            yield [item]
            continue
        group.append(item)
        shape = shp
        nwin += shp[0] * len(window_list(shp[2], shp[3], tile_size))
        if nwin >= window_batch:
            yield group
            group, nwin = [], 0
    if group:
        yield group


# ----------------------------------------------------------------------------- IAST self-training (tools.py:323-398)
class _RegLoss(torch.autograd.Function):
    """One of IAST's region regularisers on full-resolution logits: rgda_upsample_reg with h == H, w == W, one head, the
    caller's weight map and the reference's 0 / 0 = NaN for an empty region."""

    @staticmethod
    def forward(ctx, logits, weight, term):
        x = logits.detach()
        want = ctx.needs_input_grad[0]
        kw = dict(w_ent=weight) if term == ops.REG_ENT else dict(w_kld=weight)
        loss, g1, g2 = ops.upsample_reg(x, x, terms=term, size=x.shape[-2:], want_grad=want, heads=1, **kw)
        ctx.grad = g1.add_(g2).to(logits.dtype) if want else None
        return loss[0 if term == ops.REG_ENT else 1].clone()

    @staticmethod
    def backward(ctx, grad_out):
        return grad_out * ctx.grad, None, None


def _reg_weight(weight, who):
    if weight is None:          # the reference indexes it: TypeError there too
        raise TypeError(f'{who}: weight is required (N x 1 x H x W)')
    return weight.detach()


def entropyloss(logits, weight=None):
    """sum(-softmax * weight * log_softmax) / #(weight > 0) (tools.py:376-385).  logits N x C x H x W on the GPU, weight
    N x 1 x H x W (or N x H x W).  Differentiable in the logits."""
    return _RegLoss.apply(logits, _reg_weight(weight, 'entropyloss'), ops.REG_ENT)


def kldloss(logits, weight):
    """sum(-1 / C * weight * log_softmax) / #(weight > 0) (tools.py:388-398); arguments as entropyloss."""
    return _RegLoss.apply(logits, _reg_weight(weight, 'kldloss'), ops.REG_KLD)


class IASTSelector:
    """The instance-adaptive selector of generate_pseudo's loop (tools.py:342-370 with ias_thresh, :323-332): per-class
    thresholds `cls_thresh` (host float64, 0.9 at the start) that move, batch by batch, towards a percentile of the
    class's confidences.  update() runs rgda_iast_hist / _percentile / _label; the C percentiles come back to the host
    (the one sync per batch), where the EMA and the exponent are numpy's own arithmetic."""

    def __init__(self, n_class=7, pl_alpha=0.2, pl_beta=0.9, pl_gamma=8.0):
        ops.check_class_count(n_class, 'IASTSelector')
        self.n_class, self.alpha, self.beta, self.gamma = n_class, pl_alpha, pl_beta, pl_gamma
        self.cls_thresh = np.ones(n_class) * 0.9

    # training state (regda_amd/checkpoint.py): the thresholds, as the float64 they are
    def state_dict(self):
        return {'cls_thresh': torch.from_numpy(np.array(self.cls_thresh, dtype=np.float64))}

    def load_state_dict(self, sd, strict=True):
        if not isinstance(sd, dict) or 'cls_thresh' not in sd:
            raise ValueError("state entry 'IASTSelector.cls_thresh' is missing")
        t = sd['cls_thresh']
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float64 or tuple(t.shape) != (self.n_class,):
            raise ValueError(f"state entry 'IASTSelector.cls_thresh': expected a float64 tensor of {self.n_class} thresholds")
        self.cls_thresh = t.detach().cpu().numpy().copy()

    def quantiles(self):
        """q_c of np.percentile(arr, 100 * (1 - alpha * w_c ** gamma)), scalar by scalar as ias_thresh computes them."""
        w = self.cls_thresh
        q = np.array([np.true_divide(100 * (1 - self.alpha * w[c] ** self.gamma), 100) for c in range(self.n_class)],
                     dtype=np.float64)
        if not np.all((q >= 0) & (q <= 1)):
            raise ValueError('Percentiles must be in the range [0, 100]')
        return q

    def update(self, probs):
        """probs f32 (n, n_class, H, W) in [0, 1] on the GPU -> labels uint8 (n, H, W) on the GPU: argmax + 1, 0 where the
        confidence is below its class's updated threshold."""
        n, c, H, W = probs.shape
        if c != self.n_class:
            raise ValueError(f'IASTSelector: {c} channels for {self.n_class} classes')
        ws = ops.iast_hist(probs.float())
        tq = torch.from_numpy(np.stack([self.cls_thresh, self.quantiles()])).to(probs.device)
        tmp = ops.iast_percentile(ws, tq[0], tq[1]).cpu().numpy()
        # the moving average: the candidate's share in float32 (tmp's type), the sum in float64; a threshold that reaches
        # 1 would select nothing and restarts at 0.999
        moved = self.beta * self.cls_thresh + (1 - self.beta) * tmp
        self.cls_thresh = np.where(moved >= 1, 0.999, moved)
        return ops.iast_label(ws, torch.from_numpy(self.cls_thresh).to(probs.device), n, H, W)


def _default_writer():
    try:
        from skimage.io import imsave
        return imsave
    except ImportError:
        from PIL import Image
        return lambda path, arr: Image.fromarray(arr).save(path)


def generate_pseudo(model, target_loader, save_dir, n_class=7, pseudo_dict=None, logger=None, writer=None):
    """IAST pseudo-label generation (tools.py:335-373): every batch of `target_loader` ((image, {'fname': [...]}))
    goes through `model` in eval mode and an IASTSelector(pseudo_dict['pl_alpha' / 'pl_beta' / 'pl_gamma']); the uint8
    labels are written with `writer(path, array)` (skimage's imsave, else PIL) to save_dir/pred/<fname>.  Returns that
    directory.  The reference's palette visualisation (er.viz) is not provided."""
    if pseudo_dict is None:
        pseudo_dict = dict()
    if logger is not None:
        logger.info('Start generate pseudo labels: %s' % save_dir)
    pred_dir = os.path.join(save_dir, 'pred')
    os.makedirs(pred_dir, exist_ok=True)
    if writer is None:
        writer = _default_writer()
    model.eval()
    selector = IASTSelector(n_class, pseudo_dict['pl_alpha'], pseudo_dict['pl_beta'], pseudo_dict['pl_gamma'])
    for image, labels in target_loader:
        with torch.no_grad():
            out = model(image.cuda())
        probs = out[0] if isinstance(out, tuple) else out
        label = selector.update(probs).cpu().numpy()
        for i, fname in enumerate(labels['fname']):
            writer(os.path.join(pred_dir, fname), label[i])
    return pred_dir
