"""evaluate -- mirror of regda/utils/eval.py:14-56: eval-mode sliding-window inference over a loader, argmax, confusion
matrix, mIoU with class 0 dropped for IsprsDA.  Datasets / loaders and the colour visualisations are outside the
path: the loader is passed in (`dataloader=`), anything yielding `(image (1,3,H,W), {'cls': (1,H,W)})`."""
import torch

from .. import ops
from ..gast.metrics import PixelMetricIgnore
from .tools import (batched_slide_supported, check_window_batch, multiscale_accumulate, pre_slide, predict_multiscale,
                    slide_accumulate, window_groups)


def evaluate(model, cfg, is_training=False, ckpt_path=None, logger=None, slide=True, tta=False, test=False,
             dataloader=None, class_names=None, window_batch=None, scales=None):
    """window_batch=K (with slide): consecutive items of one shape are grouped until they hold K windows and run
    through the model K windows (x 8 views with tta) at a time; the normalisation, argmax and confusion matrix of a
    group are one launch (rgda_window_finish).  The counts are integers, so the table is the per-item one whenever the
    probabilities are.
    scales (with slide): multi-scale testing -- every item's probabilities are predict_multiscale's over `scales`; with
    window_batch=K the groups above go through multiscale_accumulate and the same single rgda_window_finish."""
    ignore_labels = [0] if getattr(cfg, 'DATASETS', None) == 'IsprsDA' else []
    if dataloader is None:
        raise ValueError('regda_amd.utils.eval.evaluate needs dataloader=: the dataset classes are not part of this build')
    if not is_training:
        model.load_state_dict(torch.load(ckpt_path), strict=True)
        if logger is not None:
            logger.info('[Load params] from {}'.format(ckpt_path))
    num_class = getattr(cfg, 'NUM_CLASSES', None) or model.num_classes
    model.eval()
    names = list(class_names) if class_names is not None else [str(i) for i in range(num_class)]
    metric_op = PixelMetricIgnore(len(names), class_names=names, logdir=getattr(cfg, 'SNAPSHOT_DIR', None), logger=logger,
                                  ignore_labels=ignore_labels)
    if scales is not None:
        if not slide:
            raise ValueError('evaluate: scales= is multi-scale sliding-window inference and needs slide=True')
        with torch.no_grad():
            if window_batch is None:
                for ret, ret_gt in dataloader:
                    cls = predict_multiscale(model, ret.cuda(), scales, num_classes=num_class, tta=tta, window_batch=None)
                    metric_op.forward(ret_gt['cls'].to('cuda', torch.int64), ops.argmax_nchw(cls))
                return metric_op.summary_all()
            check_window_batch(window_batch, tta=tta)
            for group in window_groups(dataloader, tta=tta, window_batch=window_batch):
                img = torch.cat([ret for ret, _ in group]).cuda().contiguous().float()
                acc, cnt = multiscale_accumulate(model, img, num_class, scales, tta=tta, window_batch=window_batch)
                gt = torch.cat([ret_gt['cls'] for _, ret_gt in group]).to('cuda', torch.int64)
                ops.window_finish(acc, cnt, y_true=gt, cm=metric_op._total, flag=metric_op._flag)
        return metric_op.summary_all()
    if slide and window_batch is not None:
        check_window_batch(window_batch, tta=tta)
        with torch.no_grad():
            for group in window_groups(dataloader, tta=tta, window_batch=window_batch):
                img = torch.cat([ret for ret, _ in group]).cuda().contiguous().float()
                if not batched_slide_supported(img.shape, tta=tta):
                    cls = pre_slide(model, img, num_classes=num_class, tta=tta)
                    metric_op.forward(group[0][1]['cls'].to('cuda', torch.int64), ops.argmax_nchw(cls))
                    continue
                full, count = slide_accumulate(model, img, num_class, tta=tta, window_batch=window_batch)
                gt = torch.cat([ret_gt['cls'] for _, ret_gt in group]).to('cuda', torch.int64)
                ops.window_finish(full, count, y_true=gt, cm=metric_op._total, flag=metric_op._flag)
        return metric_op.summary_all()
    with torch.no_grad():
        for ret, ret_gt in dataloader:
            ret = ret.cuda()
            cls = pre_slide(model, ret, num_classes=num_class, tta=tta) if slide else model(ret)
            pred = ops.argmax_nchw(cls)
            metric_op.forward(ret_gt['cls'].to('cuda', torch.int64), pred)      # y_true < 0 is masked in the kernel
    return metric_op.summary_all()
