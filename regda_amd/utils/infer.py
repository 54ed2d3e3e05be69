"""Whole-scene prediction -- the library counterpart of tools/infer_single.py: one orthophoto, as imread returns it
(uint8 H x W x 3), in one call.  The scene stays uint8 on the device: the windows are normalised as they are gathered
(rgda_window_gather through the test config's Normalize table), so no fp32 copy of the scene is ever made."""
import numpy as np
import torch

from .. import aug, ops
from .tools import (batched_slide_supported, check_scales, multiscale_accumulate, pre_slide, predict_multiscale,
                    slide_accumulate)


def scene_table(cfg):
    """f32 [3][256]: the normalisation of `cfg.TEST_DATA_CONFIG` (EVAL_DATA_CONFIG where a config has no test loader)
    as a per-(channel, byte) table -- what `aug.from_config(...)(img)['image']` applies."""
    data = getattr(cfg, 'TEST_DATA_CONFIG', None) or getattr(cfg, 'EVAL_DATA_CONFIG')
    return aug.from_config(data).table()


def predict_scene(model, image_u8, cfg, num_classes, tile_size=(512, 512), tta=False, window_batch=16,
                  return_probs=False, scales=None):
    """argmax(pre_slide(model, normalise(image), num_classes, tile_size, tta)) of one scene as a uint8 (H, W) label map
    on the GPU (`.cpu().numpy()` is the array infer_single.py saves as prediction.png).  image_u8: uint8 (H, W, 3) numpy
    array or tensor, on the host or the device.  Sets model.eval() as the reference does.  window_batch: windows per
    forward (x 8 views with tta); None runs the per-window path on a normalised fp32 copy.  A scene smaller than the
    tile (or a non-square tile with tta) takes the per-window path too.  return_probs: also return the (1, C, H, W)
    probabilities.  scales: multi-scale testing -- the argmax of predict_multiscale(model, normalise(image), scales, ...);
    the windows of every scale are made from the uint8 scene (rgda_window_gather_scaled), so neither a normalised nor a
    rescaled copy of it is stored."""
    img = torch.as_tensor(np.ascontiguousarray(image_u8) if isinstance(image_u8, np.ndarray) else image_u8)
    if img.dtype != torch.uint8 or img.dim() != 3 or img.shape[2] != 3:
        raise ValueError('predict_scene: the scene must be uint8 (H, W, 3), got %s %s' % (img.dtype, tuple(img.shape)))
    dev = torch.device('cuda', torch.cuda.current_device())
    img = img.to(dev).contiguous()[None]
    H, W = img.shape[1], img.shape[2]
    if scales is not None:
        scales = tuple(scales)
        check_scales(H, W, scales)
    lut = scene_table(cfg).to(dev)
    model.eval()
    with torch.no_grad():
        if scales is not None and window_batch is not None:
            full, count = multiscale_accumulate(model, img, num_classes, scales, tile_size, tta, window_batch, lut=lut)
            labels = torch.empty(1, H, W, dtype=torch.uint8, device=dev)
            ops.window_finish(full, count, labels=labels)
        elif scales is not None:
            x = ops.augment_tiles(img, torch.zeros(1, 4, dtype=torch.int32), lut, (H, W))['image']
            full = predict_multiscale(model, x, scales, tile_size, num_classes, tta, window_batch=None)
            labels = ops.argmax_nchw(full).to(torch.uint8)
        elif window_batch is not None and batched_slide_supported((H, W), tile_size, tta):
            full, count = slide_accumulate(model, img, num_classes, tile_size, tta, window_batch, lut=lut)
            labels = torch.empty(1, H, W, dtype=torch.uint8, device=dev)
            ops.window_finish(full, count, labels=labels)
        else:
            # the normalised scene through the identity element of rgda_augment_tiles, then the per-window path
            x = ops.augment_tiles(img, torch.zeros(1, 4, dtype=torch.int32), lut, (H, W))['image']
            full = pre_slide(model, x, num_classes=num_classes, tile_size=tile_size, tta=tta)
            labels = ops.argmax_nchw(full).to(torch.uint8)
    return (labels[0], full) if return_probs else labels[0]
