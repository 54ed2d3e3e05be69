"""Region maps without SAM -- the GPU counterpart of regda/gast/superpixels.py and regda/gast/slic/superpixel.py.

NOT pinned: the superpixel algorithm.  The reference's `SuperPixelsLSC` (superpixels.py:49-83) and its SLIC
(slic/superpixel.py:66-90) call third-party generators (cv2.ximgproc, skimage).  `SuperPixelsSLIC` stands in for them
and reproduces neither: it is this project's own integer SLIC (include/rgda_hip.h: rgda_superpixels), bit-exact
against its numpy restatement.  Its maps have the format `Homogenizer` (LRH) and the superpixel view of `label_refine`
read: int32, 0 = "no region" (components below `min_area` are dropped there, never merged into a neighbour), kept
regions numbered 1..R.
PINNED: `edge_shrinking` (superpixels.py:129-152), the reference's own loop, bit-exact (rgda_region_shrink).

No files and no visualisation: reading tiles and saving maps stay with the caller."""
import numpy as np
import torch

from .. import ops


class SuperPixelsSLIC(object):

    def __init__(self, region_size=16, compactness=10, iterate_num=10, min_area=None):
        self.region_size = int(region_size)
        self.compactness = int(compactness)
        self.iterate_num = int(iterate_num)
        self.min_area = self.region_size ** 2 // 4 if min_area is None else int(min_area)
        self._ws = None

    def max_regions(self, H, W):
        """The `max_regions` to give Homogenizer / SSLStep for H x W maps of this generator (ids lie below it)."""
        return ops.superpixels_max_regions(H, W, self.min_area)

    def __call__(self, imgs, out=None):
        """imgs: uint8 [N][H][W][3] on the GPU -> (regs int32 [N][H][W], count int32 [N]), on the current stream."""
        regs, count = ops.superpixels(imgs, self.region_size, self.compactness, self.iterate_num, self.min_area, out=out,
                                      ws=self._ws)
        return regs, count

    def reserve(self, N, H, W, device='cuda'):
        """Allocate the workspace for [N][H][W][3] batches once, so that later calls allocate only their outputs."""
        from .._lib import lib
        need = lib().size('rgda_superpixels_workspace', N, H, W, self.region_size)
        if need and (self._ws is None or self._ws.numel() < need):
            self._ws = torch.empty(need, dtype=torch.uint8, device=device)
        return self

    def get_super_pixels(self, img):
        """img: one (H, W, 3) uint8 array or tensor -> (number_supixl, label_supixl) as the reference's
        get_super_pixels returns them (without its visualisation): the region count and the (H, W) int32 map -- a
        numpy array for an array, a GPU tensor for a tensor."""
        as_numpy = not torch.is_tensor(img)
        t = torch.from_numpy(np.ascontiguousarray(img)) if as_numpy else img
        regs, count = self(t.cuda()[None])
        number = int(count.item())
        return number, (regs[0].cpu().numpy() if as_numpy else regs[0])


def edge_shrinking(label_supixl, win_size=3, region_size=16, fill=None):
    """The reference's edge_shrinking without its file output: ids whose (2 * win_size + 1)^2 window holds another id
    become `fill`.  fill=None gives the reference's cnt_sup = int(h / region_size * w / region_size); 0 ("no region") is
    the useful value in front of LRH.  label_supixl: (H, W) or (N, H, W), int32 array or tensor -> the same kind."""
    as_numpy = not torch.is_tensor(label_supixl)
    t = torch.from_numpy(np.ascontiguousarray(label_supixl)) if as_numpy else label_supixl
    h, w = t.shape[-2:]
    if fill is None:
        fill = int(h / region_size * w / region_size)
    out = ops.region_shrink(t.to(torch.int32).cuda(), win_size, fill)
    return out.cpu().numpy() if as_numpy else out
