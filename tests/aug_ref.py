"""CPU restatement of rgda_augment_tiles (include/rgda_hip.h) with torch ops: crop, the dihedral element as flips and
a transpose, then the per-(channel, byte) and per-byte tables.  Used by tests/test_augment_*.py and
tests/golden/make_augment_goldens.py."""
import torch


def apply_d(x, d):
    """x [..., H, W] -> out[..., i, j] = x[..., y, x] with (u, v) = t ? (j, i) : (i, j), y = fr ? H-1-u : u,
    x = fc ? W-1-v : v, d = t | fr << 1 | fc << 2."""
    if d & 2:
        x = x.flip(-2)
    if d & 4:
        x = x.flip(-1)
    if d & 1:
        x = x.transpose(-2, -1)
    return x.contiguous()


def augment(img, params, size, lut, label=None, label_lut=None, soft=None, regs=None):
    """The kernel's outputs for CPU inputs: img uint8 [N][H][W][3], label uint8 [N][H][W], soft f32 [N][C][H][W],
    regs int32 [N][H][W], params int32 [N][4], lut f32 [3][256], label_lut int32 [256]."""
    ho, wo = size
    out = {'image': [], 'label': [], 'soft': [], 'regs': []}
    for n in range(img.shape[0]):
        y0, x0, d = (int(v) for v in params[n, :3])
        win = (slice(y0, y0 + ho), slice(x0, x0 + wo))
        im = apply_d(img[n][win].permute(2, 0, 1), d).long()
        out['image'].append(torch.stack([lut[c][im[c]] for c in range(3)]))
        if label is not None:
            out['label'].append(label_lut[apply_d(label[n][win], d).long()].long())
        if soft is not None:
            out['soft'].append(apply_d(soft[n][(slice(None),) + win], d))
        if regs is not None:
            out['regs'].append(apply_d(regs[n][win], d).long()[None])
    return {k: (torch.stack(v) if v else None) for k, v in out.items()}
