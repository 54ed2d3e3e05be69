"""Transforms of the input tiles: crop + dihedral and affine augmentation of raw uint8 tiles
(csrc/augment_kernels.hip), colour jitter and Gaussian blur of the student's tile (csrc/strong_kernels.hip),
Fourier style transfer of the source tile (csrc/fourier_kernels.hip); the last two are small and grouped here."""
import torch

from .._lib import lib
from .base import _H, _need_cuda, _out_like, _p, _stream, _table_check, _write_host_table, _ws, _ws_or


def check_augment_params(params, hi, wi, ho, wo):
    """Host-side check of a CPU int32 [N][4] (y0, x0, d, 0) table: the crop lies inside the hi x wi input, d in 0..7,
    and a transposing (odd) d only for a square output.  Raises ValueError."""
    p = params.numpy()
    if p.ndim != 2 or p.shape[1] != 4:
        raise ValueError('augment params must be [N][4], got %s' % (tuple(p.shape),))
    y0, x0, d = p[:, 0], p[:, 1], p[:, 2]
    if (y0 < 0).any() or (x0 < 0).any() or (y0 > hi - ho).any() or (x0 > wi - wo).any():
        raise ValueError('augment crop outside the %d x %d input' % (hi, wi))
    if (d < 0).any() or (d > 7).any() or ((d & 1).astype(bool) & (ho != wo)).any():
        raise ValueError('augment element d outside 0..7, or odd d with a non-square %d x %d output' % (ho, wo))


def augment_tiles(img, params, lut, size, label=None, label_lut=None, soft=None, regs=None, out=None, flag=None):
    """rgda_augment_tiles: crop + dihedral element + normalisation / label tables of N raw tiles, one launch.
    img uint8 [N][Hi][Wi][3]; label uint8 [N][Hi][Wi]; soft f32 [N][C][Hi][Wi]; regs int32 [N][Hi][Wi] (each optional but
    img, on the GPU); params int32 [N][4] (y0, x0, d, 0): a CPU tensor is checked (check_augment_params) and copied on
    the current stream, a device tensor is used as it is; lut f32 [3][256], label_lut int32 [256] device tables;
    size = (Ho, Wo).  out: {'image', 'label', 'soft', 'regs'} device tensors to write into (allocated where missing).
    flag: optional device int32 tensor, set to 1 by a sample whose device-side params are invalid.
    -> {'image': f32 [N][3][Ho][Wo], 'label': int64 [N][Ho][Wo], 'soft': f32 [N][C][Ho][Wo], 'regs': int64 [N][1][Ho][Wo]}
    (None where the input is None)."""
    return _augment('augment_tiles', check_augment_params, 4, img, params, lut, size, label, label_lut, soft, regs, out, flag)


def _augment(who, check_params, width, img, params, lut, size, label, label_lut, soft, regs, out, flag, *ignore_label):
    """The body of augment_tiles and augment_affine (rgda_<who>): check_params(params, hi, wi, ho, wo) checks a CPU table
    of `width` columns; ignore_label: the affine call's extra argument, behind label_lut."""
    _need_cuda(img, label, soft, regs, lut, label_lut)
    n, hi, wi, three = img.shape
    ho, wo = size
    if three != 3 or img.dtype != torch.uint8:
        raise ValueError('%s: img must be uint8 [N][H][W][3]' % who)
    want = dict(label=(label, torch.uint8, (n, hi, wi)), regs=(regs, torch.int32, (n, hi, wi)),
                soft=(soft, torch.float32, (n, soft.shape[1] if soft is not None else 0, hi, wi)))
    for k, (t, dt, shape) in want.items():
        if t is not None and (t.dtype != dt or tuple(t.shape) != shape):
            raise ValueError('%s: %s must be %s %s, got %s %s' % (who, k, dt, shape, t.dtype, tuple(t.shape)))
    if label is not None and label_lut is None:
        raise ValueError('%s: a label needs label_lut' % who)
    if not params.is_cuda:
        check_params(params, hi, wi, ho, wo)
        params = params.to(img.device, torch.int32, non_blocking=True)
    assert params.dtype == torch.int32 and tuple(params.shape) == (n, width)
    c = soft.shape[1] if soft is not None else 0
    shapes = dict(image=((n, 3, ho, wo), torch.float32, img), label=((n, ho, wo), torch.int64, label),
                  soft=((n, c, ho, wo), torch.float32, soft), regs=((n, 1, ho, wo), torch.int64, regs))
    res = {}
    for k, (shape, dt, src) in shapes.items():
        t = None if out is None else out.get(k)
        if src is None:
            res[k] = None
            continue
        if t is None:
            t = torch.empty(shape, dtype=dt, device=img.device)
        assert tuple(t.shape) == shape and t.dtype == dt and t.is_contiguous(), k
        res[k] = t
    ptr = lambda t: None if t is None else t.contiguous().data_ptr()
    lib().call('rgda_' + who, ptr(img), ptr(label), ptr(soft), ptr(regs), ptr(params), n, hi, wi, c, ho, wo,
               ptr(lut), ptr(label_lut), *ignore_label, ptr(res['image']), ptr(res['label']), ptr(res['soft']),
               ptr(res['regs']), ptr(flag), _stream())
    return res


AFFINE_A_MAX = 131072           # |a_kl| <= 4 * 32768: rgda_augment_affine takes scales inside [1/4, 4]


def check_affine_params(params, hi, wi):
    """Host-side check of a CPU int32 [N][8] (cy, cx, a00, a01, a10, a11, fill, 0) table, the device-side row check of
    rgda_augment_affine: |a_kl| <= 131072, the centre inside [0, hi * 65536] x [0, wi * 65536], fill below 2^24 and
    column 7 zero.  Raises ValueError."""
    p = params.numpy()
    if p.ndim != 2 or p.shape[1] != 8:
        raise ValueError('affine params must be [N][8], got %s' % (tuple(p.shape),))
    if (abs(p[:, 2:6].astype('int64')) > AFFINE_A_MAX).any():
        raise ValueError('affine matrix entry outside +-%d (a scale outside [1/4, 4])' % AFFINE_A_MAX)
    if (p[:, 0] < 0).any() or (p[:, 0] > hi * 65536).any() or (p[:, 1] < 0).any() or (p[:, 1] > wi * 65536).any():
        raise ValueError('affine crop centre outside the %d x %d input' % (hi, wi))
    if (p[:, 6] < 0).any() or (p[:, 6] >> 24).any() or (p[:, 7] != 0).any():
        raise ValueError('affine fill must be r | g << 8 | b << 16 and column 7 zero')


def augment_affine(img, params, lut, size, label=None, label_lut=None, ignore_label=-1, soft=None, regs=None, out=None,
                   flag=None):
    """rgda_augment_affine: one affine warp per sample (random scale / rotation) + normalisation / label tables of N raw
    tiles, one launch.  Arguments as augment_tiles, except params int32 [N][8] (cy, cx, a00, a01, a10, a11, fill, 0) (a
    CPU tensor is checked by check_affine_params), up to 16 soft planes, a size that may exceed the input, and
    ignore_label: the label of a pixel whose source lies outside the input (its regions are 0, its soft label all 0,
    its image the fill colour).
    -> {'image': f32 [N][3][Ho][Wo], 'label': int64 [N][Ho][Wo], 'soft': f32 [N][C][Ho][Wo], 'regs': int64 [N][1][Ho][Wo]}
    (None where the input is None)."""
    return _augment('augment_affine', lambda p, hi, wi, ho, wo: check_affine_params(p, hi, wi), 8, img, params, lut, size,
                    label, label_lut, soft, regs, out, flag, int(ignore_label))


STRONG_TABLE_COLS = _H['RGDA_STRONG_TABLE_COLS']        # {fb, fc, fs, theta, sigma, flags, 0, 0} per image
STRONG_MAX_RADIUS = _H['RGDA_STRONG_MAX_RADIUS']        # sigma <= 4


def strong_write_table(table, host, size):
    """rgda_strong_write_table: table (f32 (N, 8) on the device, N <= 16) <- host (a float32 numpy array of that shape:
    fb, fc, fs, theta, sigma, flags, 0, 0 per image -- StrongAugment.draw), carried in the launch's arguments: the host
    buffer is read before this returns.  size = (H, W) of the tiles the table is for.  A row the transform does not serve
    (sigma outside (0, 4] with the blur bit, a radius that does not fit the tile, values that are not finite) is a
    ValueError before any launch."""
    return _write_host_table('strong_write_table', table, host, STRONG_TABLE_COLS, 'float32', size)


def strong_augment(images, table, mean, std, out=None, ws=None, flag=None):
    """rgda_strong_augment: colour jitter and Gaussian blur of normalised tiles, image n as row n of `table` (f32 (N, 8)
    on the device) says; include/rgda_hip.h carries the semantics.  images f32 (N,3,H,W), never written; out: the
    result (allocated unless given), a different buffer -- the blur reads neighbours, so in place is refused.  mean, std:
    three values each, the normalisation the tiles carry.  ws: workspace of rgda_strong_augment_workspace(N) bytes, a
    uint8 tensor (allocated unless given; the call rewrites it: each image's constants and its grey sum).  flag: optional device int32, set to 1 by a row whose blur is outside the served range (that image
    is copied).  -> out."""
    _need_cuda(images, table, out, ws, flag)
    if images.dim() != 4 or images.shape[1] != 3 or images.dtype != torch.float32:
        raise ValueError('strong_augment: images must be torch.float32 (N,3,H,W), got %s %s'
                         % (images.dtype, tuple(images.shape)))
    n, _, h, w = images.shape
    _table_check('strong_augment', table, n, STRONG_TABLE_COLS, torch.float32)
    mean, std = tuple(float(v) for v in mean), tuple(float(v) for v in std)
    if len(mean) != 3 or len(std) != 3 or not all(v > 0 for v in std):
        raise ValueError('strong_augment: mean and std are three values each, std positive')
    out = _out_like('strong_augment', out, images)
    ws = _ws_or('strong_augment', ws, lib().size('rgda_strong_augment_workspace', n), images.device)
    if n * h * w == 0:
        return out
    src = images.contiguous()
    if src.data_ptr() == out.data_ptr():
        raise ValueError('strong_augment: out must not be the input (the blur reads neighbouring pixels)')
    lib().call('rgda_strong_augment', src.data_ptr(), out.data_ptr(), table.data_ptr(), ws.data_ptr(), n, h, w, *mean, *std,
               _p(flag) or None, _stream())
    return out


STYLE_TABLE_COLS = _H['RGDA_STYLE_TABLE_COLS']      # {partner, b, on, 0} per source image
STYLE_MAX_B = _H['RGDA_STYLE_MAX_B']                # the widest band of swapped frequencies
STYLE_MAX_IMAGES = _H['RGDA_STYLE_MAX_IMAGES']      # source images, and target images, of one call


def fourier_style_write_table(table, host, n_targets, size):
    """rgda_fourier_style_write_table: table (int32 (N, 4) on the device, N <= 16) <- host (an int32 numpy array of that
    shape: partner, b, on, 0 per source image -- FourierStyle.draw), carried in the launch's arguments: the host buffer is
    read before this returns.  n_targets: the target images the partners index; size = (H, W) of the tiles.  A row the
    transform does not serve (a partner outside [0, n_targets), b above 64 or 2 b + 1 above min(H, W), on not 0 or 1) is a
    ValueError before any launch."""
    return _write_host_table('fourier_style_write_table', table, host, STYLE_TABLE_COLS, 'int32', size, int(n_targets))


def fourier_style_workspace(n, m, h, w, device):
    """A workspace for ops.fourier_style(ws=) at n source and m target tiles of h x w: a uint8 tensor of
    rgda_fourier_style_workspace(n, m, h, w) bytes; ValueError for a shape that is not served."""
    need = lib().size('rgda_fourier_style_workspace', int(n), int(m), int(h), int(w))
    if need == 0:
        raise ValueError('fourier_style: %d + %d tiles of %d x %d are not served (1..%d images of each, H, W <= 4096)'
                         % (n, m, h, w, STYLE_MAX_IMAGES))
    return _ws(need, device)


def fourier_style(images_s, images_t, table, mean_s, std_s, mean_t, std_t, out=None, ws=None, flag=None):
    """rgda_fourier_style: Fourier Domain Adaptation of normalised source tiles -- the amplitudes of the (2 b + 1)^2 lowest
    frequencies of source image n are replaced with those of its partner target image, as row n of `table` (int32 (N, 4)
    on the device: partner, b, on, 0) says; include/rgda_hip.h carries the semantics.  images_s f32 (N,3,H,W) and
    images_t f32 (M,3,H,W), N, M <= 16, never written; out: the result (allocated unless given), a different buffer.
    mean_*, std_*: three values each, the normalisation the source and the target tiles carry.  ws: workspace of
    rgda_fourier_style_workspace(N, M, H, W) bytes, a uint8 tensor (allocated unless given; the call rewrites it).  flag:
    optional device int32, set to 1 by a row that is not served (that image is copied).  -> out."""
    _need_cuda(images_s, images_t, table, out, ws, flag)
    for name, x in (('images_s', images_s), ('images_t', images_t)):
        if x.dim() != 4 or x.shape[1] != 3 or x.dtype != torch.float32:
            raise ValueError('fourier_style: %s must be torch.float32 (N,3,H,W), got %s %s' % (name, x.dtype, tuple(x.shape)))
    n, _, h, w = images_s.shape
    m = images_t.shape[0]
    if tuple(images_t.shape[-2:]) != (h, w):
        raise ValueError('fourier_style: source and target tiles must have one size, got %s and %s'
                         % (tuple(images_s.shape[-2:]), tuple(images_t.shape[-2:])))
    if not 1 <= n <= STYLE_MAX_IMAGES or not 1 <= m <= STYLE_MAX_IMAGES:
        raise ValueError('fourier_style: %d source and %d target images; the kernels serve 1..%d of each'
                         % (n, m, STYLE_MAX_IMAGES))
    _table_check('fourier_style', table, n, STYLE_TABLE_COLS, torch.int32)
    norms = [tuple(float(v) for v in t) for t in (mean_s, std_s, mean_t, std_t)]
    if any(len(t) != 3 for t in norms) or not all(v > 0 for v in norms[1] + norms[3]):
        raise ValueError('fourier_style: mean and std are three values each, std positive')
    out = _out_like('fourier_style', out, images_s)
    if h * w == 0:
        return out
    need = lib().size('rgda_fourier_style_workspace', n, m, h, w)
    if need == 0:
        raise ValueError('fourier_style: %d x %d tiles are not served (H, W <= 4096)' % (h, w))
    ws = _ws_or('fourier_style', ws, need, images_s.device)
    src, tgt = images_s.contiguous(), images_t.contiguous()
    if out.data_ptr() in (src.data_ptr(), tgt.data_ptr()):
        raise ValueError('fourier_style: out must not be an input (the transform is out of place)')
    lib().call('rgda_fourier_style', src.data_ptr(), tgt.data_ptr(), out.data_ptr(), table.data_ptr(), ws.data_ptr(), n, m, h, w,
               *norms[0], *norms[1], *norms[2], *norms[3], _p(flag) or None, _stream())
    return out
