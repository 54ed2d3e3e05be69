"""The training transforms of regda/aug/augmentation.py on the GPU, from raw uint8 tiles.

The reference runs them per sample on the loader's CPU workers (regda/datasets/basedata.py:68-98): the image as
`torch.from_numpy(imread(...)).float().permute(2, 0, 1)`, the soft label or the class label as `mask`, the region map
as `mask_sup`.  Here the same pipeline draws each sample's parameters on the host, in the reference's order, and
one launch of `rgda_augment_tiles` writes every output of a whole batch: crop + one dihedral element (the flips and
the rotation compose into one, include/rgda_hip.h) + the normalisation as a per-(channel, byte) table.

One documented difference: the image comes in as uint8 HWC, exactly as imread returns it, not as
`.float().permute(2, 0, 1)`.  A float image of uint8 values normalises to the same bits through the table
(INTEGRATION.md shows the one-line change to BaseData).

Random draws (the mag pipeline): by default the global generators, as a `num_workers=0` loader draws them --
`torch.randint` for the crop (torchvision's RandomCrop.get_params: i, then j, nothing when the input already has the
crop size) and one `random.random()` per flip / rotation, in list order.  `rng` (a random.Random) and `generator`
(a torch.Generator) replace them."""
import random

import numpy as np
import torch

from .. import ops

# ---------------------------------------------------------------------------------------------- dihedral elements
# d = t | fr << 1 | fc << 2: output (i, j) reads crop (y, x), (u, v) = t ? (j, i) : (i, j), y = fr ? H-1-u : u,
# x = fc ? W-1-v : v.  As a signed permutation M of the centred coordinates, (y', x') = M (i', j'); applying transform
# A, then B composes to M_A @ M_B.
HFLIP = np.array([[1, 0], [0, -1]])
VFLIP = np.array([[-1, 0], [0, 1]])
ROT90 = np.array([[0, 1], [-1, 0]])         # torch.rot90(x, 1, [1, 2]) == np.rot90 on HW: R[i][j] = X[j][S-1-i]
IDENTITY = np.eye(2, dtype=np.int64)


def code(m):
    """signed permutation matrix -> d."""
    t = int(m[0][0] == 0)
    fr = int((m[0][1] if t else m[0][0]) < 0)
    fc = int((m[1][0] if t else m[1][1]) < 0)
    return t | fr << 1 | fc << 2


def matrix(d):
    """d -> signed permutation matrix (inverse of `code`)."""
    t, sr, sc = d & 1, -1 if d & 2 else 1, -1 if d & 4 else 1
    return np.array([[0, sr], [sc, 0]]) if t else np.array([[sr, 0], [0, sc]])


# ---------------------------------------------------------------------------------------------- tables
def label_table(offset=0, num_class=6, ignore_label=-1):
    """int32 [256]: byte -> `byte + offset`, then `mask[mask >= n_classes] = ignore_label` (basedata.py:83-88).  Both
    steps are pointwise, so they commute with the geometry."""
    v = torch.arange(256, dtype=torch.int64) + offset
    v[v >= num_class] = ignore_label
    return v.to(torch.int32)


def identity_table():
    """f32 [3][256]: the byte's value (a pipeline without Normalize hands the float image on)."""
    return torch.arange(256, dtype=torch.float32).expand(3, 256).contiguous()


def affine_row(y0, x0, m, b, ho, wo, h, w, fill=(0, 0, 0)):
    """One row (cy, cx, a00, a01, a10, a11, fill, 0) of rgda_augment_affine's table: the crop at (y0, x0) of an h x w tile,
    the output-to-source map p -> m p + b in the crop's centred coordinates (b in pixels), the fill colour.  A centre
    that b moves off the tile is clamped to its edge."""
    cy = min(max((2 * y0 + ho) * 32768 + int(round(float(b[0]) * 65536)), 0), h * 65536)
    cx = min(max((2 * x0 + wo) * 32768 + int(round(float(b[1]) * 65536)), 0), w * 65536)
    a = [int(round(float(v) * 32768)) for v in (m[0][0], m[0][1], m[1][0], m[1][1])]
    return [cy, cx] + a + [int(fill[0]) | int(fill[1]) << 8 | int(fill[2]) << 16, 0]


class _Pipeline:
    """Crop size, composed geometric draws and the two tables of one pipeline; the launch is shared by both pipelines.
    Subclasses implement `sample(h, w) -> (y0, x0, d)` and `table()`; `crop` is the output size (None: the input's).
    A pipeline that holds a scale / rotation transform (`affine`) implements `sample_affine(h, w) -> (y0, x0, m, b)`
    instead, has `param_cols = 8` and launches rgda_augment_affine."""
    crop = None
    affine = None
    param_cols = 4

    def __init__(self, offset=0, num_class=6, ignore_label=-1):
        self.offset, self.num_class, self.ignore_label = offset, num_class, ignore_label
        self._dev = {}

    def label_table(self):
        return label_table(self.offset, self.num_class, self.ignore_label)

    def device_tables(self, device):
        """(f32 [3][256], int32 [256]) on `device`, built once."""
        key = str(torch.device(device))
        if key not in self._dev:
            self._dev[key] = (self.table().to(device), self.label_table().to(device))
        return self._dev[key]

    def out_size(self, h, w):
        return tuple(self.crop) if self.crop is not None else (h, w)

    def params(self, n, h, w):
        """int32 [n][4] (y0, x0, d, 0): the draws of n consecutive samples of h x w inputs, in order.  With a scale /
        rotation transform: int32 [n][8] (cy, cx, a00, a01, a10, a11, fill, 0), the rows of rgda_augment_affine."""
        if self.param_cols == 8:
            ho, wo = self.out_size(h, w)
            rows = []
            for i in range(n):
                y0, x0, m, b = self.sample_affine(h, w)
                rows.append(affine_row(y0, x0, m, b, ho, wo, h, w, self.affine.fill))
            return torch.tensor(rows, dtype=torch.int32)
        p = torch.zeros(n, 4, dtype=torch.int32)
        for i in range(n):
            p[i, :3] = torch.tensor(self.sample(h, w), dtype=torch.int32)
        return p

    def check_params(self, params, h, w):
        """Host-side check of a CPU table of `params()` for h x w inputs; raises ValueError."""
        if self.param_cols == 8:
            ops.check_affine_params(params, h, w)
        else:
            ops.check_augment_params(params, h, w, *self.out_size(h, w))

    def launch(self, img, params, lut, size, label=None, label_lut=None, soft=None, regs=None, out=None):
        """The pipeline's one launch on device tensors: rgda_augment_tiles, or rgda_augment_affine for [N][8] rows."""
        if self.param_cols == 8:
            return ops.augment_affine(img, params, lut, size, label=label, label_lut=label_lut,
                                      ignore_label=self.ignore_label, soft=soft, regs=regs, out=out)
        return ops.augment_tiles(img, params, lut, size, label=label, label_lut=label_lut, soft=soft, regs=regs, out=out)

    def batch(self, images_u8, mask=None, soft=None, mask_sup=None, out=None, params=None):
        """images_u8 uint8 [N][H][W][3]; mask uint8 [N][H][W] class labels (through the label table); soft f32
        [N][C][H][W]; mask_sup int32 [N][H][W] region ids.  Tensors on the host are copied to the current device.
        Draws each sample's parameters in order (or takes `params`, int32 [N][param_cols]) and issues one launch.
        -> {'image': f32 [N][3][Ho][Wo], 'mask': int64 [N][Ho][Wo], 'soft': f32 [N][C][Ho][Wo],
            'mask_sup': int64 [N][1][Ho][Wo]} (None where the input is None)."""
        dev = torch.device('cuda', torch.cuda.current_device())
        mv = lambda t: None if t is None else (t if t.is_cuda else t.to(dev)).contiguous()
        images_u8, mask, soft, mask_sup = mv(images_u8), mv(mask), mv(soft), mv(mask_sup)
        n, h, w, _ = images_u8.shape
        ho, wo = self.out_size(h, w)
        if params is None:
            params = self.params(n, h, w)
        lut, llut = self.device_tables(images_u8.device)
        names = dict(image='image', label='mask', soft='soft', regs='mask_sup')
        o = None if out is None else {k: out.get(v) for k, v in names.items()}
        r = self.launch(images_u8, params, lut, (ho, wo), label=mask, label_lut=llut, soft=soft, regs=mask_sup, out=o)
        return {v: r[k] for k, v in names.items()}

    def __call__(self, image, mask=None, mask_sup=None):
        """One sample, one launch, the reference's dict: image uint8 [H][W][3]; mask uint8 [H][W] class labels or f32
        [C][H][W] soft labels; mask_sup int32 [H][W] or [1][H][W].  -> {'image', 'mask', 'mask_sup'} on the GPU."""
        soft = lab = None
        if mask is not None:
            if mask.dtype == torch.uint8:
                lab = mask[None]
            else:
                soft = mask[None]
        sup = None if mask_sup is None else mask_sup.reshape(1, image.shape[0], image.shape[1])
        r = self.batch(image[None], mask=lab, soft=soft, mask_sup=sup)
        m = r['mask'][0] if lab is not None else (r['soft'][0] if soft is not None else None)
        return {'image': r['image'][0], 'mask': m, 'mask_sup': None if sup is None else r['mask_sup'][0]}


# ---------------------------------------------------------------------------------------------- the reference's classes
class RandomHorizontalFlip:
    m = HFLIP

    def __init__(self, prob):
        self.prob = prob


class RandomVerticalFlip:
    m = VFLIP

    def __init__(self, prob):
        self.prob = prob


class RandomRotate90:
    m = ROT90                                # torch.rot90(image, k=1, dims=[1, 2])

    def __init__(self, prob):
        self.prob = prob


class RandomCrop:
    def __init__(self, size):
        self.size = size

    def get_params(self, h, w, generator=None):
        """torchvision's RandomCrop.get_params: (i, j); no draw when the input already has the crop size."""
        th, tw = self.size
        if h < th or w < tw:
            raise ValueError('Required crop size %s is larger than input image size %s' % ((th, tw), (h, w)))
        if w == tw and h == th:
            return 0, 0
        i = torch.randint(0, h - th + 1, size=(1,), generator=generator).item()
        j = torch.randint(0, w - tw + 1, size=(1,), generator=generator).item()
        return i, j


class Normalize:
    def __init__(self, mean, std, clamp=False):
        self.mean = mean
        self.std = std
        self.clamp = clamp

    def table(self):
        """f32 [3][256]: torchvision's F.normalize on a float image (`tensor.sub_(mean).div_(std)`, mean / std as f32
        tensors), computed with torch on the CPU, then `torch.clamp(max=1.0)` when clamp."""
        mean = torch.as_tensor(self.mean, dtype=torch.float32).view(3, 1)
        std = torch.as_tensor(self.std, dtype=torch.float32).view(3, 1)
        v = torch.arange(256, dtype=torch.float32).expand(3, 256).clone()
        v.sub_(mean).div_(std)
        if self.clamp:
            v = torch.clamp(v, max=1.0)
        return v.contiguous()


class RandomScaleRotate:
    """Random rescaling and rotation about the crop's centre (this project's own transform; rgda_augment_affine).  With
    probability `prob` the crop is magnified by s, uniform in scale = (lo, hi), and turned by theta, uniform in
    [-degrees, degrees]: the output-to-source matrix is (1/s) [[cos, -sin], [sin, cos]] on centred (row, column)
    coordinates.  Pixels whose source lies outside the raw tile take `fill` (r, g, b bytes), the ignore label, region 0
    and an all-zero soft label."""

    def __init__(self, scale=(1.0, 1.0), degrees=0.0, prob=0.5, fill=(0, 0, 0)):
        lo, hi = scale
        if not 0.25 <= lo <= hi <= 4:
            raise ValueError('RandomScaleRotate: scale=(lo, hi) needs 0.25 <= lo <= hi <= 4, got %r' % (scale,))
        if not 0 <= degrees <= 180:
            raise ValueError('RandomScaleRotate: degrees must lie in [0, 180], got %r' % (degrees,))
        if len(fill) != 3 or any(int(v) != v or not 0 <= v <= 255 for v in fill):
            raise ValueError('RandomScaleRotate: fill is three bytes (r, g, b), got %r' % (fill,))
        self.scale, self.degrees, self.prob, self.fill = (lo, hi), degrees, prob, tuple(int(v) for v in fill)

    def draw(self, rng):
        """Three draws whatever the coin says (the coin, s, theta) -> the 2 x 2 matrix, or None when the coin fails."""
        coin, s, theta = rng.random(), rng.uniform(*self.scale), rng.uniform(-self.degrees, self.degrees)
        if coin >= self.prob:
            return None
        return rotation(s, theta)


def rotation(s, theta):
    """(1/s) [[cos, -sin], [sin, cos]], theta in degrees: the output-to-source matrix of a magnification by s and a turn
    by theta."""
    c, sn = np.cos(np.deg2rad(theta)), np.sin(np.deg2rad(theta))
    return np.array([[c, -sn], [sn, c]]) / s


_GEOM = (RandomHorizontalFlip, RandomVerticalFlip, RandomRotate90)


class Compose(_Pipeline):
    """Compose([RandomCrop?, flips / rotation..., Normalize?]) of the reference (mag) pipeline; at most one
    RandomScaleRotate among the flips.
    rng: random.Random for the flip / rotation draws (default: the `random` module); generator: torch.Generator for
    the crop (default: torch's global generator).  offset / num_class / ignore_label: the label table (IsprsDA's)."""

    def __init__(self, transforms, rng=None, generator=None, offset=0, num_class=6, ignore_label=-1):
        super().__init__(offset, num_class, ignore_label)
        self.transforms = list(transforms)
        self.rng = random if rng is None else rng
        self.generator = generator
        kinds = [type(t) for t in self.transforms]
        for i, t in enumerate(self.transforms):
            if isinstance(t, RandomCrop) and i != 0:
                raise ValueError('RandomCrop must come first')
            if isinstance(t, Normalize) and i != len(self.transforms) - 1:
                raise ValueError('Normalize must come last')
            if not isinstance(t, (RandomCrop, Normalize, RandomScaleRotate) + _GEOM):
                raise ValueError('unsupported transform %r' % (t,))
        self.crop = tuple(self.transforms[0].size) if kinds and kinds[0] is RandomCrop else None
        self.norm = self.transforms[-1] if kinds and kinds[-1] is Normalize else None
        warps = [t for t in self.transforms if isinstance(t, RandomScaleRotate)]
        if len(warps) > 1:
            raise ValueError('at most one RandomScaleRotate')
        if warps:
            self.affine, self.param_cols = warps[0], 8

    def sample_affine(self, h, w):
        """-> (y0, x0, m, b): the crop origin and the composed output-to-source map p -> m p + b (b = 0 here)."""
        y0 = x0 = 0
        m = IDENTITY
        for t in self.transforms:
            if isinstance(t, RandomCrop):
                y0, x0 = t.get_params(h, w, self.generator)
            elif isinstance(t, _GEOM):
                if self.rng.random() < t.prob:
                    m = m @ t.m
            elif isinstance(t, RandomScaleRotate):
                mt = t.draw(self.rng)
                if mt is not None:
                    m = m @ mt
        return y0, x0, m, (0.0, 0.0)

    def sample(self, h, w):
        y0, x0, m, _ = self.sample_affine(h, w)
        return y0, x0, code(m)

    def table(self):
        return self.norm.table() if self.norm is not None else identity_table()
