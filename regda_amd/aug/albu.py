"""The albumentations pipeline of the source domain and of evaluation (configs/ToPotsdam.py `_TRAIN_AUG` /
`_EVAL_AUG`: albumentations 1.3.0 RandomCrop, OneOf([HorizontalFlip, VerticalFlip, RandomRotate90], p=0.75), Normalize,
ToTensor) on the GPU, from raw uint8 tiles, through the same launch as regda_amd.aug.augmentation.

This reproduces the pipeline's DISTRIBUTION, not albumentations' random stream (which is not pinned here): crop
offsets uniform over the valid origins; OneOf applies with probability p and then picks one child, weighted by the
children's p (the config builds them with always_apply=True, so with equal weight); RandomRotate90 draws k uniformly
from 0..3.  All draws come from `rng` (a random.Random; default: the `random` module).

Normalize is albumentations 1.3.0's `normalize` as restated below (f32 `mean * max_pixel_value`, the f32 reciprocal of
`std * max_pixel_value`, subtract, then multiply), tabulated per (channel, byte).  It is a restatement, not pinned
against albumentations: its cv2 branch could differ by <= 1 ulp, and switching to it changes one line of `table()`."""
import random

import numpy as np
import torch

from .augmentation import HFLIP, IDENTITY, ROT90, VFLIP, _Pipeline, code, identity_table, rotation


class _Child:
    def __init__(self, always_apply=False, p=0.5):
        self.always_apply = always_apply
        self.p = p


class HorizontalFlip(_Child):
    def element(self, rng):
        return HFLIP


class VerticalFlip(_Child):
    def element(self, rng):
        return VFLIP


class RandomRotate90(_Child):
    def element(self, rng):
        """np.rot90(img, k), k uniform in 0..3."""
        return np.linalg.matrix_power(ROT90, rng.randint(0, 3))


class OneOf:
    def __init__(self, transforms, p=0.5):
        self.transforms = list(transforms)
        self.p = p
        s = sum(t.p for t in self.transforms)
        self.weights = [t.p / s for t in self.transforms]

    def element(self, rng):
        if rng.random() >= self.p:
            return IDENTITY
        t = rng.choices(self.transforms, weights=self.weights)[0]
        return t.element(rng)


class ShiftScaleRotate:
    """albumentations' ShiftScaleRotate with a constant border (rgda_augment_affine): with probability p, an angle uniform
    in [-rotate_limit, rotate_limit] degrees (counter-clockwise as displayed, cv2's convention), a scale uniform in
    [1 - scale_limit, 1 + scale_limit] and a shift uniform in [-shift_limit, shift_limit] of the output's height and
    width.  A limit may also be a (lo, hi) pair instead of a symmetric bound: shift and rotate pairs are the range
    itself, a scale pair is, as in albumentations, a pair of offsets from 1 (scale_limit=(-0.5, 1.0) draws the scale from
    [0.5, 2]).  border_mode: only 0 (cv2.BORDER_CONSTANT), value the
    fill colour; albumentations' default reflecting border is not provided.  Five draws whatever the coin says.  The
    distribution is albumentations'; the bilinear weights are the kernel's 8-bit ones, not cv2's 5-bit ones."""

    def __init__(self, shift_limit=0.0625, scale_limit=0.1, rotate_limit=45, border_mode=0, value=(0, 0, 0),
                 always_apply=False, p=0.5):
        if border_mode != 0:
            raise ValueError('ShiftScaleRotate: only border_mode=0 (cv2.BORDER_CONSTANT) is provided, got %r' % (border_mode,))
        pair = lambda v, bias=0.0: tuple(bias + x for x in (v if isinstance(v, (tuple, list)) else (-v, v)))
        self.shift, self.scale, self.rotate = pair(shift_limit), pair(scale_limit, 1.0), pair(rotate_limit)
        if not 0.25 <= self.scale[0] <= self.scale[1] <= 4:
            raise ValueError('ShiftScaleRotate: the scale must stay inside [1/4, 4], got %r' % (self.scale,))
        value = (value,) * 3 if isinstance(value, (int, float)) else tuple(value)
        if len(value) != 3 or any(int(v) != v or not 0 <= v <= 255 for v in value):
            raise ValueError('ShiftScaleRotate: value is a byte or three bytes (r, g, b), got %r' % (value,))
        self.fill, self.always_apply, self.p = tuple(int(v) for v in value), always_apply, p

    def draw(self, rng, ho, wo):
        """-> (m, b) of the output-to-source map p -> m p + b in centred (row, column) pixels, or None."""
        coin, angle, s = rng.random(), rng.uniform(*self.rotate), rng.uniform(*self.scale)
        dx, dy = rng.uniform(*self.shift), rng.uniform(*self.shift)
        if not self.always_apply and coin >= self.p:
            return None
        # cv2 turns counter-clockwise with rows pointing down: in (row, column) order that is rotation(s, -angle); the
        # warped content moves by (dy ho, dx wo), so the source of p is m (p - shift)
        m = rotation(s, -angle)
        return m, -(m @ np.array([dy * ho, dx * wo]))


class RandomCrop:
    def __init__(self, height, width, always_apply=False, p=1.0):
        self.height, self.width = height, width

    def get_params(self, h, w, rng):
        """uniform origin: int((h - height + 1) * u) for u uniform in [0, 1), as albumentations' get_random_crop_coords."""
        if h < self.height or w < self.width:
            raise ValueError('Requested crop size (%d, %d) is larger than the image size (%d, %d)' % (
                self.height, self.width, h, w))
        return int((h - self.height + 1) * rng.random()), int((w - self.width + 1) * rng.random())


class Normalize:
    def __init__(self, mean=(0.485, 0.456, 0.406), std=(0.229, 0.224, 0.225), max_pixel_value=255.0,
                 always_apply=False, p=1.0):
        self.mean, self.std, self.max_pixel_value = mean, std, max_pixel_value

    def table(self):
        """f32 [3][256]: albumentations 1.3.0 `normalize(img, mean, std, max_pixel_value)` on a uint8 image."""
        mean = np.array(self.mean, dtype=np.float32)
        mean *= self.max_pixel_value
        std = np.array(self.std, dtype=np.float32)
        std *= self.max_pixel_value
        denominator = np.reciprocal(std, dtype=np.float32)
        img = np.broadcast_to(np.arange(256, dtype=np.uint8)[None, :], (3, 256)).astype(np.float32)
        img -= mean[:, None]
        img *= denominator[:, None]
        return torch.from_numpy(np.ascontiguousarray(img))


class ToTensor:
    """HWC -> CHW float image, int64 mask: what the launch writes anyway."""


class Compose(_Pipeline):
    """Compose([RandomCrop?, HorizontalFlip / VerticalFlip / RandomRotate90 / OneOf..., Normalize?, ToTensor?]); at most
    one ShiftScaleRotate among the flips.
    rng: random.Random (default: the `random` module); offset / num_class / ignore_label: the label table (IsprsDA's)."""

    def __init__(self, transforms, rng=None, offset=0, num_class=6, ignore_label=-1):
        super().__init__(offset, num_class, ignore_label)
        self.transforms = [t for t in transforms if not isinstance(t, ToTensor)]
        self.rng = random if rng is None else rng
        geom = (HorizontalFlip, VerticalFlip, RandomRotate90, OneOf, ShiftScaleRotate)
        for i, t in enumerate(self.transforms):
            if isinstance(t, RandomCrop) and i != 0:
                raise ValueError('RandomCrop must come first')
            if isinstance(t, Normalize) and i != len(self.transforms) - 1:
                raise ValueError('Normalize must come last')
            if not isinstance(t, (RandomCrop, Normalize) + geom):
                raise ValueError('unsupported transform %r' % (t,))
        ts = self.transforms
        self.crop = (ts[0].height, ts[0].width) if ts and isinstance(ts[0], RandomCrop) else None
        self.norm = ts[-1] if ts and isinstance(ts[-1], Normalize) else None
        warps = [t for t in ts if isinstance(t, ShiftScaleRotate)]
        if len(warps) > 1:
            raise ValueError('at most one ShiftScaleRotate')
        if warps:
            self.affine, self.param_cols = warps[0], 8

    def sample_affine(self, h, w):
        """-> (y0, x0, m, b): the crop origin and the composed output-to-source map p -> m p + b."""
        y0 = x0 = 0
        m, b = IDENTITY, np.zeros(2)
        for t in self.transforms:
            if isinstance(t, RandomCrop):
                y0, x0 = t.get_params(h, w, self.rng)
            elif isinstance(t, OneOf):
                m = m @ t.element(self.rng)
            elif isinstance(t, _Child):
                if t.always_apply or self.rng.random() < t.p:
                    m = m @ t.element(self.rng)
            elif isinstance(t, ShiftScaleRotate):
                drawn = t.draw(self.rng, *self.out_size(h, w))
                if drawn is not None:
                    m, b = m @ drawn[0], b + m @ drawn[1]
        return y0, x0, m, b

    def sample(self, h, w):
        y0, x0, m, _ = self.sample_affine(h, w)
        return y0, x0, code(m)

    def table(self):
        return self.norm.table() if self.norm is not None else identity_table()
