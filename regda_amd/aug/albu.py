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

from .augmentation import HFLIP, IDENTITY, ROT90, VFLIP, _Pipeline, code, identity_table


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
    """Compose([RandomCrop?, HorizontalFlip / VerticalFlip / RandomRotate90 / OneOf..., Normalize?, ToTensor?]).
    rng: random.Random (default: the `random` module); offset / num_class / ignore_label: the label table (IsprsDA's)."""

    def __init__(self, transforms, rng=None, offset=0, num_class=6, ignore_label=-1):
        super().__init__(offset, num_class, ignore_label)
        self.transforms = [t for t in transforms if not isinstance(t, ToTensor)]
        self.rng = random if rng is None else rng
        geom = (HorizontalFlip, VerticalFlip, RandomRotate90, OneOf)
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

    def sample(self, h, w):
        y0 = x0 = 0
        m = IDENTITY
        for t in self.transforms:
            if isinstance(t, RandomCrop):
                y0, x0 = t.get_params(h, w, self.rng)
            elif isinstance(t, OneOf):
                m = m @ t.element(self.rng)
            elif isinstance(t, _Child):
                if t.always_apply or self.rng.random() < t.p:
                    m = m @ t.element(self.rng)
        return y0, x0, code(m)

    def table(self):
        return self.norm.table() if self.norm is not None else identity_table()
