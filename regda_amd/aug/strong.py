"""The host side of the strong (photometric) augmentation of the student's tile ("Strong augmentation"):
what colour jitter and Gaussian blur each image of a batch gets, drawn per batch; ops.strong_augment /
rgda_strong_augment applies it on the device (SSLStep(strong=...))."""
import math

import numpy as np

from .mix import load_rng_state_dict, rng_state_dict

TABLE_COLS = 8          # RGDA_STRONG_TABLE_COLS: {fb, fc, fs, theta, sigma, flags, 0, 0} per image
JITTER, BLUR = 1, 2     # the bits of `flags`
MEAN = (123.675, 116.28, 103.53)        # the configs' normalisation
STD = (58.395, 57.12, 57.375)


class StrongAugment:
    """Colour jitter with probability jitter_prob -- brightness, contrast and saturation factors uniform in
    [1 - x, 1 + x], a hue rotation of theta = 2 pi h radians with h uniform in [-hue, hue] (a fraction of the colour
    circle) -- and a Gaussian blur with probability blur_prob, sigma uniform in [sigma[0], sigma[1]].  mean / std: the
    normalisation the step's tiles carry (rgda_strong_augment computes on the 0..1 image).

    The reference has no strong augmentation; these defaults are this project's own choice (the usual weak end of the
    DACS / mean-teacher recipes), not values taken from it.  The draws come from this object's own numpy Generator
    (seed), as DomainMix's do."""

    def __init__(self, jitter_prob=0.2, brightness=0.2, contrast=0.2, saturation=0.2, hue=0.05, blur_prob=0.5,
                 sigma=(0.15, 1.15), mean=MEAN, std=STD, seed=None):
        if not 0.0 <= jitter_prob <= 1.0 or not 0.0 <= blur_prob <= 1.0:
            raise ValueError('StrongAugment: jitter_prob and blur_prob lie in [0, 1]')
        if not all(0.0 <= v <= 1.0 for v in (brightness, contrast, saturation)) or not 0.0 <= hue <= 0.5:
            raise ValueError('StrongAugment: brightness, contrast and saturation lie in [0, 1], hue in [0, 0.5]')
        sigma = tuple(float(v) for v in sigma)
        if len(sigma) != 2 or not 0.0 < sigma[0] <= sigma[1] <= 4.0:
            raise ValueError('StrongAugment: sigma is (low, high) with 0 < low <= high <= 4, got %r' % (sigma,))
        mean, std = tuple(float(v) for v in mean), tuple(float(v) for v in std)
        if len(mean) != 3 or len(std) != 3 or not all(v > 0 and math.isfinite(v) for v in std) \
                or not all(math.isfinite(v) for v in mean):
            raise ValueError('StrongAugment: mean and std are three finite values each, std positive')
        self.jitter_prob, self.blur_prob = float(jitter_prob), float(blur_prob)
        self.brightness, self.contrast, self.saturation, self.hue = (float(v) for v in (brightness, contrast, saturation, hue))
        self.sigma, self.mean, self.std = sigma, mean, std
        self.rng = np.random.default_rng(seed)

    # training state (regda_amd/checkpoint.py): where the generator stands
    def state_dict(self):
        return rng_state_dict(self.rng)

    def load_state_dict(self, sd, strict=True):
        load_rng_state_dict(self.rng, sd, 'StrongAugment')

    def draw(self, n):
        """One batch's table, f32 (n, 8): row i = {fb, fc, fs, theta, sigma, flags, 0, 0}, flags = JITTER * (jitter coin)
        + BLUR * (blur coin).  Per image, in this order: the jitter coin, fb, fc, fs, h, the blur coin, sigma -- seven
        draws whether or not a coin fires, so the sequence of a seed does not depend on the outcomes.  The values of a
        switch that is off stay in the row; the kernel does not read them."""
        n = int(n)
        if n < 1:
            raise ValueError('StrongAugment.draw: %d images' % n)
        t = np.zeros((n, TABLE_COLS), np.float32)
        r = self.rng
        for i in range(n):
            jitter = r.random() < self.jitter_prob
            fb = r.uniform(1.0 - self.brightness, 1.0 + self.brightness)
            fc = r.uniform(1.0 - self.contrast, 1.0 + self.contrast)
            fs = r.uniform(1.0 - self.saturation, 1.0 + self.saturation)
            h = r.uniform(-self.hue, self.hue)
            blur = r.random() < self.blur_prob
            sigma = r.uniform(self.sigma[0], self.sigma[1])
            t[i, :6] = (fb, fc, fs, 2.0 * math.pi * h, sigma, JITTER * jitter + BLUR * blur)
        return t
