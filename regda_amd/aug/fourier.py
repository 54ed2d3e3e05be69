"""The host side of the Fourier style transfer of the source tile ("Fourier style transfer"): which target
image lends its low-frequency amplitudes to each source image of a batch, and how wide the swapped window is, drawn per
batch; ops.fourier_style / rgda_fourier_style applies it on the device (the steps' style=...)."""
import math

import numpy as np

from .mix import load_rng_state_dict, rng_state_dict
from .strong import MEAN, STD

TABLE_COLS = 4          # RGDA_STYLE_TABLE_COLS: {partner, b, on, 0} per source image
MAX_B = 64              # RGDA_STYLE_MAX_B
MAX_IMAGES = 16         # RGDA_STYLE_MAX_IMAGES


def _norm(who, mean, std, cls='FourierStyle'):
    mean, std = tuple(float(v) for v in mean), tuple(float(v) for v in std)
    if len(mean) != 3 or len(std) != 3 or not all(v > 0 and math.isfinite(v) for v in std) \
            or not all(math.isfinite(v) for v in mean):
        raise ValueError('%s: %s are three finite values each, std positive' % (cls, who))
    return mean, std


class FourierStyle:
    """Fourier Domain Adaptation (Yang and Soatto, CVPR 2020): with probability prob a source image takes the amplitudes
    of its (2 b + 1)^2 lowest frequencies from a target image of the batch, drawn uniformly, and keeps its own phase;
    b = floor(min(H, W) * beta), beta a float or (low, high) to draw it uniformly per image.  mean_s / std_s and
    mean_t / std_t: the normalisations the source and the target tiles carry (the swap acts on the raw grey scale).

    The reference has no such pass; beta = 0.01 is the smallest of the published settings (0.01, 0.05, 0.09).  The draws
    come from this object's own numpy Generator (seed), as DomainMix's do."""

    def __init__(self, beta=0.01, prob=1.0, mean_s=MEAN, std_s=STD, mean_t=MEAN, std_t=STD, seed=None):
        try:
            beta = tuple(float(v) for v in beta)
        except TypeError:
            beta = (float(beta), float(beta))
        if len(beta) != 2 or not 0.0 <= beta[0] <= beta[1] or not math.isfinite(beta[1]):
            raise ValueError('FourierStyle: beta is a float or (low, high) with 0 <= low <= high, got %r' % (beta,))
        if not 0.0 <= prob <= 1.0:
            raise ValueError('FourierStyle: prob lies in [0, 1]')
        self.beta, self.prob = beta, float(prob)
        self.mean_s, self.std_s = _norm('mean_s and std_s', mean_s, std_s)
        self.mean_t, self.std_t = _norm('mean_t and std_t', mean_t, std_t)
        self.rng = np.random.default_rng(seed)

    # training state (regda_amd/checkpoint.py): where the generator stands
    def state_dict(self):
        return rng_state_dict(self.rng)

    def load_state_dict(self, sd, strict=True):
        load_rng_state_dict(self.rng, sd, 'FourierStyle')

    @staticmethod
    def half_width(h, w, beta):
        """b = floor(min(h, w) * beta)"""
        return int(math.floor(min(int(h), int(w)) * float(beta)))

    def draw(self, n, m, h, w):
        """One batch's table, int32 (n, 4): row i = {partner in [0, m), b, on, 0} for n source and m target images of
        h x w.  Per image, in this order: the coin, the partner, beta -- three draws whether or not the coin fires, so the
        sequence of a seed does not depend on the outcomes.  The values of a row that is off stay in it; the kernel does
        not read them."""
        n, m = int(n), int(m)
        if not 1 <= n <= MAX_IMAGES or not 1 <= m <= MAX_IMAGES:
            raise ValueError('FourierStyle.draw: %d source and %d target images; served are 1..%d of each' % (n, m, MAX_IMAGES))
        top = self.half_width(h, w, self.beta[1])
        if top > MAX_B or 2 * top + 1 > min(int(h), int(w)):
            raise ValueError('FourierStyle.draw: beta %g gives b = %d at %d x %d tiles; served are b <= %d and '
                             '2 b + 1 <= min(H, W)' % (self.beta[1], top, h, w, MAX_B))
        t = np.zeros((n, TABLE_COLS), np.int32)
        r = self.rng
        for i in range(n):
            on = r.random() < self.prob
            partner = int(r.integers(m))
            beta = r.uniform(self.beta[0], self.beta[1])
            t[i, :3] = (partner, self.half_width(h, w, beta), int(on))
        return t

    # what a step's style= calls (regda_amd/step.py: _style_source); HistogramStyle has the same three
    def workspace(self, n, m, h, w, device):
        from .. import ops
        return ops.fourier_style_workspace(n, m, h, w, device)

    def write_table(self, table, rows, n_targets, size):
        from .. import ops
        return ops.fourier_style_write_table(table, rows, n_targets, size)

    def apply(self, images_s, images_t, table, ws=None, flag=None):
        from .. import ops
        return ops.fourier_style(images_s, images_t, table, self.mean_s, self.std_s, self.mean_t, self.std_t, ws=ws, flag=flag)
