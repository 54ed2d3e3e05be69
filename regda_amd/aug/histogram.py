"""The host side of the histogram matching of the source tile ("Histogram matching"): which target
image lends its grey-level distribution to each source image of a batch, and how far the match is blended in, drawn per
batch; hist_style / rgda_hist_style applies it on the device (the steps' style=...).  The functional wrappers
(regda_amd/_ops/histogram.py) are re-exported here: this module is their public home until they join regda_amd.ops."""
import numpy as np

from .._ops.histogram import hist_style, hist_style_workspace, hist_style_write_table  # noqa: F401
from .fourier import MAX_IMAGES, TABLE_COLS, _norm
from .mix import load_rng_state_dict, rng_state_dict
from .strong import MEAN, STD

BLEND_ONE = 65536       # RGDA_HIST_BLEND_ONE: blend_q of a full match


class HistogramStyle:
    """Per-channel histogram matching (scikit-image's match_histograms, albumentations' HistogramMatching): with
    probability prob a source image takes the grey-level distribution of a target image of the batch, drawn uniformly;
    the matched image is blended with the source, out = source + blend * (matched - source), blend a float or (low, high)
    within [0, 1] to draw it uniformly per image.  mean_s / std_s and mean_t / std_t: the normalisations the source and
    the target tiles carry (the levels are those of the raw grey scale).

    The reference has no such pass.  The draws come from this object's own numpy Generator (seed), as FourierStyle's do."""

    def __init__(self, blend=(0.5, 1.0), prob=1.0, mean_s=MEAN, std_s=STD, mean_t=MEAN, std_t=STD, seed=None):
        try:
            blend = tuple(float(v) for v in blend)
        except TypeError:
            blend = (float(blend), float(blend))
        if len(blend) != 2 or not 0.0 <= blend[0] <= blend[1] <= 1.0:
            raise ValueError('HistogramStyle: blend is a float or (low, high) with 0 <= low <= high <= 1, got %r' % (blend,))
        if not 0.0 <= prob <= 1.0:
            raise ValueError('HistogramStyle: prob lies in [0, 1]')
        self.blend, self.prob = blend, float(prob)
        self.mean_s, self.std_s = _norm('mean_s and std_s', mean_s, std_s, 'HistogramStyle')
        self.mean_t, self.std_t = _norm('mean_t and std_t', mean_t, std_t, 'HistogramStyle')
        self.rng = np.random.default_rng(seed)

    # training state (regda_amd/checkpoint.py): where the generator stands
    def state_dict(self):
        return rng_state_dict(self.rng)

    def load_state_dict(self, sd, strict=True):
        load_rng_state_dict(self.rng, sd, 'HistogramStyle')

    @staticmethod
    def blend_q(blend):
        """blend in [0, 1] -> the table's integer: round(blend * 65536)"""
        return int(round(float(blend) * BLEND_ONE))

    def draw(self, n, m, h, w):
        """One batch's table, int32 (n, 4): row i = {partner in [0, m), blend_q, on, 0} for n source and m target images of
        h x w.  Per image, in this order: the coin, the partner, the blend -- three draws whether or not the coin fires, so
        the sequence of a seed does not depend on the outcomes.  The values of a row that is off stay in it; the kernel
        does not read them."""
        n, m = int(n), int(m)
        if not 1 <= n <= MAX_IMAGES or not 1 <= m <= MAX_IMAGES:
            raise ValueError('HistogramStyle.draw: %d source and %d target images; served are 1..%d of each' % (n, m, MAX_IMAGES))
        if not 1 <= int(h) <= 4096 or not 1 <= int(w) <= 4096:
            raise ValueError('HistogramStyle.draw: %d x %d tiles; served are H, W in 1..4096' % (h, w))
        t = np.zeros((n, TABLE_COLS), np.int32)
        r = self.rng
        for i in range(n):
            on = r.random() < self.prob
            partner = int(r.integers(m))
            blend = r.uniform(self.blend[0], self.blend[1])
            t[i, :3] = (partner, self.blend_q(blend), int(on))
        return t

    # what a step's style= calls (regda_amd/step.py: _style_source); FourierStyle has the same three
    def workspace(self, n, m, h, w, device):
        return hist_style_workspace(n, m, h, w, device)

    def write_table(self, table, rows, n_targets, size):
        return hist_style_write_table(table, rows, n_targets, size)

    def apply(self, images_s, images_t, table, ws=None, flag=None):
        return hist_style(images_s, images_t, table, self.mean_s, self.std_s, self.mean_t, self.std_t, ws=ws, flag=flag)
