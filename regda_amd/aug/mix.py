"""The host side of cross-domain mixing: what to paste from the source batch over the target batch,
drawn per batch; ops.domain_mix / rgda_domain_mix does the pasting (DevicePrefetcher(mix=...) on its copy stream), or,
inside a training step, ops.domain_mix_table / rgda_domain_mix_table from `draw_step` (SSLStep(mix=...))."""
import numpy as np

from ..utils.cutmix import box_from_draw


def rng_state_dict(rng):
    """Where a numpy Generator stands, as a training state entry (DomainMix, StrongAugment).  The 128-bit words of
    numpy's bit generators travel as decimal strings, everything else as it is."""
    def enc(v):
        if isinstance(v, dict):
            return {k: enc(x) for k, x in v.items()}
        return str(v) if isinstance(v, int) and not isinstance(v, bool) and abs(v) >= 2 ** 63 else v
    return {'rng': enc(rng.bit_generator.state)}


def load_rng_state_dict(rng, sd, who):
    """The inverse of rng_state_dict: validated first, nothing written on error (ValueError naming `who`)."""
    def dec(v):
        if isinstance(v, dict):
            return {k: dec(x) for k, x in v.items()}
        return int(v) if isinstance(v, str) and v.lstrip('-').isdigit() else v
    if not isinstance(sd, dict) or not isinstance(sd.get('rng'), dict):
        raise ValueError(f"state entry '{who}.rng' is missing")
    own = rng.bit_generator.state['bit_generator']
    if sd['rng'].get('bit_generator') != own:
        raise ValueError(f"state entry '{who}.rng.bit_generator': {sd['rng'].get('bit_generator')!r}, this "
                         f'object draws from {own!r}')
    try:
        rng.bit_generator.state = dec(sd['rng'])      # numpy validates the rest and leaves the state on error
    except (KeyError, TypeError, ValueError) as e:
        raise ValueError(f"state entry '{who}.rng': {e}") from None


class DomainMix:
    """kind 'class': ClassMix, int(class_num * ratio) classes of a permutation (regda/utils/classmix.py:42);
    kind 'box': CutMix, one box from lam ~ Beta(alpha, alpha) and a uniform centre (regda/utils/cutmix.py:17-27).
    kind 'dacs': DACS, per image half of the classes that occur in its source label map -- the labels live on the device,
    so the host draws one permutation per image (the classes' ranks) and rgda_mix_select_classes chooses; only a training
    step can use it (`draw_step`).
    prob: the probability that a batch is mixed at all.  The draws come from this object's own numpy Generator
    (seed), never from a global one, so a run is reproducible from the seed whatever else draws."""

    def __init__(self, kind, class_num, ratio=0.5, alpha=1.0, prob=1.0, ignore_label=-1, seed=None):
        if kind not in ('class', 'box', 'dacs'):
            raise ValueError("DomainMix: kind must be 'class', 'box' or 'dacs', got %r" % (kind,))
        if not 1 <= int(class_num) <= 32:
            raise ValueError('DomainMix: %r classes; rgda_domain_mix serves 1..32' % (class_num,))
        if not 0.0 <= ratio <= 1.0 or not 0.0 <= prob <= 1.0 or not alpha > 0:
            raise ValueError('DomainMix: ratio and prob lie in [0, 1] and alpha is positive')
        self.kind, self.class_num, self.ratio, self.alpha, self.prob = kind, int(class_num), ratio, alpha, prob
        self.ignore_label = ignore_label
        self.rng = np.random.default_rng(seed)

    # training state (regda_amd/checkpoint.py): where the generator stands
    def state_dict(self):
        return rng_state_dict(self.rng)

    def load_state_dict(self, sd, strict=True):
        load_rng_state_dict(self.rng, sd, 'DomainMix')

    def draw(self, h, w):
        """One batch's draw for h x w tiles -> None (this batch is not mixed), ('classes', (ids...)) or
        ('box', (y0, y1, x0, x1)): the keyword and value ops.domain_mix takes.  Every call draws the coin first, so the
        sequence of a seed does not depend on h and w except through the box itself."""
        if self.kind == 'dacs':
            raise ValueError("DomainMix('dacs') chooses among the classes of each source label map, on the device: it is "
                             "drawn by a training step (SSLStep(mix=...)), not per batch on the host")
        if self.rng.random() >= self.prob:
            return None
        if self.kind == 'class':
            ids = self.rng.permutation(self.class_num)[: int(self.class_num * self.ratio)]
            return 'classes', tuple(int(c) for c in ids)
        lam = self.rng.beta(self.alpha, self.alpha)
        cx = self.rng.uniform(0, w)
        cy = self.rng.uniform(0, h)
        return 'box', box_from_draw(lam, cx, cy, h, w)

    def draw_step(self, n, h, w):
        """What a training step needs for one batch of n images of h x w -> None (not mixed), ('classes', ids) or
        ('box', box), one draw for all n images and the same values `draw` gives for this seed, or, for kind 'dacs',
        ('ranks', uint8 [n][class_num]): one rng.permutation(class_num) per image, image by image, row i the ranks of image
        i's classes (rgda_mix_select_classes keeps the present classes of smallest rank).  The coin comes first, as in
        `draw`."""
        if self.kind != 'dacs':
            return self.draw(h, w)
        if self.rng.random() >= self.prob:
            return None
        return 'ranks', np.stack([self.rng.permutation(self.class_num) for _ in range(int(n))]).astype(np.uint8)
