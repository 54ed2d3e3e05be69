"""The host side of cross-domain mixing: what to paste from the source batch over the target batch,
drawn per batch; ops.domain_mix / rgda_domain_mix does the pasting (DevicePrefetcher(mix=...) on its copy stream)."""
import numpy as np

from ..utils.cutmix import box_from_draw


class DomainMix:
    """kind 'class': ClassMix, int(class_num * ratio) classes of a permutation (regda/utils/classmix.py:42);
    kind 'box': CutMix, one box from lam ~ Beta(alpha, alpha) and a uniform centre (regda/utils/cutmix.py:17-27).
    prob: the probability that a batch is mixed at all.  The draws come from this object's own numpy Generator
    (seed), never from a global one, so a run is reproducible from the seed whatever else draws."""

    def __init__(self, kind, class_num, ratio=0.5, alpha=1.0, prob=1.0, ignore_label=-1, seed=None):
        if kind not in ('class', 'box'):
            raise ValueError("DomainMix: kind must be 'class' or 'box', got %r" % (kind,))
        if not 1 <= int(class_num) <= 32:
            raise ValueError('DomainMix: %r classes; rgda_domain_mix serves 1..32' % (class_num,))
        if not 0.0 <= ratio <= 1.0 or not 0.0 <= prob <= 1.0 or not alpha > 0:
            raise ValueError('DomainMix: ratio and prob lie in [0, 1] and alpha is positive')
        self.kind, self.class_num, self.ratio, self.alpha, self.prob = kind, int(class_num), ratio, alpha, prob
        self.ignore_label = ignore_label
        self.rng = np.random.default_rng(seed)

    # training state (regda_amd/checkpoint.py): where the generator stands.  The 128-bit words of numpy's bit generators
    # travel as decimal strings, everything else as it is
    def state_dict(self):
        def enc(v):
            if isinstance(v, dict):
                return {k: enc(x) for k, x in v.items()}
            return str(v) if isinstance(v, int) and not isinstance(v, bool) and abs(v) >= 2 ** 63 else v
        return {'rng': enc(self.rng.bit_generator.state)}

    def load_state_dict(self, sd, strict=True):
        def dec(v):
            if isinstance(v, dict):
                return {k: dec(x) for k, x in v.items()}
            return int(v) if isinstance(v, str) and v.lstrip('-').isdigit() else v
        if not isinstance(sd, dict) or not isinstance(sd.get('rng'), dict):
            raise ValueError("state entry 'DomainMix.rng' is missing")
        own = self.rng.bit_generator.state['bit_generator']
        if sd['rng'].get('bit_generator') != own:
            raise ValueError(f"state entry 'DomainMix.rng.bit_generator': {sd['rng'].get('bit_generator')!r}, this "
                             f'object draws from {own!r}')
        try:
            self.rng.bit_generator.state = dec(sd['rng'])      # numpy validates the rest and leaves the state on error
        except (KeyError, TypeError, ValueError) as e:
            raise ValueError(f"state entry 'DomainMix.rng': {e}") from None

    def draw(self, h, w):
        """One batch's draw for h x w tiles -> None (this batch is not mixed), ('classes', (ids...)) or
        ('box', (y0, y1, x0, x1)): the keyword and value ops.domain_mix takes.  Every call draws the coin first, so the
        sequence of a seed does not depend on h and w except through the box itself."""
        if self.rng.random() >= self.prob:
            return None
        if self.kind == 'class':
            ids = self.rng.permutation(self.class_num)[: int(self.class_num * self.ratio)]
            return 'classes', tuple(int(c) for c in ids)
        lam = self.rng.beta(self.alpha, self.alpha)
        cx = self.rng.uniform(0, w)
        cy = self.rng.uniform(0, h)
        return 'box', box_from_draw(lam, cx, cy, h, w)
