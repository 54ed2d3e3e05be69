"""The stage-1 ("source") inner loop of tools/train_src.py:117-140 as one fused, sync-free step, on the same kernel
plans as the SSL step; a FusedStep (regda_amd/step.py), so the optimizer tail, the source loss and the state are shared:

    model(src) [-> model(tgt)] -> loss = loss_calc(src) [+ CORAL(feat_s, feat_t)  with --align-domain 1]
    -> backward -> clip_grad_norm_(32) -> SGD

No EMA, no prototypes, no label path.  With align_domain the source and the target batch run through the network
together as two BatchNorm groups (statistics per domain, as the reference's two forward calls); the target heads get
a zero gradient (train_src.py discards the target logits) and CORAL reaches the network through the instance-normalised
features: rgda_coral_loss writes d CORAL / d feat for both halves pixel-major, `Deeplabv2._backward_plan(gfeat=...)`
adds it in the instance-norm backward.

align_domain='mmd' / 'mmd_linear' puts the MMD of regda/gast/mmd.py (rgda_mmd_loss; the reference's commented
`self.mmd`, alignment.py:68) in CORAL's place, on the same gradient rows; `mmd=dict(kernel_mul=, kernel_num=, fix_sigma=)`
sets its kernel parameters and `domain_weight` scales either domain term.

fada_weight > 0 adds the feature-space, class-level adversarial term of regda_amd/gast/fada.py (FADA's recipe on
regda/models/Discriminator.py:60-78's PixelDiscriminator) onto the same rows: after CORAL / MMD,
fada_weight * l(D(feat_t), a_t, source side) adds its gradient onto the TARGET rows (there is no adversarial term on the
source features); after the model's update the discriminator (`pixel_discriminator=`, default
PixelDiscriminator(2048, 512, class_num)) takes one Adam step on the step's own detached features and head-2 logits of
both domains.  Both domains then run as two BatchNorm groups even without align_domain (the rows start at zero).
`step.fada = dict(aligner=, temperature=, clip=)` is read at every step; `step.loss_fada` and `step.loss_fada_disc` hold
the terms.  fada_weight = 0, the default, launches exactly what the step launched before.  The discriminator's gradients
are not all-reduced: with data-parallel ranks the term raises NotImplementedError.

Data-parallel ranks compute CORAL / MMD on their local batch (the rank's own source and target pixels),
the same per-rank semantics as the per-GPU BatchNorm statistics: there is no extra collective."""
import torch

from . import ops
from .gast.fada import FeatureAdversarialAligner
from .models.PixelDiscriminator import PixelDiscriminator
from .step import FusedStep, Part

BF = torch.bfloat16

MMD_OPTIONS = ('kernel_mul', 'kernel_num', 'fix_sigma')


def domain_kind(align_domain, mmd=None):
    """align_domain False / True / 'coral' / 'mmd' / 'mmd_linear' -> (kind or None, the MMD keyword arguments)"""
    kinds = {False: None, True: 'coral', 'coral': 'coral', 'mmd': 'mmd', 'mmd_linear': 'mmd_linear'}
    if not isinstance(align_domain, (bool, int, str)) or align_domain not in kinds:       # 0 / 1 as False / True
        raise ValueError(f"align_domain {align_domain!r}; served are False, True, 'coral', 'mmd' and 'mmd_linear'")
    mmd = dict(mmd or {})
    if set(mmd) - set(MMD_OPTIONS):
        raise ValueError(f'mmd: unknown options {sorted(set(mmd) - set(MMD_OPTIONS))}; served are {MMD_OPTIONS}')
    return kinds[align_domain], mmd


def domain_loss(kind, mmd, feat_s, feat_t, weight, **kw):
    """the domain term of a fused step: CORAL or MMD of the two halves of the feature map, onto the gradient rows"""
    if kind == 'coral':
        return ops.coral_loss(feat_s, feat_t, weight, **kw)
    return ops.mmd_loss(feat_s, feat_t, weight, 'linear' if kind == 'mmd_linear' else 'rbf', **mmd, **kw)


class SourceStep(FusedStep):
    _STATE_LEGACY = ('prototypes',)     # states written while this class derived from SSLStep carry a zero tensor

    def __init__(self, model, class_balancer_s=None, align_domain=False, class_num=6, loss_s='CrossEntropy', mmd=None,
                 domain_weight=1.0, fada_weight=0.0, pixel_discriminator=None, **kw):
        self.fada_weight = float(fada_weight)
        if not self.fada_weight >= 0.0:         # before the model is touched
            raise ValueError('SourceStep: fada_weight must be >= 0')
        self.domain_kind, self.mmd = domain_kind(align_domain, mmd)
        super().__init__(model, class_num=class_num, class_balancer_s=class_balancer_s, loss_s=loss_s,
                         **self._refuse_ssl_only(kw))
        self.align_domain = bool(align_domain)
        self.domain_weight = float(domain_weight)
        self.loss_domain = torch.zeros(1, device=model.device)
        self.loss_fada = torch.zeros(1, device=model.device)
        self.loss_fada_disc = torch.zeros(1, device=model.device)
        self.fada = dict(aligner=None, temperature=1.8, clip=0.9)
        if self.fada_weight > 0.0:
            d = pixel_discriminator
            if d is None:
                d = PixelDiscriminator(2048, 512, class_num).to(model.device)
            self.fada['aligner'] = FeatureAdversarialAligner(d)

    @torch.no_grad()
    def step(self, images_s, label_s, images_t, lr):
        """One stage-1 iteration.  Returns device tensors (loss_seg, loss_domain, grad_norm_sq); loss_domain stays 0
        without align_domain.  images_t may be None when align_domain, fada_weight and style are off (no target forward
        then; style= reads the target tiles' spectra and needs them even without a target forward)."""
        if self.align_domain and images_t is None:
            raise ValueError('SourceStep(align_domain=True) needs the target images')
        if self.style is not None and images_t is None:
            raise ValueError('SourceStep(style=) needs the target images')
        if self.fada_weight > 0.0:
            self._fada_check(images_s, images_t)
        self._check_shape(images_s, images_t if self.align_domain or self.fada_weight > 0.0 else None)
        ops.set_f32(self.lr_dev, lr)
        with ops.use_stream(torch.cuda.current_stream()):
            return self._step(images_s, label_s, images_t)

    def _fada_check(self, images_s, images_t):
        if images_t is None:
            raise ValueError('SourceStep(fada_weight > 0) needs the target images')
        if self.reducer.active:
            raise NotImplementedError('SourceStep(fada_weight > 0) with data-parallel ranks: the discriminator\'s gradients '
                                      'are not all-reduced')
        aligner = self.fada['aligner']
        if aligner is None:
            raise ValueError("SourceStep: fada_weight was 0 at construction, so no discriminator exists; put a "
                             "FeatureAdversarialAligner into step.fada['aligner']")
        T, clip = float(self.fada['temperature']), float(self.fada['clip'])
        if not T > 0.0 or not 0.0 < clip <= 1.0:
            raise ValueError(f"SourceStep: step.fada needs temperature > 0 and 0 < clip <= 1, got {T!r} and {clip!r}")
        h, w = ((int(v) + 15) // 16 for v in images_t.shape[-2:])      # the feature map lies at output stride 16
        aligner.check_served((images_t.shape[0], 2048, h, w), (images_t.shape[0], self.C, h, w))

    def _state_parts(self):
        """+ the adversarial term's discriminator and its Adam moments"""
        return [*super()._state_parts(), Part('fada', self.fada['aligner'], hint=" (step.fada['aligner'])")]

    def _step(self, images_s, label_s, images_t):
        m = self.model
        nb = images_s.shape[0]
        fada = self.fada_weight > 0.0
        images_s = self._style_source(images_s, images_t)       # the caller's tile itself without style=
        # both domains run as two BatchNorm groups where a term reads the target features; else the source batch alone
        T, main, x1, x2, feat = self._forward_domains(*((images_s, images_t) if self.align_domain or fada else (images_s,)))
        # d(loss) / d(logits): the source rows from the CE kernel, the target rows (when there are any) zero
        g1, g2 = torch.zeros_like(x1), torch.zeros_like(x2)
        loss_seg = self._source_loss(x1[:nb], x2[:nb], label_s, g1[:nb], g2[:nb])
        self.loss_domain.zero_()
        gfeat = None
        if self.align_domain:
            n, k, h, w = feat.shape
            gfeat = torch.empty(n * h * w, k, dtype=BF, device=m.device)
            domain_loss(self.domain_kind, self.mmd, feat[:nb], feat[nb:], self.domain_weight, loss=self.loss_domain,
                        dfeat_s=gfeat[:nb * h * w], dfeat_t=gfeat[nb * h * w:])
        if fada:
            aligner = self.fada['aligner']
            aligner.temperature, aligner.clip = float(self.fada['temperature']), float(self.fada['clip'])
            n, k, h, w = feat.shape
            if gfeat is None:       # no domain term: the rows start at zero
                gfeat = torch.zeros(n * h * w, k, dtype=BF, device=m.device)
            feat_s, feat_t, rows_t = feat[:nb], feat[nb:], gfeat[nb * h * w:]
            before = rows_t.clone() if self.keep_debug else None
            self.loss_fada = aligner.generator_term(feat_t, x2[nb:], rows_t, self.fada_weight)
            if self.keep_debug:     # tests: the step's own features and head-2 logits, the target rows before and after
                self.debug = dict(feat_s=feat_s.clone(), feat_t=feat_t.clone(), s2=x2[:nb].clone(), t2=x2[nb:].clone(),
                                  rows_t_before=before, rows_t=rows_t.clone())
        self._backward_and_update(T, main, g1, g2, gfeat=gfeat)
        if fada:
            self.loss_fada_disc = aligner.discriminator_step(feat_s, x2[:nb], feat_t, x2[nb:])
        self._keep_source(images_s)
        return loss_seg, self.loss_domain, self.gn
