"""The stage-2 ("align") inner loop of tools/train_align_reg.py:144-196 as one fused, sync-free step (SURVEY.md 8f
rank 2): a PseudoLabelStep (regda_amd/step.py) on the same kernel plans as the SSL step, without its teacher, target loss,
mix / strong and plan replay:

    model(src) -> update_prototype -> model(tgt) -> the student's own (softmax(up x1) + softmax(up x2)) / 2 as soft
    labels -> label_refine -> pseudo_selection -> Homogenizer (LRH) -> DownscaleLabel
    loss = loss_calc(src) + 0.5 * (PrototypeContrastiveLoss(src) + PrototypeContrastiveLoss(tgt))
           [+ domain_weight * CoralLoss(feat_s, feat_t)  with align_domain=True, --align-domain 1; align_domain='mmd' /
              'mmd_linear': the MMDLoss of regda/gast/mmd.py in its place (regda_amd/source.py)]
           [+ whiten_weight * 0.5 * (ClassWareWhitening(feat_s, label_s_down) + ClassWareWhitening(feat_t, label_t))
              with whiten_weight > 0: an extension, tools/train_align_reg.py never calls the whitener]
           [+ contrast_weight * 0.5 * (PixelContrastLoss(feat_s, label_s, argmax x2_s) + PixelContrastLoss(feat_t, label_t,
              argmax x2_t)) with contrast_weight > 0: an extension, tools/train_align_reg.py never constructs that loss]
           [+ triplet_weight * 0.5 * (TripletLoss(feat_s rows, label_s_down) + TripletLoss(feat_t rows, label_t)) with
              triplet_weight > 0: an extension, tools/train_align_reg.py never constructs that loss]
           [+ dca_weight * (CCR(src, tgt) + ICR(src) + ICR(tgt)) on (x1, x2, feat) of each domain with dca_weight > 0
              (regda/dca_modules.py, multi_layer=True): an extension, tools/train_align_reg.py never calls them]
           [+ saw_weight * 0.5 * (SAW(feat_s) + SAW(feat_t)) with saw_weight > 0 (regda/gast/SAW.py, the prototypes as the
              classifier): an extension, tools/train_align_reg.py never constructs that loss]
           [+ adv_weight * sum_i head_weights[i] * BCE(D_i(softmax(up(x_i of the target))), source label) with adv_weight >
              0 (regda/models/Discriminator.py): an extension, no loop of the reference trains that class;
              adv_kind='clan': adv_weight * wBCE(up(D(softmax(up x1_t + up x2_t))), source label, 1 - cos(softmax(up x1_t),
              softmax(up x2_t)), epsilon, lambda_local) in its place (regda/loss.py:60-85, regda_amd/gast/clan.py)]
    -> backward -> clip_grad_norm_(32) -> SGD

Differences to the SSL step that matter for the kernels: there is no CE on the target logits (their gradient is
zero) and the loss reaches the network through the third forward output, the instance-normalised features
(rgda_pcl_loss writes d loss / d feat pixel-major, `Deeplabv2._backward_plan(gfeat=...)` adds it in the
instance-norm backward).  The bracketed terms are the entries of TERMS below, launched in that order: each adds its
gradient onto the rows PCL wrote (bf16 accumulation, so the order is part of the result), except the adversarial term,
which adds onto the target rows of the logit gradients.  Every term is computed on the rank's local batch."""
from collections import namedtuple

import torch

from . import ops
from .ddp import all_reduce_prototype_statistics
from .gast.SAW import classifier_weight
from .gast.adversarial import AdversarialAligner
from .gast.clan import CategoryAdversarialAligner
from .gast.contrastive import select_and_plan
from .models.Discriminator import FCDiscriminator
from .source import domain_kind, domain_loss
from .step import Part, PseudoLabelStep


def saw_selection(class_num, selected_classes):
    """The classes of the SAW term: the caller's selection, or every class where their number is one SAW serves.  The
    step asks at every iteration (step.saw is read then), before it launches anything."""
    if selected_classes is None:
        if class_num not in ops.SAW_CLASS_COUNTS:
            raise ValueError(f"AlignStep(saw_weight > 0): {class_num} classes, and SAW serves {ops.SAW_CLASS_COUNTS} selected "
                             f"classes: set step.saw['selected_classes'] to that many of them")
        selected_classes = range(class_num)
    sel = [int(c) for c in selected_classes]
    if len(sel) not in ops.SAW_CLASS_COUNTS:
        raise ValueError(f"AlignStep(saw_weight > 0): {len(sel)} selected classes; SAW serves {ops.SAW_CLASS_COUNTS}")
    return sel


# One optional loss term, a row of TERMS below.  on: the attribute of the step that switches it on while > 0, read at every
# step -- its weight, a keyword checked >= 0 (the domain term goes by align_domain).  params: the defaults of `step.<name>`,
# read at every step too.  launch(step, c), then after_update(step, c) behind the model's update, for a term that is on;
# check(step, images_s, images_t) before anything is launched; construct(step) once, for a term that is on then
Term = namedtuple('Term', 'name on params launch check construct after_update', defaults=(None,) * 3)
# what a term sees of the step: per domain (features, full-size and downscaled labels, head-2 logits, gradient rows), the
# logits and their gradients, nb source images of n, the feature size, the tile size
Ctx = namedtuple('Ctx', 'sides s1 s2 t1 t2 g1 g2 nb n h w size')


def domain(step, c):
    """--align-domain 1: + aligner.align_domain(feat_s, feat_t), :188.  rgda_coral_loss (rgda_mmd_loss: regda_amd/source.py)
    adds the gradient of both halves onto the rows; domain_weight scales it.  Data-parallel ranks compute CORAL on their
    local batch (regda_amd/source.py)."""
    step.loss_domain.zero_()
    (fs, *_, rows_s), (ft, *_, rows_t) = c.sides
    domain_loss(step.domain_kind, step.mmd, fs, ft, step.domain_weight, loss=step.loss_domain, dfeat_s=rows_s,
                dfeat_t=rows_t, accumulate=True)


def whiten(step, c):
    """whiten_weight * Aligner.whiten_class_ware(feat_s, label_s, feat_t, label_t) (32 groups, alignment.py:71), on the local
    batch too: rgda_whiten_loss, added onto the same gradient rows after PCL and CORAL.  `step.loss_white` holds the term."""
    step.loss_white.zero_()
    for f, _, lab, _, rows in c.sides:
        ops.whiten_loss(f, lab, step.C, 32, step.ig, 0.5 * step.whiten_weight, loss=step.loss_white, dfeat=rows,
                        accumulate=True)


def whiten_served(step):
    k = step.prototypes.shape[-1]
    if k % 32 or k // 32 not in ops.WHITEN_BLOCKS:
        raise NotImplementedError(f'AlignStep(whiten_weight > 0): {k} feature channels in 32 groups; served are '
                                  f'{ops.WHITEN_BLOCKS} channels per group')


def contrast(step, c):
    """PixelContrastLoss, the reference's defaults (rgda_pixel_contrast_loss, added after those above; the predictions are
    the argmax of the head-2 logits at feature resolution, taken inside rgda_pixel_contrast_select; its random draws come
    from the global CPU generator, the source side first, which costs one host sync per domain and step; a domain without a
    class of more than max_views labelled pixels contributes 0).  Its parameters are kept in `step.contrast` and read at
    every step, so assigning `step.contrast['max_views'] = ...` changes them.  The head logits and the features of the
    fused model are f32, so the `.float()` below copies nothing.  `step.last_contrast` holds, per domain, the (order,
    counts, anchors, ranks) the term used, or None."""
    step.loss_contrast.zero_()
    pc = step.contrast
    for side, (f, lab, _, logits, rows) in enumerate(c.sides):
        lab = lab.reshape(lab.shape[0], *lab.shape[-2:])
        order, counts, anchors, ranks, _ = select_and_plan(lab, logits.float(), step.C, (c.h, c.w), step.ig,
                                                           pc['max_samples'], pc['max_views'], None)
        step.last_contrast[side] = None if anchors is None else (order, counts, anchors, ranks)
        if anchors is None:        # no class of this domain's batch has more than max_views pixels: the term is 0
            continue
        ops.pixel_contrast_loss(f, order, counts, anchors, ranks, pc['temperature'], pc['base_temperature'], pc['eps'],
                                0.5 * step.contrast_weight, loss=step.loss_contrast, dfeat=rows, accumulate=True)


def triplet(step, c):
    """The batch-hard TripletLoss of regda/gast/triple.py (rgda_triplet_loss, on the downscaled labels the whitening term
    uses, the step's ignore label excluded); its margin is kept in `step.triplet` and read at every step;
    `step.loss_triplet` holds the term and `step.last_triplet`, per domain, what the kernel left on the device: `stats`
    (int32: rows in the mean, positive hinges) and the per-row tables of ops.triplet_tables."""
    step.loss_triplet.zero_()
    for side, (f, _, lab, _, rows) in enumerate(c.sides):
        _, stats, ws = ops.triplet_loss(f, lab, step.triplet['margin'], step.ig, 0.5 * step.triplet_weight,
                                        loss=step.loss_triplet, dfeat=rows, accumulate=True, return_ws=True)
        step.last_triplet[side] = dict(ops.triplet_tables(ws, rows.shape[0]), stats=stats)


def dca(step, c):
    """The category alignment of regda/dca_modules.py, multi_layer=True, at the full dca_weight (rgda_dca_loss, added after
    the triplet term: it needs no labels and no host draws, its predictions are the step's own head logits at feature
    resolution, taken as constants); its parameters are kept in `step.dca` (kind 'cov' or 'mse', ccr, icr, ignore_bg) and
    read at every step; `step.loss_dca` holds the term."""
    step.loss_dca.zero_()
    dc, hw = step.dca, c.h * c.w
    (fs, *_, rows_s), (ft, *_, rows_t) = c.sides
    if dc['ccr']:        # the source side is a constant: the target rows alone receive
        ops.dca_loss(fs, (c.s1, c.s2), ft, (c.t1, c.t2), 'logits2', dc['kind'], dc['ignore_bg'], step.dca_weight,
                     loss=step.loss_dca, dfeat_b=rows_t, accumulate=True)
    if dc['icr']:
        for f, (p1, p2), rows, bd in ((fs, (c.s1, c.s2), rows_s, c.nb), (ft, (c.t1, c.t2), rows_t, c.n - c.nb)):
            q = bd // 2
            ops.dca_loss(f[:q], (p1[:q], p2[:q]), f[q:], (p1[q:], p2[q:]), 'logits2', dc['kind'], dc['ignore_bg'],
                         step.dca_weight, loss=step.loss_dca, dfeat_a=rows[:q * hw], dfeat_b=rows[q * hw:], accumulate=True)


def dca_check(step, images_s, images_t):
    if step.dca['icr'] and min(images_s.shape[0], images_t.shape[0]) < 2:
        raise ValueError('AlignStep(dca_weight > 0): icr splits the batch of each domain in two; it needs at least two '
                         'images per domain')


def saw(step, c):
    """The semantic-aware whitening of regda/gast/SAW.py (rgda_saw_loss, added after the DCA term; it needs no labels
    either).  Its parameters are kept in `step.saw` and read at every step; `step.loss_saw` holds the term.  classifier
    None: the step's prototypes, after this step's EMA update, as PCL sees them -- stage 2's PCL is a cosine classifier on
    `feat` with the prototypes as weights, so they are the (C, k) classifier this model has on that tensor; the PPM / ASPP
    heads have no 2-D weight on `feat`.  A caller's (n_cls, k) tensor or module replaces them.  selected_classes None:
    range(C) where C is one of the served counts 2, 4, 6, 8, 16; any other C (LoveDA's 7) needs a selection.  relax_denom
    defaults to 0 here, not to the reference's 2.0: `feat` is instance-normalised and the weights are sigmoids below 1, so
    each |cov| stays near or below 1 and a group's sum s over its 15 pairs (C = 6) rarely exceeds the margin 15 // 2.0 = 7
    -- the term would be identically zero: on the features of the CPU oracle's untrained network the mean s was 1.3, and
    even with strongly correlated unit-variance features on the CPU it was 8.2, with 36 % of the groups clamped at that
    margin."""
    step.loss_saw.zero_()
    sw = step.saw
    cls_w = step.prototypes if sw['classifier'] is None else classifier_weight(sw['classifier']).to(step.model.device)
    sel = saw_selection(step.C, sw['selected_classes'])
    for f, *_, rows in c.sides:
        ops.saw_loss(f, cls_w, sel, sw['relax_denom'], 0.5 * step.saw_weight, loss=step.loss_saw, dfeat=rows, accumulate=True)


def adv(step, c):
    """The output-space adversarial term (regda_amd/gast/adversarial.py, AdaptSegNet's recipe on
    regda/models/Discriminator.py's FCDiscriminator) differs from the terms above in that it reaches the network through
    the logits, not the features: after the SAW term, adv_weight * head_weights[i] * BCE(D_i(softmax(up(target logits of
    head i))), source label) adds its gradient onto the TARGET rows of the logit gradients g1 / g2, which are zero
    otherwise; after the model's update the discriminators (`discriminators=`: one per head or None for a head to skip)
    take one Adam step on the step's own detached logits of both domains.  Its parameters are kept in `step.adv` and read
    at every step; `step.loss_adv` and `step.loss_disc` hold the terms.  adv_weight = 0, the default, launches nothing.
    The discriminators' gradients are not all-reduced: with data-parallel ranks the term raises NotImplementedError.
    kind 'clan' (AlignStep(adv_kind='clan')): the category-level form of regda_amd/gast/clan.py in its place -- one
    discriminator on softmax(up x1 + up x2), its output upsampled to the tile, the BCE weighted per pixel by epsilon +
    lambda_local * (1 - cos of the two heads' probabilities), at the full adv_weight; head_weights is not read.  epsilon,
    lambda_local, preheat_steps and weight_grad of `step.adv` are the step's only source for them: they are checked (in
    adv_check, before anything is launched) and handed to the aligner at every step, over whatever was set on the aligner
    itself; a resumed state puts the saved three back into `step.adv`.  While the aligner has taken fewer than preheat_steps steps both losses are
    the plain BCE on the upsampled map."""
    if step.adv['kind'] == 'clan':
        step.adv['aligner'].set_hyper(*(step.adv[k] for k in ('epsilon', 'lambda_local', 'preheat_steps', 'weight_grad')))
        weights = step.adv_weight
    else:
        weights = [step.adv_weight * float(hw) for hw in step.adv['head_weights']]
    step.loss_adv = step.adv['aligner'].generator_term((c.t1, c.t2), (c.g1[c.nb:], c.g2[c.nb:]), weights, c.size)
    if step.keep_debug:     # tests: the step's own logits and the target rows of the logit gradients
        step.debug = dict(s1=c.s1.clone(), s2=c.s2.clone(), t1=c.t1.clone(), t2=c.t2.clone(), g1_t=c.g1[c.nb:].clone(),
                          g2_t=c.g2[c.nb:].clone())


def adv_construct(step):
    ds = step._adv_discriminators
    if step.adv['kind'] == 'clan':
        live = [] if ds is None else [d for d in ds if d is not None]
        if ds is not None and len(live) != 1:
            raise ValueError(f"AlignStep(adv_kind='clan'): one discriminator reads softmax(x1 + x2); discriminators= holds "
                             f"{len(live)}")
        d = live[0] if live else FCDiscriminator(step.C).to(step.model.device)
        a = step.adv
        step.adv['aligner'] = CategoryAdversarialAligner(d, epsilon=a['epsilon'], lambda_local=a['lambda_local'],
                                                         preheat_steps=a['preheat_steps'], weight_grad=a['weight_grad'])
        return
    if ds is None:
        ds = [FCDiscriminator(step.C).to(step.model.device) for _ in range(2)]
    step.adv['aligner'] = AdversarialAligner(ds)


def adv_check(step, images_s, images_t):
    if step.reducer.active:
        raise NotImplementedError('AlignStep(adv_weight > 0) with data-parallel ranks: the discriminators\' gradients '
                                  'are not all-reduced')
    if step.adv['aligner'] is None:
        raise ValueError("AlignStep: adv_weight was 0 at construction, so no discriminators exist; put an "
                         "AdversarialAligner into step.adv['aligner']")
    if step.adv['kind'] == 'clan':
        CategoryAdversarialAligner.check_hyper(step.adv['epsilon'], step.adv['lambda_local'], step.adv['preheat_steps'],
                                               "AlignStep(adv_kind='clan'): step.adv")
    step.adv['aligner'].check_served(images_t.shape[0], step.C, tuple(images_t.shape[-2:]))


def adv_discriminators(step, c):
    step.loss_disc = step.adv['aligner'].discriminator_step((c.s1, c.s2), (c.t1, c.t2), c.size)


# the order in which the terms add onto the gradient rows, after PCL: part of the result.  A new term goes to the end
TERMS = (Term('domain', 'align_domain', None, domain),
         Term('whiten', 'whiten_weight', None, whiten, construct=whiten_served),
         Term('contrast', 'contrast_weight', dict(temperature=0.1, base_temperature=0.07, max_samples=1024, max_views=100,
                                                  eps=1e-5), contrast),
         Term('triplet', 'triplet_weight', dict(margin=0.3), triplet),
         Term('dca', 'dca_weight', dict(kind='cov', ccr=True, icr=True, ignore_bg=True), dca, dca_check),
         Term('saw', 'saw_weight', dict(relax_denom=0.0, selected_classes=None, classifier=None), saw,
              lambda step, *images: saw_selection(step.C, step.saw['selected_classes'])),
         Term('adv', 'adv_weight', dict(head_weights=(1.0, 1.0), aligner=None, kind='adaptsegnet', epsilon=0.4,
                                        lambda_local=40.0, preheat_steps=0, weight_grad=True), adv, adv_check, adv_construct,
              adv_discriminators))
ADV_KINDS = ('adaptsegnet', 'clan')


class AlignStep(PseudoLabelStep):
    def __init__(self, model, prototypes, pcl_temperature=8.0, align_domain=False, whiten_weight=0.0, mmd=None,
                 domain_weight=1.0, contrast_weight=0.0, triplet_weight=0.0, dca_weight=0.0, saw_weight=0.0, adv_weight=0.0,
                 discriminators=None, adv_kind='adaptsegnet', proto_decay=0.999, **kw):
        weights = dict(whiten_weight=whiten_weight, contrast_weight=contrast_weight, triplet_weight=triplet_weight,
                       dca_weight=dca_weight, saw_weight=saw_weight, adv_weight=adv_weight)
        for t in TERMS:      # before the model is touched
            if t.on in weights:
                setattr(self, t.on, float(weights[t.on]))
                if getattr(self, t.on) < 0.0:
                    raise ValueError(f'AlignStep: {t.on} must be >= 0')
            if t.params is not None:
                setattr(self, t.name, dict(t.params))
        if adv_kind not in ADV_KINDS:
            raise ValueError(f'AlignStep: adv_kind is one of {ADV_KINDS}, got {adv_kind!r}')
        self.adv['kind'] = adv_kind
        self._adv_discriminators = discriminators
        self.domain_kind, self.mmd = domain_kind(align_domain, mmd)
        # proto_decay: Aligner(decay=0.999), train_align_reg.py:112-113
        super().__init__(model, prototypes, proto_decay=proto_decay, **self._refuse_ssl_only(kw))
        self.pcl_temp, self.align_domain, self.domain_weight = pcl_temperature, bool(align_domain), float(domain_weight)
        for name in ('align', 'domain', 'white', 'contrast', 'triplet', 'dca', 'saw', 'adv', 'disc'):
            setattr(self, 'loss_' + name, torch.zeros(1, device=model.device))
        self.last_contrast, self.last_triplet = [None, None], [None, None]
        for t in TERMS:
            if t.construct is not None and getattr(self, t.on) > 0.0:
                t.construct(self)

    @torch.no_grad()
    def step(self, images_s, label_s, images_t, regs_t, lr):
        """One stage-2 iteration.  Returns device tensors (loss_seg, loss_align, grad_norm_sq)."""
        for t in TERMS:
            if t.check is not None and getattr(self, t.on) > 0.0:
                t.check(self, images_s, images_t)
        self._check_shape(images_s, images_t)
        ops.set_f32(self.lr_dev, lr)
        with ops.use_stream(torch.cuda.current_stream()):
            return self._step(images_s, label_s, images_t, regs_t)

    def _state_parts(self):
        """+ the adversarial aligner; CLAN's three saved parameters go back into `step.adv`, the step's only source for them"""
        def clan(saved):
            self.adv.update({k: saved['clan'][k] for k in ('epsilon', 'lambda_local', 'preheat_steps') if 'clan' in saved})
        return [*super()._state_parts(), Part('adv', self.adv['aligner'], after=clan, hint=" (step.adv['aligner'])")]

    def _step(self, images_s, label_s, images_t, regs_t):
        m = self.model
        nb = images_s.shape[0]
        images_s = self._style_source(images_s, images_t)       # the caller's tile itself without style=
        T, main, x1, x2, feat = self._forward_domains(images_s, images_t)
        s1, t1, s2, t2 = x1[:nb], x1[nb:], x2[:nb], x2[nb:]
        feat_s, feat_t = feat[:nb], feat[nb:]
        # ema-updating prototypes comes first here (train_align_reg.py:157): the target branch sees the new ones
        label_s_down = self._proto_local(feat_s, label_s, self.reducer.active)
        if self.reducer.active:
            # data-parallel ranks (or RGDA_FORCE_DDP at world 1, as in SSLStep): all-reduce the statistics and apply the
            # totals -- the prototypes of the concatenated global batch, identical on every rank.  Through the step's
            # communicator when it has one (`comm=`: the torch-free route), else through torch.distributed
            all_reduce_prototype_statistics(self.proto_stats, self.C, self.prototypes.shape[1], self.group, self.comm,
                                            world=self.world)
            ops.proto_apply(self.prototypes, self.proto_stats, self.pdecay)
        soft_t = ops.teacher_probs(t1, t2, tuple(images_t.shape[-2:]))             # :164-166
        if self.refine_label:
            soft, cm = ops.label_refine(feat_t, self.prototypes, t1, t2, soft_t, self.temp, return_ws=True)
            hard = ops.pseudo_select(soft, self.top, self.low, self.ig, classmax_ws=cm, check=False)
        else:
            hard = ops.pseudo_select(soft_t, self.top, self.low, self.ig, check=False)
        if self.sam_refine:
            hard = self._lrh(regs_t.squeeze(1) if regs_t.dim() == 4 else regs_t, hard)
        label_t = ops.downscale_label(hard, self.C, 16, self.ig, 0.75)              # aligner.downscale_gt, :180
        # ---- losses and their gradients: d loss / d logits, the source rows from the loss kernels, the target rows zero
        g1, g2 = torch.zeros_like(x1), torch.zeros_like(x2)
        loss_seg = self._source_loss(s1, s2, label_s, g1[:nb], g2[:nb])
        n, k, h, w = feat.shape
        gfeat = torch.empty(n * h * w, k, dtype=torch.bfloat16, device=m.device)
        # per domain: features, full-size and downscaled labels, head-2 logits, its gradient rows.  PCL writes the rows
        # (it is not optional); every term that is on then adds onto them, in the order of TERMS
        sides = ((feat_s, label_s, label_s_down, s2, gfeat[:nb * h * w]), (feat_t, label_t, label_t, t2, gfeat[nb * h * w:]))
        self.loss_align.zero_()
        for f, _, lab, _, rows in sides:
            ops.pcl_loss(f, lab, self.prototypes, self.pcl_temp, self.ig, 0.5, loss=self.loss_align, dfeat=rows)
        c = Ctx(sides, s1, s2, t1, t2, g1, g2, nb, n, h, w, tuple(images_t.shape[-2:]))
        on = [t for t in TERMS if getattr(self, t.on) > 0.0]
        for t in on:
            t.launch(self, c)
        self._backward_and_update(T, main, g1, g2, gfeat=gfeat)
        for t in on:
            if t.after_update is not None:
                t.after_update(self, c)
        self.last_hard, self.last_label_t, self.last_label_s_down = hard, label_t, label_s_down
        self._keep_source(images_s)
        return loss_seg, self.loss_align, self.gn
