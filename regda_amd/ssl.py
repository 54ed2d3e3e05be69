"""The self-training (SSL) inner loop of tools/train_ssl_reg.py:198-241 as ONE fused, sync-free step.

Same composition and hyper-parameters as the reference loop --
    model(src), model(tgt) -> label_refine -> pseudo_selection -> Homogenizer (LRH) -> update_prototype
    -> loss_calc x2 -> backward -> clip_grad_norm_(32) -> SGD(momentum .9, wd 5e-4)
-- but driven directly over the HIP kernel plans (no autograd graph, no host sync, no .item()):
flat gradient buffer, bucketed RCCL all-reduce overlapped with the second backward pass, and one fused
clip + SGD (+ EMA shadow + bf16 weight mirror) kernel.  Optionally the soft target labels come from an
online EMA teacher (regda/utils/ema.py semantics: parameters averaged, BN buffers shared) instead of
the offline `.pt` files of the reference (BASELINE.json north_star; SURVEY.md header table).
SSLStep is a PseudoLabelStep (regda_amd/step.py: the optimizer tail, the gradient exchange, the source loss, the state walk,
prototypes and LRH live there, and style=, the Fourier style transfer of the source tile); its own are the teacher, the
target loss, mix / strong and the recorded plans and graphs.
"""
import numpy as np
import torch

from . import ops
from . import plan
from .ddp import all_reduce_prototype_statistics
from .gast.balance import target_loss
from .checkpoint import check_module_state
from .step import Part, PseudoLabelStep, check_generator


class SSLStep(PseudoLabelStep):
    def __init__(self, model, prototypes, ema_decay=None, class_balancer_t=None, loss_t='none', uvem_m=0.2, uvem_t=0.7,
                 uvem_g=4.0, gdp_prototype=True, gdp_class_balance=False, ent_weight=0.0, kld_weight=0.0, adv_weight=0.0,
                 discriminators=None, mix=None, strong=None, pycda_weight=0.0, pycda_sizes=(8, 16, 32, 64, 0),
                 pycda_thresh=0.5, overlap_weight_t=0.0, **kw):
        if adv_weight or discriminators is not None:
            raise NotImplementedError('the adversarial term (adv_weight / discriminators) belongs to the stage-2 step, AlignStep')
        # PyCDA's region pyramid term (regda_amd/gast/pycda.py) on the target logits and the label path's
        # soft label: one rgda_upsample_pycda call behind the target loss and its regularisers that adds its gradient onto
        # theirs.  Weight 0: no launch.  Checked before the model is touched.
        self.pycda_weight, self.pycda_sizes = float(pycda_weight), ops.pycda_sizes(pycda_sizes)
        self.pycda_thresh = float(pycda_thresh)
        if not self.pycda_weight >= 0.0 or not 0.0 <= self.pycda_thresh <= 1.0:
            raise ValueError(f'{type(self).__name__}: pycda_weight must be >= 0 and pycda_thresh in [0, 1]')
        # The overlap term (FusedStep: overlap_weight_s, overlap=) on the student's target logits against the step's final
        # pseudo labels (with mix= the pasted copy; unlabelled pixels are ignored): one rgda_upsample_overlap call behind
        # the pyramid term that adds its gradient onto the target loss's.  Weight 0: no launch.
        self.overlap_weight_t = self._overlap_weight(overlap_weight_t, 'overlap_weight_t')
        super().__init__(model, prototypes, **kw)
        class_num, ignore_label, dev = self.C, self.ig, model.device
        self.ema_decay = ema_decay
        if ema_decay is not None:
            self.teacher = model.make_teacher()
        self.source_side = self.wgrad_stream is not None    # source half of the label path on the second stream
        # --bct, --lt (+ --uvem-m/-t/-g) of tools/train_ssl_reg.py:52-63,125-158, as --bcs and --ls in regda_amd/step.py
        self.class_balancer_t = class_balancer_t
        # loss_t='gdp': GDPLoss (balance.py:218-303).  gdp_prototype adds the prototype weight of every pseudo-labelled
        # pixel (Aligner.get_prototype_weight_4pixel on feat_t and the step's final pseudo labels, from the prototypes as
        # label_refine reads them), gdp_class_balance the class weight (class_balancer_t if given, else the loss's own)
        self.loss_fn_t = target_loss(loss_t, class_balancer_t, uvem_m, uvem_t, uvem_g, class_num, ignore_label,
                                     device=dev, gdp_prototype=gdp_prototype, gdp_class_balance=gdp_class_balance)
        self.last_proto_weight = None
        # IAST's region regularisers (regda/utils/tools.py:376-398) on the target logits and the step's final pseudo
        # labels: ent_weight * entropy over the ignored pixels + kld_weight * KLD-to-uniform over the labelled ones, one
        # rgda_upsample_reg call behind the target loss that adds its gradient onto that loss's.  Both 0: no launch.
        self.ent_weight, self.kld_weight = float(ent_weight), float(kld_weight)
        self.loss_ent = self.loss_kld = None    # the unscaled terms of the last step (device tensors)
        self.loss_pycda = self.pycda_active = None      # f32 [1 + L]: the unscaled total and levels of the last step; int32 [L]
        self.pycda_flag = torch.zeros(1, dtype=torch.int32, device=dev) if self.pycda_weight > 0.0 else None
        self._pycda_bufs = {}       # shape -> (workspace, loss, n_active): allocated once
        # mix: a regda_amd.aug.mix.DomainMix (kind 'class', 'box' or 'dacs') -- DACS inside the step: the
        # student's target tile is the source batch pasted over images_t, the teacher (or the offline soft labels) labels
        # the clean tile, and the source labels are pasted onto the pseudo labels after selection and LRH.  None: no launch.
        if mix is not None and mix.class_num != class_num:
            raise ValueError(f'{type(self).__name__}: mix draws among {mix.class_num} classes, the step has {class_num}')
        self.mix = mix
        self.mix_flag = torch.zeros(1, dtype=torch.int32, device=dev) if mix is not None else None
        self.last_mix = self.last_mix_table = None      # the last step's draw (host) and the table its kernels read
        # strong: a regda_amd.aug.strong.StrongAugment -- colour jitter and Gaussian blur of the student's target tile, after
        # the mix where there is one: the teacher, the caller's images_t, soft_t and the source tile are
        # never touched, the result is a buffer of the step's own.  None: no launch.
        self.strong = strong
        self.strong_flag = torch.zeros(1, dtype=torch.int32, device=dev) if strong is not None else None
        self.last_strong = None     # the last step's table as drawn on the host, f32 (N, 8)
        self._graph = self._plan = None

    # ------------------------------------------------------------------
    @torch.no_grad()
    def step(self, images_s, label_s, images_t, soft_t, regs_t, lr):
        """One SSL iteration.  Returns device tensors (loss_source, loss_target, grad_norm_sq): nothing here
        synchronises with the host."""
        self._check_shape(images_s, images_t)
        if self._graph is not None:
            return self._replay(images_s, label_s, images_t, soft_t, regs_t, lr)
        if self._plan is not None:
            return self._replay_plan(images_s, label_s, images_t, soft_t, regs_t, lr)
        ops.set_f32(self.lr_dev, lr)
        with ops.use_stream(torch.cuda.current_stream()):
            return self._step(images_s, label_s, images_t, soft_t, regs_t)

    def capture(self, images_s, label_s, images_t, soft_t, regs_t):
        """Capture one whole step (both streams) into a hipGraph; later `step()` calls replay it.  The step is a
        static launch sequence over fixed shapes, so replay removes the ~20 ms of per-step host launch work.
        Call after at least one eager step, or after load_state_dict() of a run that has stepped (momentum
        initialisation is a different kernel variant)."""
        self._check_shape(images_s, images_t)
        assert not self.first, 'run one eager step before capture()'
        if self.world > 1:
            raise RuntimeError('whole-step graphs are single-GPU; the multi-GPU path stays eager')
        if self._host_balancers():
            # ClassBalance.next_class_weight rebinds its frequency tensor and is host arithmetic: a graph would keep the
            # address of the pre-capture tensor and never advance the EMA.  record_plan() re-runs it as a host action.
            raise RuntimeError('class balancing (--bcs / --bct) is host-side state: use record_plan(), not capture()')
        if self.mix is not None:
            # the draws come from the DomainMix's generator on the host and travel as kernel arguments, which a graph
            # freezes: record_plan() re-runs the draw and the table write as a host action
            raise RuntimeError('the cross-domain mix (mix=) draws on the host: use record_plan(), not capture()')
        if self.strong is not None:
            # the same: the table is drawn on the host and travels as kernel arguments
            raise RuntimeError('the strong augmentation (strong=) draws on the host: use record_plan(), not capture()')
        if self.style is not None:
            raise RuntimeError('the style transfer of the source tile (style=) draws on the host: use record_plan(), not capture()')
        self._static = self._static_inputs(images_s, label_s, images_t, soft_t, regs_t)
        self._build_maps(images_s)
        torch.cuda.synchronize()
        m = self.model
        m._hw_ready = m._wt_ready = None          # everything recorded before the synchronize is complete
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            with ops.use_stream(torch.cuda.current_stream()):
                self._out = self._step(*self._static)
                if self.wgrad_stream is not None:   # the weight re-layouts issued on the second stream at the end
                    torch.cuda.current_stream().wait_stream(self.wgrad_stream)     # of the step join the graph
        m._hw_ready = m._wt_ready = None          # (they are events inside the graph now: nothing to wait for outside)
        self._graph = g

    def _build_maps(self, images):
        """The models' host-built operand tables for these tiles, made before a recording or capture starts
        (Deeplabv2.build_maps): a step loaded from a saved state may not have run a forward yet."""
        for net in (self.model, self.teacher):
            if net is not None:
                net.build_maps(*images.shape[-2:])

    @staticmethod
    def _static_inputs(images_s, label_s, images_t, soft_t, regs_t):
        """Static input buffers of a recorded / captured step, in the dtype and layout the step's kernels read (the
        conversions `_step` would otherwise do with torch ops at record time only): fp32 contiguous images and soft
        labels, int64 contiguous labels and region maps.  `copy_` into them converts whatever the caller passes."""
        conv = lambda t, dt: None if t is None else t.detach().to(dt).contiguous().clone()
        return [conv(images_s, torch.float32), conv(label_s, torch.int64), conv(images_t, torch.float32),
                conv(soft_t, torch.float32), conv(regs_t, torch.int64)]

    def teacher_model(self):
        """The EMA teacher, ready to be evaluated or saved: shadow weights as they stand, BatchNorm buffers adopted from
        the student NOW (the teacher keeps a snapshot, not an alias: with offline soft labels nothing else refreshes
        it), bf16 mirror current, eval mode."""
        t = self.teacher
        if t is None:
            return None
        t.adopt_buffers(self.model)
        t.refresh_from_master(mirror_is_fresh=(not self.first) and t.flat_p._version == t._synced_version)
        t.eval()
        return t

    # ------------------------------------------------------------------ training state (regda_amd/step.py)
    _STATE_CONFIG_FREE = ('ema_decay',)     # recorded; whether there is a teacher is what a load compares

    def _state_config(self):
        return dict(super()._state_config(), loss_t=self.loss_fn_t.kind, ema_decay=self.ema_decay)

    def _state_parts(self):
        t = self.teacher    # behind its load, flat_pb and _synced_version agree with the shadow again
        return [Part('teacher', t, check_module_state, lambda saved: t.refresh_from_master(), ' (ema_decay)'),
                *super()._state_parts(), Part('class_balancer_t', self.class_balancer_t, check_module_state),
                Part('loss_fn_t', self.loss_fn_t, check_module_state), Part('mix', self.mix, check_generator),
                Part('strong', self.strong, check_generator)]

    def _state_loads(self, sd, strict):
        if self._graph is not None:     # (a recorded plan stays valid: it replays the loaded state)
            raise RuntimeError(f'{type(self).__name__}.load_state_dict: this step holds a captured graph, which owns '
                               f'generator state that a load cannot restore: load the state first and capture() afterwards')
        loads = super()._state_loads(sd, strict)
        if sd.get('first') and self._plan is not None:
            raise ValueError("state entry 'step.first': the state is that of a run that has not stepped, and this "
                             "step holds a recorded plan, which is the optimizer's later variant: release_plan() first")
        return loads

    def record_plan(self, images_s, label_s, images_t, soft_t, regs_t, lr=None):
        """Record one whole step (all streams) as a launch plan (regda_amd/plan.py): its ~750 entry-point calls become
        rows of a table that `rgda_plan_run` walks in C, the torch ops / stream waits between them stay host actions.
        Later `step()` calls replay the plan on the recorded buffers (a private memory pool): same kernels, same
        streams, same results as the eager step, a fraction of the host time.  Call after at least one eager step, or
        after load_state_dict() of a run that has stepped (the first step initialises the momentum with another kernel
        variant).  Inputs are copied into static buffers at every replay; the returned tensors (losses, `last_hard`,
        ...) are overwritten by the next step."""
        self._check_shape(images_s, images_t)
        assert not self.first, 'run one eager step before record_plan()'
        assert self._graph is None and self._plan is None
        self._static = self._static_inputs(images_s, label_s, images_t, soft_t, regs_t)
        if lr is not None:          # recording IS a real step: run it with this learning rate (default: the last one)
            ops.set_f32(self.lr_dev, lr)
        self._build_maps(images_s)
        torch.cuda.synchronize()
        self._plan_stream = torch.cuda.current_stream()
        p = plan.Plan()

        def run():
            with ops.use_stream(torch.cuda.current_stream()):
                return self._step(*self._static)
        self._out = p.record(run)
        self._plan = p
        return p.stats()

    def release_plan(self):
        self._plan = None

    def static_inputs(self):
        """The recorded step's input buffers {name: device tensor}: a loader may write the next batch straight into
        them once `inputs_consumed()` of the running step has passed (regda_amd/utils/prefetch.py)."""
        assert self._plan is not None or self._graph is not None
        names = ('images_s', 'label_s', 'images_t', 'soft_t', 'regs_t')
        return dict(zip(names, self._static))

    def inputs_consumed(self):
        """Event of the most recently enqueued step: recorded behind the last kernel that reads the step's inputs."""
        return self._inputs_done.ev

    def _replay_plan(self, images_s, label_s, images_t, soft_t, regs_t, lr):
        # the table rows carry the stream handles of the recording: the input copies and the learning-rate fill must
        # be ordered on that same stream, whatever stream the caller has made current
        rec = self._plan_stream
        cur = torch.cuda.current_stream()
        if cur != rec:
            rec.wait_stream(cur)
        with ops.use_stream(rec):       # host-action entry points (class weights, ...) land on the recorded stream too
            for dst, src in zip(self._static, (images_s, label_s, images_t, soft_t, regs_t)):
                assert (dst is None) == (src is None), 'a recorded step keeps its input signature (soft labels or not)'
                if dst is not None and src is not dst:
                    dst.copy_(src, non_blocking=True)
            ops.set_f32(self.lr_dev, lr)
            m = self.model
            if not m.training:
                m.train()
            if m.flat_p._version != m._synced_version:      # weights were changed from outside (load_state_dict, ...)
                m.sync_weights()
            self._plan.replay()
        if cur != rec:
            cur.wait_stream(rec)
        return self._out

    def _replay(self, images_s, label_s, images_t, soft_t, regs_t, lr):
        for dst, src in zip(self._static, (images_s, label_s, images_t, soft_t, regs_t)):
            if dst is not None and src is not dst:
                dst.copy_(src, non_blocking=True)
        ops.set_f32(self.lr_dev, lr)
        self._graph.replay()
        return self._out

    def _host_balancers(self):
        """Whether a ClassBalance takes part in the step's losses (ohem, focal and ghm targets take none)."""
        return super()._host_balancers() or self.loss_fn_t.class_balancer is not None

    def _target_loss(self, t1, t2, hard, soft, g1, g2, proto_weight=None):
        """loss_calc / loss_calc_uvem(target, loss_fn_t) on the pseudo labels (ups / uvem also read the refined soft label,
        gdp the prototype weights of the pseudo labels)."""
        f = self.loss_fn_t
        if f.kind == 'gdp':
            return f.launch(t1, t2, hard, class_weight=self._class_weights(f.class_balancer, hard), g1=g1, g2=g2,
                            pixel_weight=proto_weight)[0]
        return f.launch(t1, t2, hard, soft=soft if f.kind in ('ups', 'uvem') else None,
                        class_weight=self._class_weights(f.class_balancer, hard), g1=g1, g2=g2)[0]

    def _target_regularisers(self, t1, t2, hard, g1, g2):
        """IAST's entropy / KLD terms on the pseudo labels' ignored / labelled regions (derived in the kernel, no weight
        tensor); their gradient is added onto the target loss's in g1, g2.  An empty region gives a term of 0.  Ranks
        of a data-parallel run use their local counts, like every other loss of the step."""
        terms = (ops.REG_ENT if self.ent_weight else 0) | (ops.REG_KLD if self.kld_weight else 0)
        if not terms:
            return
        reg = ops.upsample_reg(t1, t2, hard, terms=terms, lambda_ent=self.ent_weight, lambda_kld=self.kld_weight,
                               ignore_label=self.ig, g1=g1, g2=g2, accumulate=True, empty_is_zero=True)[0]
        self.loss_ent, self.loss_kld = reg[0], reg[1]

    def _target_pyramid(self, t1, t2, soft, g1, g2):
        """PyCDA's region term: the student's mean prediction over the squares of every level against the soft label's
        mean there (the label path's soft label: refined, and with mix= the pasted copy); its gradient is added onto the
        target loss's in g1, g2.  Ranks of a data-parallel run use their local region counts."""
        if not self.pycda_weight > 0.0:
            return
        key = (tuple(t1.shape), tuple(soft.shape))
        if key not in self._pycda_bufs:
            nl = len(self.pycda_sizes)
            self._pycda_bufs[key] = (ops.upsample_pycda_workspace(t1, soft.shape, self.pycda_sizes),
                                     torch.zeros(1 + nl, dtype=torch.float32, device=t1.device),
                                     torch.zeros(nl, dtype=torch.int32, device=t1.device))
        ws, loss, n_active = self._pycda_bufs[key]
        ops.upsample_pycda(t1, t2, soft, self.pycda_sizes, thresh=self.pycda_thresh, weight=self.pycda_weight, g1=g1, g2=g2,
                           accumulate=True, flag=self.pycda_flag, loss=loss, n_active=n_active, ws=ws)
        self.loss_pycda, self.pycda_active = loss, n_active

    def pycda_flag_value(self):
        """Deferred check of the pyramid term's flag word (host sync): bit 0 = a soft-label value outside [0, 1]."""
        return 0 if self.pycda_flag is None else int(self.pycda_flag.item())

    def _step(self, images_s, label_s, images_t, soft_t, regs_t):
        m = self.model
        if not m.training:
            m.train()
        self._mark('step start')
        m._maybe_sync()
        # source and target batch go through the network TOGETHER (twice the GEMM rows per launch), as two
        # BatchNorm groups: statistics, running-stat updates and gradients stay per domain like the
        # reference's two separate forward calls (train_ssl_reg.py:210-212)
        nb = images_s.shape[0]
        T = m.new_tape(groups=2)
        main = torch.cuda.current_stream()
        online = soft_t is None
        teacher_on_side = online and self.wgrad_stream is not None
        if online:
            # the teacher sees the BatchNorm running statistics as they stand at the START of the step (a snapshot on
            # the main stream, before the student's forward rewrites them) -- the same view whether its forward then
            # runs next to the student's on the second stream or after it
            self.teacher.adopt_buffers(m)
        # style, then mix, then strong: the mix below pastes the stylised source pixels; the teacher sees the clean images_t
        # (ahead of the teacher's launch or behind it: the step time was the same)
        images_s = self._style_source(images_s, images_t)
        if teacher_on_side:
            # the EMA teacher's forward is independent of the student's: it runs on the second stream, next to it
            plan.wait_stream(self.wgrad_stream, main)
            with ops.use_stream(self.wgrad_stream):
                soft_t = self.teacher_probs(images_t, snapshot=False)
                self._mark('teacher forward done (side)', self.wgrad_stream)
                # the gradient buffer is cleared here, behind the teacher and next to the student's forward (nothing
                # writes it before the main stream has joined this one), instead of ahead of the student's first kernel
                ops.fill_zero(m.flat_g)
        else:
            ops.fill_zero(m.flat_g)
        student_t = images_t
        if self.mix is not None:
            # the teacher above reads the caller's images_t; the student gets the mixed tile, a buffer of the step's own
            images_s, label_s, mix_table, mix_mode = self._mix_draw(images_s, label_s)
            student_t = ops.domain_mix_table(images_s, label_s, mix_table, mix_mode, images_in=images_t.contiguous().float(),
                                             images_out=torch.empty(images_t.shape, dtype=torch.float32, device=images_t.device),
                                             class_num=self.C, ignore_label=self.ig, flag=self.mix_flag)[0]
        if self.strong is not None:
            # out of place: the mixed tile above, or the caller's images_t, is read; the student's tile is a new buffer
            n_t, _, h_t, w_t = images_t.shape
            student_t = ops.strong_augment(student_t.contiguous().float(), self._strong_draw(n_t, h_t, w_t, images_t.device),
                                           self.strong.mean, self.strong.std, flag=self.strong_flag)
        x1, x2, feat = m._forward_plan([images_s.contiguous().float(), student_t.contiguous().float()], T)
        self._mark('student forward done')
        s1, t1, s2, t2 = x1[:nb], x1[nb:], x2[:nb], x2[nb:]
        # d(loss) / d(logits) of both heads, source rows then target rows: the two loss kernels write their halves in place
        g1, g2 = torch.empty_like(x1), torch.empty_like(x2)
        feat_s, feat_t = feat[:nb], feat[nb:]
        if teacher_on_side:
            plan.wait_stream(main, self.wgrad_stream)
        elif online:
            soft_t = self.teacher_probs(images_t, snapshot=False)
        self.last_soft_t = soft_t
        self._mark('joined teacher')
        # ---- label path (a5-a8)
        def wait_prototypes():           # the previous step's cross-rank average of the prototypes (second stream)
            if self._proto_ready is not None:
                main.wait_event(self._proto_ready)
                self._proto_ready = None
        plan.host(wait_prototypes)
        # the source half of the label path (source loss, prototype update) is independent of the target chain
        # (refine -> select -> LRH -> target loss): with a second stream it runs there, next to the target chain
        side = self.wgrad_stream if self.source_side else None
        if side is not None:
            plan.wait_event(side, plan.record_event(main))
            with ops.use_stream(side):
                loss_s = self._source_loss(s1, s2, label_s, g1[:nb], g2[:nb])
        # pseudo_selection + LRH in ONE pass over the refined soft labels (rgda_pseudo_lrh: the selected label is never
        # written as an int64 tensor and read back) where the chain is the default one; tests that look at the selected
        # labels (keep_debug) and the other configurations take the two calls
        regs = (regs_t.squeeze(1) if regs_t.dim() == 4 else regs_t) if self.sam_refine else None
        fuse_lrh = (self.refine_label and self.sam_refine and not self.keep_debug and self.max_regions <= 65535
                    and (soft_t.shape[-1] * soft_t.shape[-2]) % 4 == 0)
        hard = None
        # GDPLoss(prototype_refine): the prototype weights of the final pseudo labels, from the prototypes as they stand
        # BEFORE this step's update_prototype.  label_refine's similarity map (the base of its workspace) is exactly that
        # and is reused; without label_refine the weights read the prototypes themselves, so the source half's prototype
        # update is released only behind them
        want_pw = self.loss_fn_t.kind == 'gdp' and self.loss_fn_t.prototype_refine
        sim = None
        if self.refine_label:
            soft, cm, *sim = ops.label_refine(feat_t, self.prototypes, t1, t2, soft_t, self.temp, return_ws=True,
                                              return_sim=want_pw)
            sim = sim[0] if sim else None
            if not fuse_lrh:
                hard = ops.pseudo_select(soft, self.top, self.low, self.ig, classmax_ws=cm, check=False)
        else:
            soft = soft_t
            hard = ops.pseudo_select(soft_t, self.top, self.low, self.ig, check=False)
        exchange_protos = self.reducer.active
        late_protos = want_pw and sim is None

        def source_prototypes():
            # update_prototype rewrites the prototypes label_refine (or the prototype weights) has just read
            plan.wait_event(side, plan.record_event(main))
            with ops.use_stream(side):
                self._proto_local(feat_s, label_s, exchange_protos)
            return plan.record_event(side)
        if side is not None and not late_protos:
            source_done = source_prototypes()
        if self.keep_debug:
            self.debug = dict(t1=t1, t2=t2, s1=s1, s2=s2, feat_t=feat_t, feat_s=feat_s, soft_in=soft_t, soft=soft,
                              hard_selected=hard, student_t=student_t)
            self._keep_source(images_s)
        if self.sam_refine:
            hard = self._lrh(regs, hard, (soft, cm) if fuse_lrh else None)
        if self.mix is not None:
            # the source labels go onto the FINAL pseudo labels: selection thresholds, label_refine and LRH have seen the
            # teacher's view of the clean tile only.  The refined soft label is pasted only where the target loss or the
            # pyramid term reads it, and never in the caller's tensor or last_soft_t (refine_label=False makes `soft` that tensor itself)
            paste_soft = self.loss_fn_t.kind in ('ups', 'uvem') or self.pycda_weight > 0.0
            if paste_soft and (soft is soft_t or self.keep_debug):
                clean, soft = soft, torch.empty(soft.shape, dtype=torch.float32, device=soft.device)
                plan.host(lambda dst=soft, src=clean: dst.copy_(src))       # a torch op: re-run at every replay
            if self.keep_debug:
                self.debug.update(hard_clean=hard)      # the pseudo labels of the clean tile, before the paste
                hard = hard.clone()
            ops.domain_mix_table(images_s, label_s, mix_table, mix_mode, label_t=hard, soft_t=soft if paste_soft else None,
                                 class_num=self.C, ignore_label=self.ig, flag=self.mix_flag)
            if self.keep_debug:
                self.debug.update(soft_loss=soft)
        proto_weight = None
        if want_pw:
            proto_weight = ops.proto_pixel_weight(None if sim is not None else feat_t, self.prototypes, hard, sim=sim,
                                                  ignore_label=self.ig)
        self.last_proto_weight = proto_weight
        if side is not None and late_protos:
            source_done = source_prototypes()
        if side is None:
            self._proto_local(feat_s, label_s, exchange_protos)
        if exchange_protos:
            # data-parallel ranks: the per-class feature sums and pixel counts of the rank's source batch are
            # all-reduced (sum) and every rank applies the same totals -- the prototypes of the concatenated GLOBAL batch
            # (alignment.py:300-327: sum feat 1[c] / (n_c + eps), old prototype kept iff the global n_c < 1), identical bits on
            # every rank, the reference exactly at world 1.  Nothing of THIS step reads the prototypes any more (label_refine
            # is done), so the 48 KB all-reduce -- pure latency -- and the apply run on the second stream next to backward;
            # the next step's label path waits for them
            pside = self.wgrad_stream if self.wgrad_stream is not None else main
            if pside is not main and side is None:
                plan.wait_event(pside, plan.record_event(main))
            def exchange_statistics():
                all_reduce_prototype_statistics(self.proto_stats, self.C, self.prototypes.shape[1], self.group, self.comm,
                                                world=self.world)
            with ops.use_stream(pside):
                plan.host(exchange_statistics)
                ops.proto_apply(self.prototypes, self.proto_stats, self.pdecay)
                plan.host(lambda: setattr(self, '_proto_ready', pside.record_event() if pside is not main else None))
        # ---- losses + d(loss)/d(logits)
        if side is None:
            loss_s = self._source_loss(s1, s2, label_s, g1[:nb], g2[:nb])
        loss_t = self._target_loss(t1, t2, hard, soft, g1[nb:], g2[nb:], proto_weight)
        self._target_regularisers(t1, t2, hard, g1[nb:], g2[nb:])
        self._target_pyramid(t1, t2, soft, g1[nb:], g2[nb:])
        self._overlap_term('t', self.overlap_weight_t, t1, t2, hard, g1[nb:], g2[nb:])
        if self.keep_debug:
            self.debug.update(g1_t=g1[nb:].clone(), g2_t=g2[nb:].clone())
        if side is not None:
            plan.wait_event(main, source_done)       # source loss, its logit gradients, the new prototypes
        if self.keep_debug:
            self.debug.update(g1_s=g1[:nb].clone(), g2_s=g2[:nb].clone())
        self._mark('label path + losses done')
        # from here on the step no longer reads its input tensors (images: stem im2col of student and teacher; labels,
        # soft labels and region maps: the label path and the losses): an input prefetcher may overwrite them
        self._inputs_done = plan.record_event(main)
        self._backward_and_update(T, main, g1, g2)
        self.last_hard = hard
        return loss_s, loss_t, self.gn

    def _mix_draw(self, images_s, label_s):
        """This batch's draw of `self.mix` on the device -> (images_s, label_s as the mixing kernels read them, the table
        int32 [N][8], the mode).  The draw and the launch that carries it (rgda_mix_write_table: values in the kernel
        arguments, nothing staged in host memory) are ONE host action, re-run at every replay of a recorded step; a batch
        whose coin says "no mix" writes the empty table, so the launch sequence never changes.  kind 'dacs': the host
        draws the classes' ranks and rgda_mix_select_classes chooses among the classes present in each label map."""
        mx = self.mix
        images_s, label_s = images_s.contiguous().float(), label_s.contiguous()
        n, _, h, w = images_s.shape
        dev = images_s.device
        dacs = mx.kind == 'dacs'
        table = torch.empty(n, ops.MIX_TABLE_COLS, dtype=torch.int32, device=dev)
        ranks = torch.empty(n, self.C, dtype=torch.uint8, device=dev) if dacs else None
        here = torch.cuda.current_stream()

        def draw():
            d = mx.draw_step(n, h, w)
            bits, box, host = 0, (0, 0, 0, 0), None
            if dacs:        # a rank of 255 never selects its class: the batch that is not mixed
                host = d[1] if d is not None else np.full((n, self.C), 255, np.uint8)
            elif d is not None and d[0] == 'classes':
                bits = ops.mix_class_bits(d[1], self.C)
            elif d is not None:
                box = d[1]
            self.last_mix = d
            with ops.use_stream(here):      # (a replay runs host actions with the library's stream set to the plan's)
                ops.mix_write_table(table, self.C, bits, box, ranks, host)
        plan.host(draw)
        if dacs:
            ops.mix_select_classes(label_s, ranks, table, ignore_label=self.ig, flag=self.mix_flag)
        self.last_mix_table = table
        return images_s, label_s, table, ops.MIX_BOX if mx.kind == 'box' else ops.MIX_CLASS

    def _strong_draw(self, n, h, w, dev):
        """This batch's table of `self.strong` on the device, f32 [n][8].  The draw and the launch that carries it
        (rgda_strong_write_table: values in the kernel arguments) are ONE host action, re-run at every replay of a
        recorded step, like `_mix_draw`."""
        table = torch.empty(n, ops.STRONG_TABLE_COLS, dtype=torch.float32, device=dev)
        here = torch.cuda.current_stream()

        def draw():
            self.last_strong = self.strong.draw(n)
            with ops.use_stream(here):      # (a replay runs host actions with the library's stream set to the plan's)
                ops.strong_write_table(table, self.last_strong, (h, w))
        plan.host(draw)
        return table

    def strong_flag_value(self):
        """Deferred check of the strong augmentation's flag word (host sync): a table row outside the served range."""
        return 0 if self.strong_flag is None else int(self.strong_flag.item())

    def mix_flag_value(self):
        """Deferred check of the mixing kernels' flag word (host sync): a source label that is neither a class nor the
        ignore label."""
        return 0 if self.mix_flag is None else int(self.mix_flag.item())

    @torch.no_grad()
    def teacher_probs(self, images_t, snapshot=True):
        """Eval-mode forward of the EMA teacher (Encoder.py:152-155 on the shadow weights; BatchNorm buffers = the
        student's, copied now unless the caller already took the snapshot)."""
        t = self.teacher
        if snapshot:
            t.adopt_buffers(self.model)
        # make_teacher() and every sgd_step keep flat_pb current; a write to the shadow from OUTSIDE the step (a resume
        # that copies into teacher.flat_p or its parameter views) bumps the tensor's version and forces a re-cast
        t.refresh_from_master(mirror_is_fresh=(t.flat_p._version == t._synced_version))
        t.eval()
        x1, x2, _ = t._forward_plan(images_t.contiguous().float(), None)
        return ops.teacher_probs(x1, x2, tuple(images_t.shape[-2:]))
