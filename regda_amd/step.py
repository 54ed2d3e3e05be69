"""What the three fused training steps share:

    FusedStep               the model, the optimizer tail, the gradient exchange, the source loss, the training state,
                            style= (the style transfer of the source tile: Fourier, or histogram matching)
      +-- SourceStep        stage 1 (regda_amd/source.py)
      +-- PseudoLabelStep   + prototypes, the selection thresholds, LRH
            +-- SSLStep     the self-training step: teacher, target loss, mix / strong, plans and graphs (regda_amd/ssl.py)
            +-- AlignStep   stage 2: PCL and the table of optional terms (regda_amd/align.py)"""
import copy
from collections import namedtuple

import torch

from . import ops
from . import plan
from .checkpoint import (FORMAT, check_equal, check_format, check_module_state, check_tensor, copy_in_place, need,
                         plain)
from .ddp import FlatGradReducer
from .gast.balance import source_loss


# One named part of a step's state: an object with state_dict() / load_state_dict(saved, strict=), or None; an empty state
# (a loss without statistics) counts as absent.  check(obj, saved, entry, strict) raises ValueError and writes nothing; None:
# the object's own check_state_dict (the aligners).  after(saved): owed behind the load.  hint: what decides the step has one
Part = namedtuple('Part', 'name obj check after hint', defaults=(None, None, ''))


def check_generator(obj, saved, entry, strict):     # the host generators (DomainMix, StrongAugment, the styles): load a copy
    try:
        copy.deepcopy(obj).load_state_dict(saved)
    except ValueError as e:
        raise ValueError(f'state entry {entry!r}: {e}') from None


class FusedStep:
    teacher = None      # the EMA shadow is an optional operand of the optimizer tail: SSLStep makes one

    def __init__(self, model, class_num=6, ignore_label=-1, momentum=0.9, weight_decay=5e-4, max_norm=32.0,
                 bucket_elems=12 << 20, process_group=None, overlap_wgrad=True, overlap_comm=True, class_balancer_s=None,
                 grad_payload='fp32', comm=None, loss_s='CrossEntropy', style=None, overlap_weight_s=0.0, overlap=None):
        ops.check_class_count(class_num, type(self).__name__)
        # The region-overlap term (Dice by default; regda_amd/gast/overlap.py) on the source logits and
        # the true labels: one rgda_upsample_overlap call behind the source loss that adds its gradient onto that loss's.
        # overlap: a dict of alpha, beta, gamma, smooth, read at every step.  Weight 0: no launch.  Checked before the model
        # is touched.
        self.overlap_weight_s = self._overlap_weight(overlap_weight_s, 'overlap_weight_s')
        self.overlap = self._overlap_dict(overlap)
        self.model = model
        self.C, self.ig = class_num, ignore_label
        self._shape_ok = None
        self.momentum, self.wd, self.max_norm = momentum, weight_decay, max_norm
        dev = model.device
        self.mom = torch.zeros_like(model.flat_p)
        self.lr_dev = torch.zeros(1, device=dev)
        self.gn = torch.zeros(1, device=dev)
        self.gn_ws = torch.zeros(1024, device=dev)
        self.first = True
        bounds = model.param_boundaries()
        # grad_payload: 'fp32' = bucketed all-reduce of the fp32 gradient; 'bf16' = all-to-all + fp32 accumulation +
        # all-gather of bf16 payloads, half the bytes on every link (regda_amd/ddp.py)
        # comm: a regda_amd.ddp.RcclComm -- the gradient buckets and the prototype statistics then go through the library's
        # own RCCL entry points (rgda_comm_*) instead of torch.distributed
        self.comm = comm
        self.reducer = FlatGradReducer(model.flat_g, bounds, bucket_elems, process_group, payload=grad_payload, comm=comm)
        self.measure_comm = False   # bench: HIP events around the main stream's wait for the gradient exchange
        self.comm_events = self.bwd_start_event = None
        self.wgrad_stream = torch.cuda.Stream(device=dev) if overlap_wgrad else None
        # --bcs of tools/train_ssl_reg.py:54-58,125-158: a regda_amd.gast.balance.ClassBalance whose frequency EMA
        # re-weights the source cross-entropy per class (None = plain CE, the default)
        self.class_balancer_s = class_balancer_s
        # --ls of tools/train_ssl_reg.py:52-63,134-158: a regda_amd.gast.balance loss whose fused kernel (rgda_upsample_ce /
        # rgda_upsample_loss) the step launches directly
        self.loss_fn_s = source_loss(loss_s, class_balancer_s, ignore_label)
        self.marks = None           # set to [] to collect (name, event) phase marks of the next step (bench --phases)
        self.overlap_comm = overlap_comm
        self.keep_debug = False     # tests: keep intermediate tensors of the step (`self.debug`)
        self.debug = None
        self.world, self.group = self.reducer.world, process_group
        # style: a regda_amd.aug.fourier.FourierStyle -- Fourier style transfer of the source tile ahead of the forward
        # (DESIGN.md 4.2j): the low-frequency amplitudes of each source image become those of a target image of the batch
        # -- or a regda_amd.aug.histogram.HistogramStyle: its grey-level distribution becomes the target image's.
        # The caller's tensors are never written, the result is a buffer of the step's own.  None: no launch.
        self.style = style
        self.style_flag = torch.zeros(1, dtype=torch.int32, device=dev) if style is not None else None
        self.last_style = None      # the last step's table as drawn on the host, int32 (N, 4)
        self._style_ws = None       # (shape, the transform's workspace): kept from step to step, like the flag word
        # the overlap term's outputs of the last step (device tensors; None while the weight is 0): the unscaled loss f32
        # [1], the per-class soft overlap index f32 [2, C], the classes' pixel counts int32 [C]; _t: the SSL step's target side
        self.loss_overlap_s = self.overlap_index_s = self.overlap_present_s = None
        self.loss_overlap_t = self.overlap_index_t = self.overlap_present_t = None
        self.overlap_flag = None    # bit 0: a label outside [0, C) that is not ignore_label (made at the first launch)
        self._overlap_bufs = {}     # (side, shapes) -> (workspace, loss, index, present): allocated once

    def _overlap_weight(self, v, name):
        v = float(v)
        if not (v >= 0.0 and v != float('inf')):
            raise ValueError(f'{type(self).__name__}: {name} must be finite and >= 0, got {v!r}')
        return v

    def _overlap_dict(self, d):
        d = dict(d or {})
        if set(d) - {'alpha', 'beta', 'gamma', 'smooth'}:
            raise ValueError(f"{type(self).__name__}: overlap= takes alpha, beta, gamma, smooth; got {sorted(d)}")
        ops.overlap_params(**d, who=f'{type(self).__name__}(overlap=)')
        return d

    def _overlap_term(self, side, weight, x1, x2, label, g1, g2):
        """The overlap term of logits x1, x2 against `label`: its gradient, times `weight`, is added onto g1, g2 (one
        launch sequence on the current stream, nothing read back) and its outputs become loss_overlap_<side>,
        overlap_index_<side>, overlap_present_<side>.  The sums run over this rank's batch: ranks of a data-parallel
        run use their local sums, like every other loss of the step."""
        if not weight > 0.0:
            return
        prm = ops.overlap_params(**self.overlap, who=f'{type(self).__name__}.overlap')
        key = (side, tuple(x1.shape), tuple(label.shape))
        if key not in self._overlap_bufs:
            dev = x1.device
            self._overlap_bufs[key] = (ops.upsample_overlap_workspace(x1, label.shape),
                                       torch.zeros(1, dtype=torch.float32, device=dev),
                                       torch.zeros(2, x1.shape[1], dtype=torch.float32, device=dev),
                                       torch.zeros(x1.shape[1], dtype=torch.int32, device=dev))
        if self.overlap_flag is None:
            self.overlap_flag = torch.zeros(1, dtype=torch.int32, device=x1.device)
        ws, loss, index, present = self._overlap_bufs[key]
        ops.upsample_overlap(x1, x2, label, *prm, weight=weight, ignore_label=self.ig, g1=g1, g2=g2, accumulate=True,
                             loss=loss, index=index, present=present, flag=self.overlap_flag, ws=ws)
        setattr(self, 'loss_overlap_' + side, loss)
        setattr(self, 'overlap_index_' + side, index)
        setattr(self, 'overlap_present_' + side, present)

    def overlap_flag_value(self):
        """Deferred check of the overlap term's flag word (host sync): bit 0 = a label outside [0, C)."""
        return 0 if self.overlap_flag is None else int(self.overlap_flag.item())

    def _style_source(self, images_s, images_t):
        """The source tile the network sees: `images_s` itself without `style=`, else its style transfer (Fourier, or
        histogram matching) towards this batch's target tiles, out of place.  The style object brings the three calls:
        workspace, write_table and apply.  The draw and the launch that carries it (rgda_*_style_write_table: values in the
        kernel arguments) are ONE host action, re-run at every replay of a recorded step."""
        st = self.style
        if st is None:
            return images_s
        if images_t is None:
            raise ValueError(f'{type(self).__name__}(style=) needs the target images')
        if images_s.dim() != 4 or images_t.dim() != 4 or tuple(images_s.shape[1:]) != tuple(images_t.shape[1:]):
            raise ValueError(f'{type(self).__name__}(style=): source and target tiles must have one size, got '
                             f'{tuple(images_s.shape)} and {tuple(images_t.shape)}')
        images_s = images_s.contiguous().float()
        n, _, h, w = images_s.shape
        m = images_t.shape[0]
        table = torch.empty(n, ops.STYLE_TABLE_COLS, dtype=torch.int32, device=images_s.device)
        if self._style_ws is None or self._style_ws[0] != (n, m, h, w):
            self._style_ws = ((n, m, h, w), st.workspace(n, m, h, w, images_s.device))
        here = torch.cuda.current_stream()

        def draw():
            self.last_style = st.draw(n, m, h, w)
            with ops.use_stream(here):      # (a replay runs host actions with the library's stream set to the plan's)
                st.write_table(table, self.last_style, m, (h, w))
        plan.host(draw)
        return st.apply(images_s, images_t.contiguous().float(), table, ws=self._style_ws[1], flag=self.style_flag)

    def _keep_source(self, source_s):
        """keep_debug: the source tile as the network saw it, next to whatever the step kept"""
        if self.keep_debug and self.style is not None:
            self.debug = dict(self.debug or {}, source_s=source_s)

    def style_flag_value(self):
        """Deferred check of the style transfer's flag word (host sync): a table row outside the served range."""
        return 0 if self.style_flag is None else int(self.style_flag.item())

    @staticmethod
    def _refuse_ssl_only(kw):
        """`kw` without the keywords of the SSL step's own options; NotImplementedError where one is switched on (before
        the model is touched).  What is left goes to the base constructors: TypeError for a keyword they do not know."""
        ent, kld = kw.pop('ent_weight', 0.0), kw.pop('kld_weight', 0.0)
        if ent or kld:
            raise NotImplementedError('the IAST regularisers (ent_weight / kld_weight) belong to the SSL step')
        pycda = kw.pop('pycda_weight', 0.0)
        kw.pop('pycda_sizes', None), kw.pop('pycda_thresh', None)
        if pycda:
            raise NotImplementedError('the PyCDA region pyramid term (pycda_weight) belongs to the SSL step')
        if kw.pop('overlap_weight_t', 0.0):
            raise NotImplementedError('the overlap term on the target logits (overlap_weight_t) belongs to the SSL step; '
                                      'overlap_weight_s is served here')
        if kw.pop('mix', None) is not None:
            raise NotImplementedError('the in-step cross-domain mix (mix=) belongs to the SSL step')
        if kw.pop('strong', None) is not None:
            raise NotImplementedError('the strong augmentation of the student tile (strong=) belongs to the SSL step')
        if kw.pop('ema_decay', None) is not None:
            raise NotImplementedError('the EMA teacher (ema_decay=) belongs to the SSL step')
        return kw

    def _check_shape(self, *images, k=None):
        """ValueError before the first launch where a kernel of the step cannot serve these tiles (ops.check_step_shape);
        k: the channels of the prototypes, for the steps whose kernels read some (PseudoLabelStep)."""
        for x in images:
            if x is None or tuple(x.shape[-2:]) == self._shape_ok:
                continue
            ops.check_step_shape(self.C, k, x.shape[-2], x.shape[-1], type(self).__name__)
            self._shape_ok = tuple(x.shape[-2:])

    def capture(self, *a, **k):
        raise NotImplementedError('whole-step graph capture is provided for the SSL step only')

    def record_plan(self, *a, **k):
        raise NotImplementedError('plan replay is provided for the SSL step only (the other steps have host actions that '
                                  'are not marked for recording)')

    def _forward_domains(self, *images):
        """How the stage-1 and stage-2 steps open: train mode, weights in sync, gradient cleared, a new tape, and ONE
        forward of the given domains as that many BatchNorm groups -> (tape, main stream, x1, x2, feat)."""
        m = self.model
        if not m.training:
            m.train()
        m._maybe_sync()
        ops.fill_zero(m.flat_g)
        T = m.new_tape(groups=len(images))
        xs = [x.contiguous().float() for x in images]
        return (T, torch.cuda.current_stream(), *m._forward_plan(xs if len(xs) > 1 else xs[0], T))

    def _class_weights(self, balancer, label):
        """Per-class CE weights of the two heads [2, C] (or None): loss_calc(multi=True) calls the loss once per head
        and every call EMA-updates the balancer (regda/gast/balance.py:27-35), so the heads see consecutive states.
        A host action of a recorded step: the counts and the 6-element arithmetic are re-run at every replay."""
        if balancer is None:
            return None
        cw = torch.empty(2, self.C, device=label.device)
        here = torch.cuda.current_stream()

        def update():
            # a replay runs this on `here` as torch's stream, but with the library's stream set to the plan's: the count
            # kernel and the torch arithmetic on its result must share one (the source side runs on the second stream)
            with ops.use_stream(here):
                for hd in range(2):
                    cw[hd].copy_(balancer.next_class_weight(label))
        plan.host(update)
        return cw

    def _host_balancers(self):
        """Whether a ClassBalance takes part in the step's losses"""
        return self.loss_fn_s.class_balancer is not None

    def _source_loss(self, s1, s2, label_s, g1, g2):
        """loss_calc(source, loss_fn_s): its value; d loss / d logits written into g1, g2.  With overlap_weight_s the
        overlap term against the true labels follows on the same stream and adds its gradient onto them; the value
        returned stays the plain loss."""
        f = self.loss_fn_s
        loss = f.launch(s1, s2, label_s, class_weight=self._class_weights(f.class_balancer, label_s), g1=g1, g2=g2)[0]
        self._overlap_term('s', self.overlap_weight_s, s1, s2, label_s, g1, g2)
        return loss

    def _mark(self, name, stream=None):
        if self.marks is not None:
            ev = torch.cuda.Event(enable_timing=True)
            ev.record(stream if stream is not None else torch.cuda.current_stream())
            self.marks.append((name, ev))

    def _backward_and_update(self, T, main, g1, g2, gfeat=None):
        """Backward (both domains in one pass; all-reduce buckets are released as it moves down the net), then clip +
        SGD (+ EMA) in one pass over the flat buffers."""
        m = self.model
        plan.host(self.reducer.reset)
        if self.measure_comm and self.reducer.active:
            def mark_backward_start():
                self.reducer.measure = True
                self.bwd_start_event = torch.cuda.Event(enable_timing=True)
                self.bwd_start_event.record()
            plan.host(mark_backward_start)
        T.update(wgrad_stream=self.wgrad_stream, main_stream=main, mark=self._mark if self.marks is not None else None)

        def progress(offset):
            if (self.world > 1 or self.reducer.force) and self.overlap_comm:
                if self.wgrad_stream is not None:
                    # a bucket needs the weight gradients (second stream) AND the BN gradients (main stream) of its
                    # layers: issue it from the second stream once that has caught up with this point of the main
                    # stream, so the critical path never waits for communication
                    plan.wait_event(self.wgrad_stream, plan.record_event(main))
                    with ops.use_stream(self.wgrad_stream):
                        plan.host(lambda: self.reducer.ready_down_to(offset))
                else:
                    plan.host(lambda: self.reducer.ready_down_to(offset))
        m._backward_plan(T, g1, g2, on_progress=progress, gfeat=gfeat)
        self._mark('backward done (streams joined)')
        def finish_exchange():
            # everything the main stream still has to wait for here is EXPOSED communication (the buckets were issued
            # while backward ran); with measure_comm the stall is bracketed by events (bench.py: comm_exposed_ms)
            if self.measure_comm and self.reducer.active:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                self.reducer.finish()
                e1.record()
                self.comm_events = (e0, e1)
            else:
                self.reducer.finish()
        plan.host(finish_exchange)
        # ---- clip + SGD (+ EMA) in one pass over the flat buffers
        ops.sumsq(m.flat_g, self.gn, self.gn_ws)
        shadow = self.teacher.flat_p if self.teacher is not None else None
        ops.sgd_step(m.flat_p, m.flat_g, self.mom, shadow, m.flat_pb, self.gn, self.lr_dev, self.momentum, self.wd,
                     self.max_norm, self.reducer.gscale, self.ema_decay if shadow is not None else 0.0, self.first,
                     shadow_bf16=self.teacher.flat_pb if shadow is not None else None)   # teacher mirror stays fresh
        self.first = False
        m.sync_derived_weights(self.wgrad_stream)
        m._synced_version = m.flat_p._version
        self._mark('optimizer + weight mirrors done')

    # ------------------------------------------------------------------ training state (regda_amd/checkpoint.py)
    # Each class declares what it owns, the walk below does the rest: the tensors loaded in place, the config a state must
    # agree on, the named parts, and the entries of earlier format-1 states for parts the class never had (ignored)
    _STATE_TENSORS = ('mom',)
    _STATE_CONFIG_FREE = ()     # config keys that are recorded and not compared
    _STATE_LEGACY = ()

    def _state_config(self):
        m = self.model
        return dict(class_num=self.C, ignore_label=self.ig, loss_s=self.loss_fn_s.kind,
                    model=dict(resnet_type=m.resnet_type, head_kind=m.head_kind, num_classes=m.num_classes,
                               n_param=m.flat_p.numel()))

    def _state_parts(self):
        return [Part('model', self.model, check_module_state),      # loaded in place; re-syncs the bf16 mirrors
                Part('class_balancer_s', self.class_balancer_s, check_module_state),
                Part('loss_fn_s', self.loss_fn_s, check_module_state), Part('style', self.style, check_generator)]

    def state_dict(self, rng=True):
        """Everything the run needs to continue with the bits of the uninterrupted one, as plain data (nested dicts and
        lists of CPU tensors, numbers, strings, None: torch.load(weights_only=True) reads a file of it): the optimizer's
        `first` flag, the class's tensors and named parts and, with `rng`, torch's CPU and device generator states (the
        Dropout2d seeds and the contrast term's draws come from the CPU one).  Not state: gradients, the learning rate
        word, the last_* / loss_* outputs, workspaces, plans, streams, and the parameter dicts the caller sets
        (step.contrast, ...).  Synchronises the device first: the end of a step leaves work on the side streams."""
        torch.cuda.synchronize()
        sd = dict(format=FORMAT, kind=type(self).__name__, config=self._state_config(), first=bool(self.first),
                  **{k: getattr(self, k) for k in self._STATE_TENSORS})
        states = {p.name: p.obj.state_dict() for p in self._state_parts() if p.obj is not None}
        sd.update({k: v for k, v in states.items() if v})       # a part without statistics writes no entry
        if rng:
            sd['rng'] = dict(cpu=torch.get_rng_state(), cuda=torch.cuda.get_rng_state(self.model.device))
        return plain(sd)

    def _state_loads(self, sd, strict):
        """Validate every entry of `sd` against this step (ValueError naming the entry; nothing is written here) and
        return the writes, in order, as closures for load_state_dict to run once ALL of them are known to be good."""
        check_format(sd, 'step')
        check_equal(need(sd, 'kind', 'step'), type(self).__name__, 'step.kind')
        cfg, own = need(sd, 'config', 'step'), self._state_config()
        for k in [k for k in own if k not in ('model', *self._STATE_CONFIG_FREE)]:
            check_equal(need(cfg, k, 'step.config'), own[k], 'step.config.' + k)
        for k, v in own['model'].items():
            check_equal(need(need(cfg, 'model', 'step.config'), k, 'step.config.model'), v, 'step.config.model.' + k)
        parts = self._state_parts()
        known = {'format', 'kind', 'config', 'first', 'rng', *self._STATE_TENSORS, *self._STATE_LEGACY, *(p.name for p in parts)}
        if strict and set(sd) - known:
            raise ValueError(f'state entries {sorted(set(sd) - known)} of the step are unknown to this {type(self).__name__}')
        take = lambda k: need(sd, k, 'step') if strict or k in sd else None     # strict=False: what is there
        loads = []
        for k in self._STATE_TENSORS:
            if take(k) is not None:
                dst = getattr(self, k)
                check_tensor(sd[k], 'step.' + k, dst.shape, dst.dtype)
                loads.append(lambda dst=dst, k=k: copy_in_place(dst, sd[k]))
        if take('first') is not None:
            if not isinstance(sd['first'], bool):
                raise ValueError(f"state entry 'step.first': expected a bool, got {sd['first']!r}")
            loads.append(lambda: setattr(self, 'first', sd['first']))
        for p in parts:
            has = p.obj is not None and bool(p.obj.state_dict())
            if (p.name in sd) != has and (strict or p.name in sd):
                raise ValueError(f"state entry 'step.{p.name}': the state has {'one' if p.name in sd else 'none'}, this step "
                                 f"has {'one' if has else 'none'}{p.hint}")
            if p.name in sd:
                if p.check is None:
                    p.obj.check_state_dict(sd[p.name], strict, 'step.' + p.name)
                else:
                    p.check(p.obj, sd[p.name], 'step.' + p.name, strict)
                loads.append(lambda p=p: p.obj.load_state_dict(sd[p.name], strict=strict))
                if p.after is not None:
                    loads.append(lambda p=p: p.after(sd[p.name]))
        if 'rng' in sd:
            cpu, cuda = (check_tensor(need(sd['rng'], k, 'step.rng'), 'step.rng.' + k, dtype=torch.uint8)
                         for k in ('cpu', 'cuda'))
            loads.append(lambda: (torch.set_rng_state(cpu), torch.cuda.set_rng_state(cuda, self.model.device)))
        return loads

    def load_state_dict(self, sd, strict=True):
        """Continue the run `sd` (a state_dict()) was taken from.  Every entry is validated before the first is written:
        a mismatch (format, step class, class count, loss kinds, tensor sizes, model fingerprint, a part the state has and
        the step has not or the reverse, missing keys) raises ValueError naming the entry and leaves the step untouched
        and usable.  Each tensor is copied into the storage the step already owns, so a recorded plan stays valid and
        replays the loaded state.  `first` is what was saved.  strict=False loads the entries and keys that are there."""
        loads = self._state_loads(sd, strict)
        torch.cuda.synchronize()        # the last step's tail is still writing weights and mirrors on the side streams
        for load in loads:
            load()
        torch.cuda.synchronize()


class PseudoLabelStep(FusedStep):
    """The steps that make pseudo labels from prototypes: label_refine's operands, the selection thresholds, LRH and the
    prototype update."""
    _STATE_TENSORS = FusedStep._STATE_TENSORS + ('prototypes',)

    def __init__(self, model, prototypes, cutoff_top=0.8, cutoff_low=0.6, percent=0.5, proto_decay=0.996, refine_temp=2.0,
                 sam_refine=True, refine_label=True, max_regions=4096, **kw):
        super().__init__(model, **kw)
        self.top, self.low, self.percent = cutoff_top, cutoff_low, percent
        self.pdecay, self.temp = proto_decay, refine_temp
        self.sam_refine, self.refine_label = sam_refine, refine_label
        self.max_regions = max_regions
        self.prototypes = prototypes.to(model.device).float().contiguous().clone()
        self.lrh_ws = self._proto_ready = None
        self.proto_stats = None     # data-parallel ranks: sums[c][k], cnt[c] of update_prototype (all-reduced per step)

    def _check_shape(self, *images):
        super()._check_shape(*images, k=self.prototypes.shape[-1])

    def _proto_local(self, feat_s, label_s, exchange):
        """update_prototype on this rank's source batch: the whole update (one rank), or its sufficient statistics only
        (data-parallel ranks: the caller all-reduces them and applies the totals).  Returns the downscaled source label."""
        if exchange:
            self.proto_stats, label_s_down = ops.proto_stats(feat_s, label_s, 16, self.ig, 0.75, self.C, stats=self.proto_stats)
            return label_s_down
        return ops.proto_update(feat_s, label_s, self.prototypes, 16, self.ig, 0.75, self.pdecay)

    def _lrh(self, regs, hard, fused=None):
        """Homogenizer (LRH) of the selected labels `hard` on the step's workspace, which keeps the flag word `lrh_flag()`
        reads.  fused = (soft, classmax): pseudo_selection + LRH in one pass instead (rgda_pseudo_lrh), `hard` unused."""
        self._lrh_flag_off = (regs.shape[0] * self.max_regions * (self.C + 1)) * 4
        if fused is not None:
            hard, self.lrh_ws = ops.pseudo_lrh(*fused, regs, self.top, self.low, self.percent, self.C, self.ig,
                                               self.max_regions, ws=self.lrh_ws)
            return hard
        need = self._lrh_flag_off + 16
        if self.lrh_ws is None or self.lrh_ws.numel() < need:
            self.lrh_ws = torch.empty(need, dtype=torch.uint8, device=self.model.device)
        return ops.lrh(hard, regs.contiguous(), self.percent, self.C, self.ig, self.max_regions, check=False, ws=self.lrh_ws)

    def lrh_flag(self):
        """Deferred check of the LRH kernel's flag word (host sync): region id / label range errors."""
        if self.lrh_ws is None:
            return 0
        o = self._lrh_flag_off
        return int(self.lrh_ws[o:o + 4].view(torch.int32).item())
