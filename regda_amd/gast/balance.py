"""CrossEntropy + ClassBalance -- mirror of regda/gast/balance.py:15-101 (the "CE + reweight" of the
SSL path).  The loss is evaluated by the fused bilinear-upsample + CE kernel (`rgda_upsample_ce`).
The losses of the --ls / --lt flags -- OhemCrossEntropy, FocalLoss, GHMLoss, UPSLoss, UVEMLoss (balance.py:104-216,
306-435) -- and loss_calc_uvem (:438-460) run on the fused upsample + loss kernels of `rgda_upsample_loss`; GDPLoss
(:218-303) on those of `rgda_upsample_gdp`."""
import torch
import torch.distributed as dist
import torch.nn as nn

from .. import ops
from ..checkpoint import check_tensor, copy_in_place, need, plain


def sync_class_counts(cnt, group=None, comm=None):
    """Data-parallel runs: the per-class pixel counts of one step are summed over the ranks before the
    frequency EMA, so every rank carries the SAME `freq` (and class weights) -- the statistic of the global batch.
    With one process this is the reference's single-GPU arithmetic unchanged."""
    if comm is not None:                    # a regda_amd.ddp.RcclComm: the library's own RCCL entry point (fp32 counts)
        if comm.world > 1:
            comm.all_reduce(cnt)
    elif dist.is_available() and dist.is_initialized() and dist.get_world_size(group) > 1:
        dist.all_reduce(cnt, op=dist.ReduceOp.SUM, group=group)
    return cnt


class ClassBalance(nn.Module):
    def __init__(self, class_num=7, ignore_label=-1, decay=0.99, temperature=0.5, process_group=None, comm=None):
        super().__init__()
        assert temperature > 0
        self.class_num, self.ignore_label = class_num, ignore_label
        self.process_group = process_group
        self.comm = comm            # regda_amd.ddp.RcclComm instead of torch.distributed
        self.decay, self.temperature, self.eps = decay, temperature, 1e-7
        self.freq = torch.ones([class_num], device='cuda').float() / class_num

    def ema_update(self, label):
        cnt = ops.class_count(label, self.class_num).float()          # per-class pixel counts
        cnt = sync_class_counts(cnt.contiguous(), self.process_group, self.comm)
        local = cnt / (cnt.sum() + self.eps)                           # balance.py:45-53
        self.freq = (1.0 - self.decay) * local + self.decay * self.freq

    def _get_class_wight(self):
        p = torch.softmax((1.0 - self.freq) / self.temperature, dim=0)
        return p / (p.max() + self.eps)

    def next_class_weight(self, label):
        """freq EMA update + class weights: what get_class_weight_4pixel (balance.py:27-35) does,
        returned per class (the kernel looks the pixel's class up)."""
        self.ema_update(label)
        return self._get_class_wight().detach()

    # training state (regda_amd/checkpoint.py): the frequency EMA travels in the module's state_dict() as extra state
    def get_extra_state(self):
        return {'freq': plain(self.freq)}

    def check_extra_state(self, state, entry='ClassBalance'):
        check_tensor(need(state, 'freq', entry), entry + '.freq', (self.class_num,))

    def set_extra_state(self, state):
        self.check_extra_state(state)
        # ema_update rebinds `freq` at every step, so no launch plan holds its address: assigned, not copied into
        self.freq = state['freq'].to(self.freq.device).float().clone()

    def __str__(self):
        f = self.freq.cpu().numpy()
        w = self._get_class_wight().cpu().numpy()
        return ('class frequency: ' + ', '.join(f'{v:.3f}' for v in f) +
                ';\tselect probability: ' + ', '.join(f'{v:.3f}' for v in w))


class _UpLoss(torch.autograd.Function):
    """Autograd wrapper of a fused loss launch: `launch(p1, p2)` -> (loss f32[1], g1, g2)."""
    @staticmethod
    def forward(ctx, p1, p2, launch):
        loss, g1, g2 = launch(p1, p2)
        ctx.save_for_backward(g1, g2)
        return loss.reshape(())

    @staticmethod
    def backward(ctx, go):
        g1, g2 = ctx.saved_tensors
        return g1 * go, g2 * go, None


class _FusedLoss(nn.Module):
    """Common surface of the --ls / --lt losses: the reference's per-prediction forward, and forward_multi for
    loss_calc(multi=True) (both heads in one launch sequence).  `launch` is the raw device call the fused steps use.
    Subclasses set `class_balancer` (None where the reference takes none) and `ignore_label` as instance attributes:
    a ClassBalance is an nn.Module, so a class-level default would shadow it."""
    kind = None

    def _params(self):
        return {}

    def launch(self, p1, p2, labels, soft=None, class_weight=None, g1=None, g2=None, heads=2, want_grad=True):
        return ops.upsample_loss(self.kind, p1, p2, labels, soft=soft, class_weight=class_weight,
                                 ignore_label=self.ignore_label, want_grad=want_grad, g1=g1, g2=g2, heads=heads,
                                 **self._params())

    def _weights(self, labels, heads):
        if self.class_balancer is None:
            return None
        # the balancer is EMA-updated once per head, as in the reference's per-head loss_fn calls
        ws = [self.class_balancer.next_class_weight(labels) for _ in range(heads)]
        return torch.stack(ws * 2 if heads == 1 else ws, 0)

    def _run(self, preds, labels, soft):
        labels = labels.long()
        heads = 2 if isinstance(preds, (list, tuple)) else 1
        p1, p2 = (preds[0], preds[1]) if heads == 2 else (preds, preds)
        cw = self._weights(labels, heads)
        if heads == 1:
            # one prediction: the kernel's two "heads" are the same call, the gradient is g1 + g2
            return _UpLoss.apply(p1, p2, lambda a, _b: self.launch(a, a, labels, soft, cw, heads=1))
        return _UpLoss.apply(p1, p2, lambda a, b: self.launch(a, b, labels, soft, cw))

    def forward(self, preds, labels):
        return self._run(preds, labels, None)

    def forward_multi(self, preds, labels):
        assert len(preds) == 2
        return self._run(tuple(preds), labels, None)


class CrossEntropy(_FusedLoss):
    """balance.py:88-101: the (class-weighted) CE, mean over ALL pixels (`rgda_upsample_ce`)."""
    kind = 'ce'

    def __init__(self, ignore_label=-1, class_balancer=None):
        super().__init__()
        self.ignore_label = ignore_label
        self.class_balancer = class_balancer

    def launch(self, p1, p2, labels, soft=None, class_weight=None, g1=None, g2=None, heads=2, want_grad=True):
        # `soft` and `heads` unused: CE reads no soft label, and one prediction arrives as p1 == p2
        return ops.upsample_ce(p1, p2, labels, self.ignore_label, class_weight, want_grad, g1, g2)


class OhemCrossEntropy(_FusedLoss):
    """balance.py:104-133: the mean of the per-pixel (class-weighted) CE above -log(thresh), or of the n_min = #valid / 5
    largest when fewer pass.  Of equal losses at the k-th place the lowest pixel index is kept."""
    kind = 'ohem'

    def __init__(self, ignore_label=-1, class_balancer=None, thresh=0.7):
        super().__init__()
        self.thresh = -torch.log(torch.tensor(thresh, dtype=torch.float))
        self.ignore_label = ignore_label
        self.class_balancer = class_balancer

    def _params(self):
        return dict(thresh=float(self.thresh))


class FocalLoss(_FusedLoss):
    """balance.py:136-158 with alpha=None, reduction='mean' (what --lt focal constructs)."""
    kind = 'focal'

    def __init__(self, alpha=None, gamma=2.0, reduction='mean', ignore_label=-1):
        super().__init__()
        if alpha is not None or reduction != 'mean':
            raise NotImplementedError('FocalLoss: only alpha=None, reduction="mean" (the --lt focal configuration)')
        self.alpha, self.gamma, self.reduction, self.ignore_label = alpha, gamma, reduction, ignore_label
        self.class_balancer = None

    def _params(self):
        return dict(gamma=float(self.gamma))


class GHMLoss(_FusedLoss):
    """balance.py:161-216.  acc_sum stays on the device and is updated in place (once per head), so a captured step
    advances it at every replay."""
    kind = 'ghm'

    def __init__(self, bins=30, momentum=0.0, ignore_label=-1, device='cuda'):
        super().__init__()
        if bins != 30:
            raise NotImplementedError('GHMLoss: bins=30 only (the --lt ghm configuration)')
        self.bins_num, self.momentum, self.ignore_label = bins, momentum, ignore_label
        self.class_balancer = None
        edges = [float(x) / bins for x in range(bins + 1)]
        edges[-1] = edges[-1] + 1e-3
        self.edges = torch.tensor(edges, dtype=torch.float32, device=device)
        self.acc_sum = torch.zeros(bins, device=device)

    def _params(self):
        return dict(acc_sum=self.acc_sum, momentum=float(self.momentum))

    def get_extra_state(self):
        return {'acc_sum': plain(self.acc_sum)}

    def check_extra_state(self, state, entry='GHMLoss'):
        check_tensor(need(state, 'acc_sum', entry), entry + '.acc_sum', (self.bins_num,))

    def set_extra_state(self, state):
        self.check_extra_state(state)
        copy_in_place(self.acc_sum, state['acc_sum'])      # in place: a recorded step holds the buffer's address

    def get_g_distribution(self):
        return self.acc_sum / (self.acc_sum.sum() + 1e-7)


class GDPLoss(_FusedLoss):
    """balance.py:218-303 (`rgda_upsample_gdp`).  The per-pixel weight is the mean of up to three terms: the
    gradient-density weight `bins_weight[bucketize(|p_y - 1|) - 1]`, with prototype_refine the prototype weight handed
    over by set_prototype_weight_4pixel (Aligner.get_prototype_weight_4pixel), with class_balance the ClassBalance weight
    of the pixel's label.  acc_sum and bins_weight stay on the device and are updated in place (acc_sum once per head),
    so a captured or recorded step advances them at every replay.

    `class_balancer` is the loss's own ClassBalance(class_num, ignore_label, 0.99, temp) when class_balance is on and None
    otherwise; a balancer passed in replaces it (a data-parallel run hands over one that carries its process group)."""
    kind = 'gdp'

    def __init__(self, bins=30, momentum=0.99, class_num=7, ignore_label=-1, class_balance=False, prototype_refine=False,
                 temp=0.5, class_balancer=None, device='cuda'):
        super().__init__()
        if bins != 30:
            raise NotImplementedError('GDPLoss: bins=30 only')
        self.bins_num, self.momentum, self.ignore_label = bins, momentum, ignore_label
        self.class_num, self.temp = class_num, temp
        self.class_balance, self.prototype_refine = class_balance, prototype_refine
        edges = [float(x) / bins for x in range(bins + 1)]
        edges[-1] = edges[-1] + 1e-3
        self.edges = torch.tensor(edges, dtype=torch.float32, device=device)
        self.acc_sum = torch.zeros(bins, device=device)
        self.bins_weight = torch.zeros(bins, device=device)
        self.weight_prototype = None
        self.class_balancer = None
        if class_balance:
            self.class_balancer = class_balancer if class_balancer is not None else ClassBalance(
                class_num=class_num, ignore_label=ignore_label, decay=0.99, temperature=temp)

    def get_extra_state(self):
        return {'acc_sum': plain(self.acc_sum), 'bins_weight': plain(self.bins_weight)}

    def check_extra_state(self, state, entry='GDPLoss'):
        for k in ('acc_sum', 'bins_weight'):
            check_tensor(need(state, k, entry), f'{entry}.{k}', (self.bins_num,))

    def set_extra_state(self, state):
        # the loss's balancer is a submodule: its frequencies travel under 'class_balancer._extra_state'
        self.check_extra_state(state)
        copy_in_place(self.acc_sum, state['acc_sum'])      # in place: a recorded step holds the buffers' addresses
        copy_in_place(self.bins_weight, state['bins_weight'])

    def set_prototype_weight_4pixel(self, weight_prototype):
        """The prototype weights of the NEXT forward call(s): f32, one per label pixel (any shape)."""
        self.weight_prototype = weight_prototype

    def _pixel_weight(self, labels):
        if not self.prototype_refine:
            return None
        w = self.weight_prototype
        if w is None:
            raise RuntimeError('GDPLoss(prototype_refine=True): call set_prototype_weight_4pixel(weights) before the loss '
                               '(Aligner.get_prototype_weight_4pixel gives them)')
        if w.numel() != labels.numel():
            raise ValueError(f'GDPLoss: {w.numel()} prototype weights for {labels.numel()} label pixels')
        return w.detach().reshape(-1).float().contiguous()

    def launch(self, p1, p2, labels, soft=None, class_weight=None, g1=None, g2=None, heads=2, want_grad=True,
               pixel_weight=None):
        # `soft` unused; pixel_weight: the fused steps pass theirs, the module path the one that was set
        if pixel_weight is None:
            pixel_weight = self._pixel_weight(labels)
        return ops.upsample_gdp(p1, p2, labels, self.acc_sum, self.bins_weight, pixel_weight=pixel_weight,
                                class_weight=class_weight, momentum=float(self.momentum),
                                ignore_label=self.ignore_label, want_grad=want_grad, g1=g1, g2=g2, heads=heads)

    def forward(self, preds, targets):
        return self._run(preds, targets, None)

    def get_g_distribution(self):
        """(acc_sum normalised, bins_weight, the balancer's report) as balance.py:302-303; without class_balance the
        report is that of the reference's idle balancer (uniform frequencies)."""
        bal = self.class_balancer
        if bal is None:
            bal = ClassBalance(class_num=self.class_num, ignore_label=self.ignore_label, decay=0.99, temperature=self.temp)
        return self.acc_sum / (self.acc_sum.sum() + 1e-7), self.bins_weight, str(bal)


class UPSLoss(_FusedLoss):
    """balance.py:306-345: CE where the soft label's entropy u <= threshold, / #(u <= threshold, valid)."""
    kind = 'ups'

    def __init__(self, threshold=0.7, class_balancer=None, class_num=7, ignore_label=-1):
        super().__init__()
        self.threshold, self.class_balancer = threshold, class_balancer
        self.class_num, self.ignore_label = class_num, ignore_label

    def _params(self):
        return dict(t=float(self.threshold))

    def forward(self, preds, targets, label_t_soft):
        return self._run(preds, targets, label_t_soft)

    def forward_multi(self, preds, targets, label_t_soft):
        assert len(preds) == 2
        return self._run(tuple(preds), targets, label_t_soft)


class UVEMLoss(UPSLoss):
    """balance.py:348-426: UPSLoss times the uncertainty weight get_weight(u)."""
    kind = 'uvem'

    def __init__(self, m=0.1, threshold=0.7, gamma=8.0, class_balancer=None, class_num=7, ignore_label=-1):
        super().__init__(threshold, class_balancer, class_num, ignore_label)
        self.m, self.gamma = m, gamma

    def _params(self):
        return dict(m=float(self.m), t=float(self.threshold), gamma=float(self.gamma))

    def get_weight(self, uncertainties):
        """The weight curve (balance.py:398-426) on a tensor of uncertainties, for inspection and plotting: the training
        path evaluates it inside the fused kernel."""
        u = uncertainties
        left = torch.ones_like(u)
        if self.m > 0:
            x = torch.where((u <= self.m) & (u >= 0), u, left)
            left = torch.clamp((-1 / (self.m ** 2)) * (x - self.m) ** 2 + 1, 0.0, 1.0) ** (1.0 / self.gamma)
        right = torch.zeros_like(u)
        if self.m < self.threshold:
            x = torch.where((u > self.m) & (u <= self.threshold), u, right)
            right = torch.clamp((-1 / ((self.threshold - self.m) ** 2)) * (x - self.m) ** 2 + 1, 0.0, 1.0) ** (1.0 / self.gamma)
        w = torch.where(u <= self.m, left, right)
        return torch.where(u >= self.threshold, torch.zeros_like(u), w)


def loss_calc_uvem(pred, label, label_soft, loss_fn, multi=True):
    """balance.py:438-460: loss_calc for the losses that also read the (full-resolution) soft label."""
    if multi is True:
        if hasattr(loss_fn, 'forward_multi') and len(pred) == 2:
            return loss_fn.forward_multi(pred, label.long(), label_soft)
        loss = 0
        for p in pred:
            loss += loss_fn(p, label.long(), label_soft)
        return loss / len(pred)
    return loss_fn(pred, label.long(), label_soft)


SOURCE_LOSSES = ('CrossEntropy', 'OhemCrossEntropy')
TARGET_LOSSES = ('ours', 'uvem', 'ohem', 'focal', 'ghm', 'ups', 'gdp', 'none')


def source_loss(ls, class_balancer=None, ignore_label=-1):
    """--ls with --bcs (tools/train_ssl_reg.py:134, train_src.py:93, train_align_reg.py:126): the balancer is honoured by
    both choices."""
    if ls not in SOURCE_LOSSES:
        raise ValueError(f'--ls {ls!r}: one of {SOURCE_LOSSES}')
    cls = CrossEntropy if ls == 'CrossEntropy' else OhemCrossEntropy
    return cls(ignore_label=ignore_label, class_balancer=class_balancer)


def target_loss(lt, class_balancer=None, uvem_m=0.2, uvem_t=0.7, uvem_g=4.0, class_num=6, ignore_label=-1,
                device='cuda', gdp_prototype=False, gdp_class_balance=False, gdp_momentum=0.99, gdp_temp=0.5):
    """--lt with --bct and --uvem-m/-t/-g, exactly as tools/train_ssl_reg.py:135-158: ours / uvem and ups honour the
    balancer, ohem, focal and ghm are built without one, none is CrossEntropy (with it).  'gdp' (no flag of the
    reference's scripts constructs it) is GDPLoss with the gdp_* options; with gdp_class_balance a `class_balancer`
    given here replaces the loss's internal one."""
    if lt not in TARGET_LOSSES:
        raise ValueError(f'--lt {lt!r}: one of {TARGET_LOSSES}')
    if lt in ('ours', 'uvem'):
        return UVEMLoss(m=uvem_m, threshold=uvem_t, gamma=uvem_g, class_balancer=class_balancer, class_num=class_num,
                        ignore_label=ignore_label)
    if lt == 'ohem':
        return OhemCrossEntropy(ignore_label=ignore_label)
    if lt == 'focal':
        return FocalLoss(gamma=2.0, reduction='mean', ignore_label=ignore_label)
    if lt == 'ghm':
        return GHMLoss(bins=30, momentum=0.99, ignore_label=ignore_label, device=device)
    if lt == 'ups':
        return UPSLoss(threshold=0.7, class_balancer=class_balancer, class_num=class_num, ignore_label=ignore_label)
    if lt == 'gdp':
        return GDPLoss(bins=30, momentum=gdp_momentum, class_num=class_num, ignore_label=ignore_label,
                       class_balance=gdp_class_balance, prototype_refine=gdp_prototype, temp=gdp_temp,
                       class_balancer=class_balancer if gdp_class_balance else None, device=device)
    return CrossEntropy(ignore_label=ignore_label, class_balancer=class_balancer)
