"""Output-space adversarial alignment -- AdaptSegNet's recipe (Tsai et al., CVPR 2018) on FCDiscriminator
(regda/models/Discriminator.py:4-28): one discriminator per segmentation head reads softmax(upsample(logits)); the
segmentation network is pushed to make target outputs look like source outputs, the discriminators to tell them apart.
Domain labels 0 (source) / 1 (target), the discriminator loss halved, Adam with betas (0.9, 0.99) and lr 1e-4, as there.

The reference ships the discriminator class but no loop that trains it (tools/ never constructs it), so this is an
extension like the library's other alignment terms.  Everything on the hot path is a kernel of csrc/adv_kernels.hip; the
optimizer is torch.optim (ten small tensors per discriminator).  Nothing here synchronises with the host.

    generator_term(logits_t, grads_t, weights, size)
        per head i with a discriminator: z = D_i(P(logits_t[i])), loss += weights[i] * BCE(z, source_label), and the
        gradient with respect to the logits -- through the discriminator's data gradients only, no weight gradients --
        is ADDED onto grads_t[i] (f32, the logits' shape).  Returns the summed loss, a device tensor.
    discriminator_step(logits_s, logits_t, size)
        per head: 0.5 * (BCE(D(P_s), source_label) + BCE(D(P_t), target_label)) on detached inputs, weight and bias
        gradients into .grad, one optimizer step, the bf16 operand copies rebuilt.  The target forward of the generator
        term is reused when it was made from the same logits tensor, unwritten since (its _version), and the same operand
        copies: then neither the input nor the weights have moved in between.
"""
import torch

from .. import ops
from ..checkpoint import check_module_state, need, plain
from ..models.Discriminator import backward_rows, forward_rows


class AdversarialAligner:
    def __init__(self, discriminators, optimizer=None, lr=1e-4, betas=(0.9, 0.99), source_label=0, target_label=1):
        self.discriminators = list(discriminators)
        live = [d for d in self.discriminators if d is not None]
        if not live:
            raise ValueError('AdversarialAligner: no discriminator given')
        if {float(source_label), float(target_label)} != {0.0, 1.0}:
            raise ValueError('AdversarialAligner: the domain labels are 0 and 1')
        self.source_label, self.target_label = float(source_label), float(target_label)
        params = [p for d in live for p in d.parameters()]
        self.optimizer = optimizer if optimizer is not None else torch.optim.Adam(params, lr=lr, betas=betas)
        dev = params[0].device
        self.loss_adv = torch.zeros(1, device=dev)
        self.loss_disc = torch.zeros(1, device=dev)
        # per head, from the generator term: (logits tensor, its _version, operands, z, activations)
        self._target = [None] * len(self.discriminators)

    def check_served(self, b, C, size):
        """ValueError before anything is launched where a discriminator does not serve (b, C, H, W) inputs"""
        for d in self.discriminators:
            if d is not None:
                d.check_served((b, C, size[0], size[1]), 'AdversarialAligner')

    # training state (regda_amd/checkpoint.py)
    def state_dict(self):
        """{'discriminators': [state_dict() or None per head], 'optimizer': the optimizer's state_dict()}, plain data"""
        torch.cuda.synchronize()
        return plain({'discriminators': [None if d is None else d.state_dict() for d in self.discriminators],
                      'optimizer': self.optimizer.state_dict()})

    def check_state_dict(self, sd, strict=True, entry='AdversarialAligner'):
        """ValueError naming the entry where load_state_dict would not take `sd`; writes nothing"""
        ds = need(sd, 'discriminators', entry)
        if not isinstance(ds, list) or len(ds) != len(self.discriminators):
            raise ValueError(f"state entry '{entry}.discriminators': expected a list of {len(self.discriminators)}")
        for i, (d, s) in enumerate(zip(self.discriminators, ds)):
            if (d is None) != (s is None):
                raise ValueError(f"state entry '{entry}.discriminators[{i}]': the state has "
                                 f"{'none' if s is None else 'one'}, this object has {'none' if d is None else 'one'}")
            if d is not None:
                check_module_state(d, s, f'{entry}.discriminators[{i}]', strict)
        opt = need(sd, 'optimizer', entry)
        groups, own = need(opt, 'param_groups', entry + '.optimizer'), self.optimizer.state_dict()['param_groups']
        need(opt, 'state', entry + '.optimizer')
        if not isinstance(groups, list) or [len(g['params']) for g in groups] != [len(g['params']) for g in own]:
            raise ValueError(f"state entry '{entry}.optimizer.param_groups': the parameter groups differ from this optimizer's")

    def load_state_dict(self, sd, strict=True):
        """Validates first, then loads the discriminators (in place), the optimizer's moments, and rebuilds the bf16
        operand copies.  Nothing of the generator term's cached forward survives."""
        self.check_state_dict(sd, strict)
        torch.cuda.synchronize()
        for d, s in zip(self.discriminators, sd['discriminators']):
            if d is not None:
                d.load_state_dict(s, strict=strict)
        self.optimizer.load_state_dict(sd['optimizer'])
        self._target = [None] * len(self.discriminators)
        for d in self.discriminators:
            if d is not None:
                d.operands()

    def _forward(self, d, x, size):
        b, C = x.shape[:2]
        d.check_served((b, C, size[0], size[1]), 'AdversarialAligner')
        P = ops.adv_probs(x, size)
        return forward_rows(d.operands(), P, b, size[0], size[1])

    def generator_term(self, logits_t, grads_t, weights, size):
        self.loss_adv.zero_()
        for i, d in enumerate(self.discriminators):
            self._target[i] = None
            if d is None or not weights[i]:
                continue
            x, g = logits_t[i].detach(), grads_t[i]
            assert g.shape == x.shape and g.dtype == torch.float32 and g.is_contiguous() and x.is_contiguous()
            z, acts = self._forward(d, x, size)
            _, dz = ops.bce_logits(z, self.source_label, scale=float(weights[i]), loss=self.loss_adv, accumulate=True)
            dP, _ = backward_rows(d.operands(), dz, acts, x.shape[0], size[0], size[1], need_dparams=False)
            ops.adv_probs_backward(dP, x, g, size)
            # valid while neither the logits nor the discriminator's operand copies (rebuilt when a parameter moves) change
            self._target[i] = (logits_t[i], logits_t[i]._version, d.operands(), z, acts)
        return self.loss_adv

    def discriminator_step(self, logits_s, logits_t, size):
        self.loss_disc.zero_()
        self.optimizer.zero_grad(set_to_none=True)
        for i, d in enumerate(self.discriminators):
            if d is None:
                continue
            op, total = d.operands(), None
            for x, label, cached in ((logits_s[i], self.source_label, None), (logits_t[i], self.target_label, self._target[i])):
                x = x.detach()
                if cached is not None and cached[0] is logits_t[i] and cached[1] == logits_t[i]._version and cached[2] is op:
                    z, acts = cached[3], cached[4]
                else:
                    z, acts = self._forward(d, x, size)
                _, dz = ops.bce_logits(z, label, scale=0.5, loss=self.loss_disc, accumulate=True)
                _, grads = backward_rows(op, dz, acts, x.shape[0], size[0], size[1], need_dparams=True, need_dinput=False)
                total = grads if total is None else {k: total[k] + v for k, v in grads.items()}
            for k in d.PARAMS:
                d.get_parameter(k).grad = total[k]
            self._target[i] = None
        self.optimizer.step()
        for d in self.discriminators:
            if d is not None:
                d.operands()                    # the parameters moved: rebuild the bf16 copies now
        return self.loss_disc
