"""Category-level adversarial alignment -- CLAN (Luo et al., CVPR 2019) on the two-head Deeplabv2 and FCDiscriminator
(regda/models/Discriminator.py:4-28) with WeightedBCEWithLogitsLoss (regda/loss.py:60-85): ONE discriminator reads
softmax(up x1 + up x2); its output is upsampled to the tile, and the adversarial loss there is weighted per pixel by
epsilon + lambda_local * wmap, wmap = 1 - cos(softmax(up x1), softmax(up x2)) -- up where the two heads disagree, which is
where the classes are not aligned yet.

The reference ships the loss and the two-head network but no loop that uses them, so this is an extension like
regda_amd/gast/adversarial.py, whose discriminator, optimizer handling and saved state it shares.  The hot path is
csrc/clan_kernels.hip around the discriminator's kernels; nothing here synchronises with the host.

    generator_term((t1, t2), (g1_t, g2_t), weight, size)
        P, wmap = clan_probs(t1, t2); z = D(P); loss = weight * wBCE(up z, source_label, wmap, epsilon, lambda_local); the
        gradient -- through the discriminator's data gradients and, with weight_grad, through the weight map -- is ADDED onto
        g1_t and g2_t (f32, the logits' shape).  While steps_done < preheat_steps the loss is the plain BCE on the upsampled
        map and the weight map carries no gradient.  Returns the loss, a device tensor.
    discriminator_step((s1, s2), (t1, t2), size)
        0.5 * (BCE(up D(P_s), source_label) + wBCE(up D(P_t), target_label, wmap)) on detached inputs (plain BCE on both
        sides during the preheat), one optimizer step, the bf16 operand copies rebuilt, steps_done += 1.  The 0.5 keeps this
        aligner on the scale of AdversarialAligner's discriminator loss; CLAN's own script does not halve.  The target
        forward of the generator term is reused under AdversarialAligner's rule: the same logits tensors, unwritten since
        (their _version), the same operand copies.

epsilon, lambda_local, preheat_steps and weight_grad are attributes, read at every call."""
from .. import ops
from ..checkpoint import need
from ..models.Discriminator import backward_rows, forward_rows
from .adversarial import AdversarialAligner


class CategoryAdversarialAligner(AdversarialAligner):
    def __init__(self, discriminator, optimizer=None, lr=1e-4, betas=(0.9, 0.99), epsilon=0.4, lambda_local=40.0,
                 preheat_steps=0, weight_grad=True, source_label=0, target_label=1):
        if discriminator is None or isinstance(discriminator, (list, tuple)):
            raise ValueError('CategoryAdversarialAligner: exactly one discriminator, which reads softmax(x1 + x2)')
        self.check_hyper(epsilon, lambda_local, preheat_steps, 'CategoryAdversarialAligner')     # before anything is built
        super().__init__([discriminator], optimizer, lr, betas, source_label, target_label)
        self.set_hyper(epsilon, lambda_local, preheat_steps, weight_grad)
        self.steps_done = 0

    def set_hyper(self, epsilon, lambda_local, preheat_steps, weight_grad):
        """checked, then written: ValueError leaves the aligner as it was"""
        self.check_hyper(epsilon, lambda_local, preheat_steps, 'CategoryAdversarialAligner')
        self.epsilon, self.lambda_local, self.preheat_steps = float(epsilon), float(lambda_local), int(preheat_steps)
        self.weight_grad = bool(weight_grad)

    @staticmethod
    def check_hyper(epsilon, lambda_local, preheat_steps, entry):
        for name, v in (('epsilon', epsilon), ('lambda_local', lambda_local)):
            if isinstance(v, bool) or not isinstance(v, (int, float)) or not v == v or v < 0:
                raise ValueError(f'{entry}: {name} is a number >= 0, got {v!r}')
        if isinstance(preheat_steps, bool) or not isinstance(preheat_steps, int) or preheat_steps < 0:
            raise ValueError(f'{entry}: preheat_steps is an integer >= 0, got {preheat_steps!r}')

    @property
    def weighted(self):
        """past the preheat: the weight map acts"""
        return self.steps_done >= self.preheat_steps

    # training state: AdversarialAligner's, and under 'clan' the step counter the preheat goes by and the hyper-parameters
    def state_dict(self):
        sd = super().state_dict()
        sd['clan'] = dict(steps_done=int(self.steps_done), epsilon=self.epsilon, lambda_local=self.lambda_local,
                          preheat_steps=self.preheat_steps)
        return sd

    def check_state_dict(self, sd, strict=True, entry='CategoryAdversarialAligner'):
        super().check_state_dict(sd, strict, entry)
        c = need(sd, 'clan', entry)
        steps = need(c, 'steps_done', entry + '.clan')
        if isinstance(steps, bool) or not isinstance(steps, int) or steps < 0:
            raise ValueError(f"state entry '{entry}.clan.steps_done': an integer >= 0, got {steps!r}")
        self.check_hyper(need(c, 'epsilon', entry + '.clan'), need(c, 'lambda_local', entry + '.clan'),
                          need(c, 'preheat_steps', entry + '.clan'), f"state entry '{entry}.clan'")

    def load_state_dict(self, sd, strict=True):
        super().load_state_dict(sd, strict)         # validates all of it, this class's entry included, before it writes
        c = sd['clan']
        self.steps_done = int(c['steps_done'])
        self.set_hyper(c['epsilon'], c['lambda_local'], c['preheat_steps'], self.weight_grad)

    def _forward_pair(self, d, x1, x2, size):
        b, C = x1.shape[:2]
        d.check_served((b, C, size[0], size[1]), 'CategoryAdversarialAligner')
        P, wmap = ops.clan_probs(x1, x2, size)
        z, acts = forward_rows(d.operands(), P, b, size[0], size[1])
        return z.view(b, size[0] // 32, size[1] // 32), acts, wmap

    def generator_term(self, logits_t, grads_t, weight, size):
        self.loss_adv.zero_()
        self._target[0] = None
        if not weight:
            return self.loss_adv
        d = self.discriminators[0]
        (t1, t2), (g1, g2) = logits_t, grads_t
        x1, x2 = t1.detach(), t2.detach()
        z, acts, wmap = self._forward_pair(d, x1, x2, size)
        hot = self.weighted
        _, dz, gw = ops.wbce_logits(z, size, self.source_label, wmap if hot else None, self.epsilon, self.lambda_local,
                                    scale=float(weight), loss=self.loss_adv, accumulate=True,
                                    want_gw=hot and self.weight_grad)
        dP, _ = backward_rows(d.operands(), dz.view(x1.shape[0], -1), acts, x1.shape[0], size[0], size[1], need_dparams=False)
        ops.clan_probs_backward(dP, gw, x1, x2, g1, g2, size)
        # valid while neither head's logits nor the discriminator's operand copies change
        self._target[0] = ((t1, t2), (t1._version, t2._version), d.operands(), z, acts, wmap)
        return self.loss_adv

    def discriminator_step(self, logits_s, logits_t, size):
        self.loss_disc.zero_()
        self.optimizer.zero_grad(set_to_none=True)
        d, hot, cached = self.discriminators[0], self.weighted, self._target[0]
        op, total = d.operands(), None
        for (x1, x2), label, target in ((logits_s, self.source_label, False), (logits_t, self.target_label, True)):
            if target and cached is not None and cached[0][0] is x1 and cached[0][1] is x2 \
                    and cached[1] == (x1._version, x2._version) and cached[2] is op:
                z, acts, wmap = cached[3:]
            else:
                z, acts, wmap = self._forward_pair(d, x1.detach(), x2.detach(), size)
            _, dz, _ = ops.wbce_logits(z, size, label, wmap if target and hot else None, self.epsilon, self.lambda_local,
                                       scale=0.5, loss=self.loss_disc, accumulate=True)
            b = x1.shape[0]
            _, grads = backward_rows(op, dz.view(b, -1), acts, b, size[0], size[1], need_dparams=True, need_dinput=False)
            total = grads if total is None else {k: total[k] + v for k, v in grads.items()}
        for k in d.PARAMS:
            d.get_parameter(k).grad = total[k]
        self._target[0] = None
        self.optimizer.step()
        d.operands()                    # the parameters moved: rebuild the bf16 copies now
        self.steps_done += 1
        return self.loss_disc
