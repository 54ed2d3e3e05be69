"""Feature-space, class-level adversarial alignment -- FADA's recipe (Wang et al., ECCV 2020, "Classes Matter") on
PixelDiscriminator (regda/models/Discriminator.py:60-78): the discriminator reads the instance-normalised feature map
and answers, per pixel, with 2 * num_classes logits, the source half first.  The segmentation head's own temperature-
softened, capped predictions a = min(softmax(logits / T), clip) (T = 1.8, clip = 0.9, no gradient) say which class a pixel
belongs to; the loss is the soft cross-entropy of log_softmax(D(feat)) against a placed in one domain's half,

    l(z, a, side) = -(1 / M) sum_p sum_k a[p, k] * log_softmax(z[p, 0 : 2 nc])[side * nc + k],   M pixel rows of one domain.

The network is pushed to make target features look like source features of the same class (side 0 on target features),
the discriminator to tell the domains apart per class.  Adam with betas (0.9, 0.99) and lr 1e-4, the discriminator loss
halved, as there.

The reference ships the discriminator class but no loop that trains it, so this is an extension like the library's other
alignment terms.  One deviation from FADA, on purpose: FADA upsamples z to the image size and compares there; here the
loss is taken at feature resolution, so the map is never upsampled and the soft labels need no resize.  Everything on the
hot path is a kernel (csrc/fada_kernels.hip and the generic convolution routes); the optimizer is torch.optim (eight
small tensors).  Nothing here synchronises with the host.

    generator_term(feat_t, logits_t, rows_t, weight)
        weight * l(D(feat_t), a_t, side 0); its gradient with respect to the features -- through the discriminator's data
        gradients only, no weight gradients -- is ADDED onto rows_t (bf16 [b*h*w, k] pixel-major, the target rows of the
        gradient Deeplabv2._backward_plan(gfeat=) consumes).  Returns the loss, a device tensor.
    discriminator_step(feat_s, logits_s, feat_t, logits_t)
        0.5 * (l(D(feat_s), a_s, 0) + l(D(feat_t), a_t, 1)) on detached inputs, weight and bias gradients into .grad, one
        optimizer step, the bf16 operand copies rebuilt.  The target forward of the generator term is reused when it was
        made from the same feature tensor, unwritten since (its _version), and the same operand copies.
"""
import torch

from .. import ops
from ..checkpoint import check_module_state, need, plain
from ..models.PixelDiscriminator import backward_rows, trunk_rows


class FeatureAdversarialAligner:
    def __init__(self, discriminator, optimizer=None, lr=1e-4, betas=(0.9, 0.99), temperature=1.8, clip=0.9):
        if discriminator is None:
            raise ValueError('FeatureAdversarialAligner: no discriminator given')
        if not float(temperature) > 0.0:
            raise ValueError(f'FeatureAdversarialAligner: temperature must be positive, got {temperature!r}')
        if not 0.0 < float(clip) <= 1.0:
            raise ValueError(f'FeatureAdversarialAligner: clip caps probabilities, 0 < clip <= 1, got {clip!r}')
        self.discriminator = discriminator
        self.temperature, self.clip = float(temperature), float(clip)
        params = list(discriminator.parameters())
        self.optimizer = optimizer if optimizer is not None else torch.optim.Adam(params, lr=lr, betas=betas)
        dev = params[0].device
        self.loss_fada = torch.zeros(1, device=dev)
        self.loss_disc = torch.zeros(1, device=dev)
        self._target = None     # from the generator term: (feature tensor, its _version, operands, activations)

    def check_served(self, feat_shape, logits_shape):
        """ValueError before anything is launched where the discriminator does not serve (b, k, h, w) features with
        (b, C, h, w) logits"""
        d = self.discriminator
        d.check_served(tuple(feat_shape), 'FeatureAdversarialAligner')
        if len(logits_shape) != 4 or tuple(logits_shape[i] for i in (0, 2, 3)) != tuple(feat_shape[i] for i in (0, 2, 3)):
            raise ValueError(f'FeatureAdversarialAligner: logits {tuple(logits_shape)} do not lie on the pixels of the '
                             f'features {tuple(feat_shape)}')
        if logits_shape[1] != d.num_classes:
            raise ValueError(f'FeatureAdversarialAligner: {logits_shape[1]} logit channels, the discriminator was built for '
                             f'num_classes = {d.num_classes} (the soft labels fill one half of its output)')

    # training state (regda_amd/checkpoint.py)
    def state_dict(self):
        """{'discriminator': its state_dict(), 'optimizer': the optimizer's state_dict()}, plain data"""
        torch.cuda.synchronize()
        return plain({'discriminator': self.discriminator.state_dict(), 'optimizer': self.optimizer.state_dict()})

    def check_state_dict(self, sd, strict=True, entry='FeatureAdversarialAligner'):
        """ValueError naming the entry where load_state_dict would not take `sd`; writes nothing"""
        check_module_state(self.discriminator, need(sd, 'discriminator', entry), entry + '.discriminator', strict)
        opt = need(sd, 'optimizer', entry)
        groups, own = need(opt, 'param_groups', entry + '.optimizer'), self.optimizer.state_dict()['param_groups']
        need(opt, 'state', entry + '.optimizer')
        if not isinstance(groups, list) or [len(g['params']) for g in groups] != [len(g['params']) for g in own]:
            raise ValueError(f"state entry '{entry}.optimizer.param_groups': the parameter groups differ from this optimizer's")

    def load_state_dict(self, sd, strict=True):
        """Validates first, then loads the discriminator (in place), the optimizer's moments, and rebuilds the bf16
        operand copies.  Nothing of the generator term's cached forward survives."""
        self.check_state_dict(sd, strict)
        torch.cuda.synchronize()
        self.discriminator.load_state_dict(sd['discriminator'], strict=strict)
        self.optimizer.load_state_dict(sd['optimizer'])
        self._target = None
        self.discriminator.operands()

    def _forward(self, feat):
        b, _, h, w = feat.shape
        return trunk_rows(self.discriminator.operands(), ops.feat_pack_rows(feat), b, h, w)

    def _loss(self, acts, logits, side, scale, loss):
        op = self.discriminator.operands()
        return ops.fada_loss(acts[2], op.wf[2], op.bias[2], logits, side, self.temperature, self.clip, scale, loss=loss)[1]

    def generator_term(self, feat_t, logits_t, rows_t, weight):
        self.loss_fada.zero_()
        self._target = None
        if not weight:
            return self.loss_fada
        x, logits = feat_t.detach(), logits_t.detach()
        self.check_served(x.shape, logits.shape)
        b, k, h, w = x.shape
        assert rows_t.dtype == torch.bfloat16 and tuple(rows_t.shape) == (b * h * w, k) and rows_t.is_contiguous()
        op = self.discriminator.operands()
        acts = self._forward(x)
        dz = self._loss(acts, logits, 0, float(weight), self.loss_fada)
        backward_rows(op, dz, acts, b, h, w, need_dparams=False, onto=rows_t)
        # valid while neither the features nor the discriminator's operand copies (rebuilt when a parameter moves) change
        self._target = (feat_t, feat_t._version, op, acts)
        return self.loss_fada

    def discriminator_step(self, feat_s, logits_s, feat_t, logits_t):
        self.loss_disc.zero_()
        self.optimizer.zero_grad(set_to_none=True)
        d = self.discriminator
        op, total = d.operands(), None
        for feat, logits, side, cached in ((feat_s, logits_s, 0, None), (feat_t, logits_t, 1, self._target)):
            x, logits = feat.detach(), logits.detach()
            self.check_served(x.shape, logits.shape)
            b, _, h, w = x.shape
            if cached is not None and cached[0] is feat and cached[1] == feat._version and cached[2] is op:
                acts = cached[3]
            else:
                acts = self._forward(x)
            dz = self._loss(acts, logits, side, 0.5, self.loss_disc)
            _, grads = backward_rows(op, dz, acts, b, h, w, need_dparams=True, need_dinput=False)
            total = grads if total is None else {k: total[k] + v for k, v in grads.items()}
        for k in d.PARAMS:
            d.get_parameter(k).grad = total[k]
        self._target = None
        self.optimizer.step()
        d.operands()                    # the parameters moved: rebuild the bf16 copies now
        return self.loss_disc
