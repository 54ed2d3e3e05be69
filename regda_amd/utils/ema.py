"""ExponentialMovingAverage with the reference's public surface (regda/utils/ema.py:34-65): `register()`, `update()`,
`apply_shadow()`, `restore()`, and the `shadow` / `backup` dicts keyed by parameter name.  Only parameters that require
gradients are averaged; BatchNorm buffers are not (they stay the live model's).

This class is the drop-in for scripts that drive the EMA themselves.  The fused training step (regda_amd/ssl.py) does
not use it: there the average is one more output of the optimizer kernel (rgda_sgd_step)."""
import torch


class ExponentialMovingAverage:
    def __init__(self, model, decay):
        self.model, self.decay = model, decay
        self.shadow, self.backup = {}, {}

    def _trainable(self):
        return ((n, p) for n, p in self.model.named_parameters() if p.requires_grad)

    def _resync(self):
        sync = getattr(self.model, 'sync_weights', None)       # regda_amd models mirror their weights in bf16
        if sync is not None:
            sync()

    def register(self):
        self.shadow = {n: p.detach().clone() for n, p in self._trainable()}

    # training state (regda_amd/checkpoint.py): the averaged weights; `backup` lives only between apply_shadow / restore
    def state_dict(self):
        return {'shadow': {n: v.detach().to('cpu', copy=True) for n, v in self.shadow.items()}}

    @torch.no_grad()
    def load_state_dict(self, sd, strict=True):
        """Validates first (ValueError naming the entry, nothing written), then copies into the shadow tensors this
        object holds, creating those it lacks.  strict=False: names the state lacks are left as they are."""
        shadow = sd.get('shadow') if isinstance(sd, dict) else None
        if not isinstance(shadow, dict):
            raise ValueError("state entry 'ExponentialMovingAverage.shadow' is missing")
        params = dict(self._trainable())
        missing = [n for n in params if n not in shadow]
        extra = [n for n in shadow if n not in params]
        if strict and (missing or extra):
            raise ValueError(f"state entry 'ExponentialMovingAverage.shadow': missing {missing[:4]}, unexpected {extra[:4]}")
        for n, v in shadow.items():
            if n in params and (not isinstance(v, torch.Tensor) or v.shape != params[n].shape):
                raise ValueError(f"state entry 'ExponentialMovingAverage.shadow.{n}': expected a tensor of shape "
                                 f'{tuple(params[n].shape)}')
        for n, v in shadow.items():
            if n not in params:
                continue
            if n in self.shadow:
                self.shadow[n].copy_(v)
            else:
                self.shadow[n] = v.to(device=params[n].device, dtype=params[n].dtype, copy=True)

    @torch.no_grad()
    def update(self):
        d = self.decay
        for n, p in self._trainable():
            if n not in self.shadow:
                raise AssertionError(f'{n} was not registered')
            self.shadow[n] = (1.0 - d) * p.detach() + d * self.shadow[n]

    @torch.no_grad()
    def apply_shadow(self):
        """Swap the averaged weights in (the live ones are kept in `backup`)."""
        for n, p in self._trainable():
            if n not in self.shadow:
                raise AssertionError(f'{n} was not registered')
            self.backup[n] = p.detach().clone()
            p.copy_(self.shadow[n])             # in place: regda_amd parameters are views of one flat buffer
        self._resync()

    @torch.no_grad()
    def restore(self):
        for n, p in self._trainable():
            if n not in self.backup:
                raise AssertionError(f'{n} has no backup: apply_shadow() first')
            p.copy_(self.backup[n])
        self.backup = {}
        self._resync()
