"""TransNorm -- mirror of regda/trans_norm.py (Transferable Normalization, Wang et al., NeurIPS 2019) on
rgda_transnorm_fwd / rgda_transnorm_bwd (csrc/transnorm_kernels.hip).

The first half of a training batch is the source domain, the rest the target domain (an odd batch gives the target one
more sample).  Each half is batch-normalised with its own statistics and the shared weight and bias, and every channel
is scaled by 1 + alpha, where alpha measures how close the two domains' normalised means are (alpha is a constant of the
gradient).  Eval mode normalises with the target's running statistics and forms alpha from the four running vectors.

Same constructor, parameters, buffers and `state_dict()` keys as the reference, so a checkpoint of either loads into
the other; a plain BatchNorm checkpoint (`running_mean` / `running_var`) fills both domains' buffers.

Where this differs from the reference, on purpose:
  * TransNorm1d serves (N, C) only and there is no TransNorm3d: on 3-D and 5-D inputs the reference never transposes
    the channels last and produces one alpha per position, an accident of its code and not the method.
  * A training batch in which a half has fewer than two values per channel raises ValueError (the reference returns NaN).
  * momentum=None raises ValueError at construction (the reference fails with a TypeError in its first forward).
  * track_running_stats=False serves training; eval raises a RuntimeError that names the cause (the reference dies on
    None + float).
  * Inputs are float32 tensors on the GPU; there is no CPU path.
"""
import itertools

import torch
from torch.nn.parameter import Parameter

from . import ops

_DOMAIN_SUFFIX = 7      # len('_source') == len('_target'): what a BatchNorm checkpoint's buffer names lack


class _TransNormFn(torch.autograd.Function):
    """y = TransNorm(x) in training or eval mode; gradients for x, weight and bias"""

    @staticmethod
    def forward(ctx, x, weight, bias, running, n_src, eps, momentum, training):
        y, saved = ops.transnorm_forward(x, n_src, weight, bias, running, eps, momentum, training)
        ctx.save_for_backward(x, weight, saved)
        ctx.n_src, ctx.training = n_src, training
        return y.view(x.shape)

    @staticmethod
    def backward(ctx, gy):
        x, weight, saved = ctx.saved_tensors
        need_dx = ctx.needs_input_grad[0]
        need_dp = weight is not None and (ctx.needs_input_grad[1] or ctx.needs_input_grad[2])
        dx, dw, db = ops.transnorm_backward(gy, x, saved, ctx.n_src, weight, ctx.training, need_dx, need_dp)
        if dx is not None:
            dx = dx.view(x.shape).to(x.dtype)
        return (dx, dw if ctx.needs_input_grad[1] else None, db if ctx.needs_input_grad[2] else None,
                None, None, None, None, None)


class _TransNorm(torch.nn.Module):
    def __init__(self, num_features, eps=1e-5, momentum=0.1, affine=True, track_running_stats=True):
        super().__init__()
        if momentum is None:
            raise ValueError('TransNorm: momentum=None (a cumulative average) is not served; the reference fails on it too')
        self.num_features = num_features
        self.eps = eps
        self.momentum = momentum
        self.affine = affine
        self.track_running_stats = track_running_stats
        if affine:
            self.weight = Parameter(torch.empty(num_features))
            self.bias = Parameter(torch.empty(num_features))
        else:
            self.register_parameter('weight', None)
            self.register_parameter('bias', None)
        if track_running_stats:
            self.register_buffer('running_mean_source', torch.zeros(num_features))
            self.register_buffer('running_mean_target', torch.zeros(num_features))
            self.register_buffer('running_var_source', torch.ones(num_features))
            self.register_buffer('running_var_target', torch.ones(num_features))
            self.register_buffer('num_batches_tracked', torch.tensor(0, dtype=torch.long))     # kept, never incremented
        else:
            for name in ('running_mean_source', 'running_mean_target', 'running_var_source', 'running_var_target'):
                self.register_parameter(name, None)
        self.reset_parameters()

    def reset_parameters(self):
        if self.track_running_stats:
            for m, v in ((self.running_mean_source, self.running_var_source),
                         (self.running_mean_target, self.running_var_target)):
                m.zero_()
                v.fill_(1)
        if self.affine:
            with torch.no_grad():
                self.weight.uniform_()       # the reference's draw: U[0, 1), not ones
                self.bias.zero_()

    def _check_input_dim(self, input):
        raise NotImplementedError

    def forward(self, input):
        self._check_input_dim(input)
        n, per_sample = input.shape[0], input[0, 0].numel() if input.shape[0] and input.shape[1] else 0
        running = None
        if self.track_running_stats:
            running = (self.running_mean_source, self.running_var_source, self.running_mean_target, self.running_var_target)
        if self.training:
            n_src = n // 2
            if n_src * per_sample < 2 or (n - n_src) * per_sample < 2:
                raise ValueError(f'TransNorm: a training batch of {n} samples of {per_sample} values per channel leaves a '
                                 f'domain half with fewer than two values per channel (no variance)')
        else:
            n_src = 0
            if running is None:
                raise RuntimeError('TransNorm: eval mode needs the running statistics, and this layer was built with '
                                   'track_running_stats=False')
        return _TransNormFn.apply(input, self.weight, self.bias, running, n_src, self.eps, self.momentum, self.training)

    def extra_repr(self):
        return '{num_features}, eps={eps}, momentum={momentum}, affine={affine}, ' \
               'track_running_stats={track_running_stats}'.format(**self.__dict__)

    def _load_from_state_dict(self, state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys, error_msgs):
        """Two kinds of checkpoint load.  One without `running_mean_source` is a plain BatchNorm's: its `running_mean` /
        `running_var` fill the buffers of BOTH domains (the domain suffix is dropped from the key that is looked up).
        One with it is a TransNorm's own and loads key for key.  As in the reference, keys of the checkpoint that this
        layer does not read are not reported."""
        if self.track_running_stats and prefix + 'num_batches_tracked' not in state_dict:
            state_dict[prefix + 'num_batches_tracked'] = torch.tensor(0, dtype=torch.long)
        from_batchnorm = prefix + 'running_mean_source' not in state_dict
        for name, mine in itertools.chain(self._parameters.items(), self._buffers.items()):
            if mine is None:
                continue
            key = prefix + name
            if from_batchnorm and name.endswith(('_source', '_target')):
                key = key[:-_DOMAIN_SUFFIX]
            if key not in state_dict:
                if strict:
                    missing_keys.append(key)
                continue
            theirs = state_dict[key]
            if theirs.shape != mine.shape:
                error_msgs.append(f'size mismatch for {key}: copying a param with shape {tuple(theirs.shape)} from '
                                  f'checkpoint, the shape in current model is {tuple(mine.shape)}.')
                continue
            with torch.no_grad():
                mine.copy_(theirs.detach())


class TransNorm1d(_TransNorm):
    """TransNorm over (N, C) inputs."""

    def _check_input_dim(self, input):
        if input.dim() == 3:
            raise ValueError('TransNorm1d: (N, C, L) inputs are not served: the reference forms one alpha per (channel, '
                             'position) on them, an accident of its code; reshape to (N, C, L, 1) and use TransNorm2d '
                             'for a per-channel alpha')
        if input.dim() != 2:
            raise ValueError('expected 2D input (got {}D input)'.format(input.dim()))
        if input.shape[1] != self.num_features:
            raise ValueError(f'TransNorm1d: {input.shape[1]} channels, expected {self.num_features}')


class TransNorm2d(_TransNorm):
    """TransNorm over (N, C, H, W) inputs."""

    def _check_input_dim(self, input):
        if input.dim() != 4:
            raise ValueError('expected 4D input (got {}D input)'.format(input.dim()))
        if input.shape[1] != self.num_features:
            raise ValueError(f'TransNorm2d: {input.shape[1]} channels, expected {self.num_features}')
