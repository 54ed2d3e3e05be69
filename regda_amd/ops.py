"""Thin tensor-level wrappers over the C ABI (include/rgda_hip.h).

Everything here takes/returns CUDA(ROCm) torch tensors, enqueues on
`torch.cuda.current_stream()` and never synchronises.  PyTorch is plumbing
(device memory + streams); the arithmetic is in librgda_hip.so.

This file is the flat namespace only: the wrappers live in regda_amd/_ops/, one module per kernel family (csrc/*.hip) on
the helpers of _ops/base.py, and tests/golden/ops_surface.json pins what is exported.  Callers keep using `ops.<name>`:
the benchmark's per-kernel probe replaces the convolution wrappers on THIS module, so the library reaches them as
attributes of it at call time and never binds them with `from`.  The stream cache (_ops/base.py: _STREAM) is not
re-exported: use_stream rebinds it, and a copy here would stay None.
"""
# flake8: noqa: F401,F403
from ._ops.base import *
from ._ops.base import _need_cuda, _p, _stream
from ._ops.label import *
from ._ops.chores import *
from ._ops.upsample import *
from ._ops.pseudo import *
from ._ops.conv import *
from ._ops.conv import _BnOperand, _ConvDesc, _WgradDesc
from ._ops.norm import *
from ._ops.window import *
from ._ops.augment import *
from ._ops.mix_domain import *
from ._ops.feature import *
from ._ops.category import *
from ._ops.adv import *
