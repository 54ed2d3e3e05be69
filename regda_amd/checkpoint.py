"""Saving and resuming a training run (INTEGRATION.md "Stopping and resuming a run").

The fused steps (regda_amd/step.py) own what the reference keeps in a torch.optim.SGD and a handful of
Python objects: momentum, the optimizer's `first` flag, the EMA teacher, the prototypes, class frequencies, loss
statistics, discriminators (and the step counter CLAN's preheat goes by), generator state.  `step.state_dict()` hands all
of it out as plain data, `step.load_state_dict()` puts it back IN PLACE (a recorded plan holds device addresses), and
because every step is bit-reproducible a resumed run continues with the bits of the uninterrupted one.

    save_training_state(path, step, iteration, **named)     named: further objects with a state_dict() (DomainMix, ...)
    load_training_state(path, step, **named) -> iteration

The rest of this module are the helpers the state_dict / load_state_dict pairs of the library share: a state is a nested
dict / list of CPU tensors, numbers, strings and None only (a file of it loads with torch.load(weights_only=True)), and a
load validates every entry before it writes the first one (ValueError naming the entry; the object stays as it was)."""
import os
import tempfile

import torch

FORMAT = 1
RESERVED = ('format', 'iteration', 'step')


def plain(obj):
    """A copy of `obj` as plain data: tensors detached and copied to the CPU, mappings as dicts, sequences as lists."""
    if isinstance(obj, torch.Tensor):
        return obj.detach().to('cpu', copy=True)
    if isinstance(obj, dict):
        return {k: plain(v) for k, v in obj.items()}
    if isinstance(obj, (list, tuple)):
        return [plain(v) for v in obj]
    if obj is None or isinstance(obj, (bool, int, float, str)):
        return obj
    if hasattr(obj, 'item') and getattr(obj, 'ndim', 1) == 0:       # a numpy scalar
        return obj.item()
    raise TypeError(f'{type(obj).__name__} is not plain data (tensor, number, string, None, list, dict)')


def need(sd, key, entry):
    """sd[key], or ValueError naming `entry.key`"""
    if not isinstance(sd, dict):
        raise ValueError(f'state entry {entry!r}: expected a dict, got {type(sd).__name__}')
    if key not in sd:
        raise ValueError(f'state entry {entry + "." if entry else ""}{key!r} is missing')
    return sd[key]


def check_equal(saved, own, entry):
    if saved != own:
        raise ValueError(f'state entry {entry!r}: the state holds {saved!r}, this object has {own!r}')


def check_format(sd, entry=''):
    f = need(sd, 'format', entry)
    if isinstance(f, bool) or not isinstance(f, int) or f != FORMAT:
        raise ValueError(f'state entry {entry + "." if entry else ""}\'format\': {f!r}; this library reads format {FORMAT}')


def check_tensor(value, entry, shape=None, dtype=None):
    if not isinstance(value, torch.Tensor):
        raise ValueError(f'state entry {entry!r}: expected a tensor, got {type(value).__name__}')
    if shape is not None and tuple(value.shape) != tuple(shape):
        raise ValueError(f'state entry {entry!r}: shape {tuple(value.shape)}, this object has {tuple(shape)}')
    if dtype is not None and value.dtype != dtype:
        raise ValueError(f'state entry {entry!r}: dtype {value.dtype}, this object has {dtype}')
    return value


def check_module_state(module, sd, entry, strict=True):
    """What module.load_state_dict(sd, strict) would object to, and what the modules' own `check_extra_state` object to,
    as ValueError BEFORE anything is written."""
    if not isinstance(sd, dict):
        raise ValueError(f'state entry {entry!r}: expected a dict, got {type(sd).__name__}')
    own = module.state_dict()
    missing = [k for k in own if k not in sd]
    extra = [k for k in sd if k not in own]
    if strict and (missing or extra):
        raise ValueError(f'state entry {entry!r}: missing keys {missing[:4]}, unexpected keys {extra[:4]} '
                         f'({len(missing)} / {len(extra)} in all)')
    for k, v in sd.items():
        if k not in own:
            continue
        if k.endswith('_extra_state'):
            owner = module.get_submodule(k.rpartition('.')[0])
            check = getattr(owner, 'check_extra_state', None)
            if check is not None:
                check(v, f'{entry}.{k}')
        else:
            check_tensor(v, f'{entry}.{k}', own[k].shape)


def copy_in_place(dst, src):
    """dst <- src into the storage `dst` already has (a recorded plan may hold its address)"""
    with torch.no_grad():
        dst.copy_(src.to(dst.dtype))


def save_training_state(path, step, iteration, **named):
    """Write {'format', 'iteration', 'step': step.state_dict(), <name>: obj.state_dict(), ...} to `path`: first to a
    temporary file in the same directory, then os.replace -- a job killed mid-write leaves the previous file whole.
    State is rank-local: every rank of a data-parallel run writes a path of its own."""
    for name in named:
        if name in RESERVED:
            raise ValueError(f'save_training_state: {name!r} is a reserved entry name')
    state = {'format': FORMAT, 'iteration': int(iteration), 'step': step.state_dict()}
    for name, obj in named.items():
        state[name] = plain(obj.state_dict())
    path = os.path.abspath(path)
    fd, tmp = tempfile.mkstemp(dir=os.path.dirname(path), prefix=os.path.basename(path) + '.', suffix='.tmp')
    try:
        with os.fdopen(fd, 'wb') as f:
            torch.save(state, f)
            f.flush()
            os.fsync(f.fileno())
        os.replace(tmp, path)
    except BaseException:
        try:
            os.unlink(tmp)
        except OSError:
            pass
        raise


def load_training_state(path, step, **named):
    """Load a file of save_training_state into `step` and the named objects; returns the iteration.  The file is read
    with weights_only=True.  Its format and its names are checked against `named` before anything is loaded; then the
    step and each object validate their own entry before they write it."""
    state = torch.load(path, map_location='cpu', weights_only=True)
    check_format(state)
    iteration = need(state, 'iteration', '')
    need(state, 'step', '')
    in_file = sorted(k for k in state if k not in RESERVED)
    if in_file != sorted(named):
        raise ValueError(f'{path}: the file holds the named entries {in_file}, the caller gave {sorted(named)}')
    step.load_state_dict(state['step'])
    for name, obj in named.items():
        obj.load_state_dict(state[name])
    return int(iteration)
