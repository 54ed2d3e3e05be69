"""Mint tests/golden/ops_surface.json: the flat namespace of regda_amd.ops as outside users see it.

Run from a checkout (no GPU and no built library needed: nothing is called):  python tests/golden/make_ops_surface.py
Data only:
  callables: every public function or class DEFINED by the binding (its __module__ is regda_amd.ops or a module of the
             private package regda_amd._ops), with str(inspect.signature(...));
  constants: every upper-case public name with its value (tuples as lists, as JSON stores them);
  private:   the underscore names that tests, the benchmark and the gast modules reach through `ops.`.
The file was minted before ops.py was split by kernel family and is the fixture tests/test_ops_surface_cpu.py holds the
split against; re-mint it only with a change that means to alter the surface."""
import inspect
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

PRIVATE = ('_stream', '_p', '_need_cuda', '_WgradDesc', '_ConvDesc', '_BnOperand')


def surface():
    from regda_amd import ops
    callables, constants = {}, {}
    for name, v in vars(ops).items():
        if name.startswith('_') or inspect.ismodule(v):
            continue
        if name.isupper():
            constants[name] = v
        elif callable(v) and (v.__module__ == 'regda_amd.ops' or v.__module__.startswith('regda_amd._ops')):
            callables[name] = str(inspect.signature(v))
    return dict(callables=dict(sorted(callables.items())), constants=dict(sorted(constants.items())), private=list(PRIVATE))


def main():
    with open(os.path.join(HERE, 'ops_surface.json'), 'w') as f:
        json.dump(surface(), f, indent=1, sort_keys=True)
        f.write('\n')


if __name__ == '__main__':
    main()
