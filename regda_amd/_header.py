"""The one reader of include/rgda_hip.h: its prototypes and its integer constants.

Standard library only, and importable by path without the package: the Makefile's thunk generator
(csrc/gen_thunks.py) and the ctypes binding (_lib.py) both read the ABI from here, so neither can drift from the header
or from the other.  A header is read once per process.
"""
import functools
import os
import re

HEADER_PATH = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'rgda_hip.h')


@functools.lru_cache(maxsize=None)
def _read(path):
    src = open(path).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    src = re.sub(r'//[^\n]*', '', src)
    protos = []
    for m in re.finditer(r'\b(int|size_t|const char\s*\*)\s+(rgda_\w+)\s*\(([^;{]*?)\)\s*;', src, flags=re.S):
        args = m.group(3).strip()
        args = [] if args in ('', 'void') else [' '.join(a.split()) for a in args.split(',')]
        protos.append((' '.join(m.group(1).split()), m.group(2), args))
    consts = {m.group(1): int(m.group(2), 0)
              for m in re.finditer(r'^[ \t]*#[ \t]*define[ \t]+(RGDA_\w+)[ \t]+(0[xX][0-9a-fA-F]+|\d+)[ \t]*$', src, flags=re.M)}
    return protos, consts


def prototypes(path=HEADER_PATH):
    """-> [(return type, name, [argument type strings])] for every function the header declares, in its order.  An
    argument string is the declaration with single spaces ('const float* x', 'int n')."""
    return _read(path)[0]


def constants(path=HEADER_PATH):
    """-> {name: value} for every `#define RGDA_* <integer>` (decimal or hex) of the header."""
    return _read(path)[1]
