"""CPU: regda_amd.ops is a facade over the family modules of regda_amd/_ops and must stay the namespace it was as one
file: the public names, signatures and constants of tests/golden/ops_surface.json (minted before the split by
tests/golden/make_ops_surface.py), one stream cache, convolution wrappers that the benchmark can still replace, and
constants that are the header's own numbers."""
import importlib
import importlib.util
import json
import os
import pkgutil
import re
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
PATCHED = ('conv2d', 'conv2d_wgrad', 'conv2d_bneval', 'conv2d_bnbwd', 'conv2d_wgrad_grouped', 'conv2d_bnin', 'conv2d_grouped')

# (python name, where it lives, header name): every number of the binding that mirrors a #define of include/rgda_hip.h
MIRRORED = [
    ('STAT_FRAC_FWD', 'ops', 'RGDA_STAT_FRAC_FWD'), ('STAT_FRAC_BWD', 'ops', 'RGDA_STAT_FRAC_BWD'),
    ('IAST_BINS', 'ops', 'RGDA_IAST_BINS'), ('ANALYSIS_MAX_BINS', 'ops', 'RGDA_ANALYSIS_MAX_BINS'),
    ('MIX_TABLE_COLS', 'ops', 'RGDA_MIX_TABLE_COLS'), ('MIX_WRITE_MAX_IMAGES', 'ops', 'RGDA_MIX_WRITE_MAX_IMAGES'),
    ('STRONG_TABLE_COLS', 'ops', 'RGDA_STRONG_TABLE_COLS'), ('STRONG_MAX_RADIUS', 'ops', 'RGDA_STRONG_MAX_RADIUS'),
    ('STYLE_TABLE_COLS', 'ops', 'RGDA_STYLE_TABLE_COLS'), ('STYLE_MAX_B', 'ops', 'RGDA_STYLE_MAX_B'),
    ('STYLE_MAX_IMAGES', 'ops', 'RGDA_STYLE_MAX_IMAGES'), ('MAX_ARGS', 'plan', 'RGDA_PLAN_MAX_ARGS'),
]


def _generator():
    spec = importlib.util.spec_from_file_location('make_ops_surface', os.path.join(HERE, 'golden', 'make_ops_surface.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope='module')
def golden():
    with open(os.path.join(HERE, 'golden', 'ops_surface.json')) as f:
        return json.load(f)


def _all_submodules():
    import regda_amd
    for m in pkgutil.walk_packages(regda_amd.__path__, 'regda_amd.'):
        importlib.import_module(m.name)
    return {k: v for k, v in sys.modules.items() if k.startswith('regda_amd.') and v is not None}


def test_public_names_signatures_and_constants_are_the_fixture(golden):
    from regda_amd import ops
    now = json.loads(json.dumps(_generator().surface()))        # tuples as lists, as the fixture stores them
    assert sorted(now['callables']) == sorted(golden['callables'])
    assert sorted(now['constants']) == sorted(golden['constants'])
    for name, sig in golden['callables'].items():
        assert now['callables'][name] == sig, name
    for name, value in golden['constants'].items():
        assert now['constants'][name] == value, name
    for name in golden['private']:
        assert hasattr(ops, name), name
    assert os.path.basename(ops.__file__) == 'ops.py'


def test_one_stream_cache():
    from regda_amd import ops
    from regda_amd._ops import base
    mods = {k: v for k, v in _all_submodules().items() if k.startswith('regda_amd._ops.')}
    assert len(mods) >= 10 and 'regda_amd._ops.conv' in mods
    for name, mod in mods.items():
        if hasattr(mod, '_stream'):
            assert mod._stream is ops._stream, name
        if mod is not base:
            assert not hasattr(mod, '_STREAM'), f'{name} holds a frozen copy of the stream cache'
    assert ops._stream is base._stream and ops.use_stream is base.use_stream and not hasattr(ops, '_STREAM')


def test_only_ops_and_the_convolution_family_bind_the_patched_names():
    for name, mod in _all_submodules().items():
        if name in ('regda_amd.ops', 'regda_amd._ops.conv'):
            continue
        held = [p for p in PATCHED if p in vars(mod)]
        assert not held, f'{name} binds {held}: a replacement set on regda_amd.ops would not reach it'


def test_a_replacement_on_ops_reaches_the_model():
    from regda_amd import ops
    from regda_amd.models import Encoder
    sentinel = object()
    orig = ops.conv2d
    try:
        ops.conv2d = sentinel
        assert Encoder.ops.conv2d is sentinel
    finally:
        ops.conv2d = orig
    assert Encoder.ops.conv2d is orig


def test_every_integer_define_parses_and_the_mirrors_are_the_headers():
    from regda_amd import _header, ops, plan
    consts = _header.constants()
    src = open(_header.HEADER_PATH).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    declared = re.findall(r'^[ \t]*#[ \t]*define[ \t]+(RGDA_\w+)[ \t]+\S', src, flags=re.M)     # every define with a value
    assert len(declared) >= 20 and sorted(declared) == sorted(consts), sorted(set(declared) ^ set(consts))
    assert len(set(declared)) == len(declared)
    assert consts['RGDA_IAST_BINS'] == 0x7C01 and consts['RGDA_ABI_VERSION'] == 10
    where = dict(ops=ops, plan=plan)
    for py, mod, c in MIRRORED:
        assert getattr(where[mod], py) == consts[c], (py, c)
    assert ops.MMD_KERNEL_TYPES == {'rbf': consts['RGDA_MMD_RBF'], 'linear': consts['RGDA_MMD_LINEAR']}


def test_prototypes_are_what_the_binding_and_the_thunks_read():
    from regda_amd import _header, _lib
    protos = _header.prototypes()
    names = [name for _, name, _ in protos]
    assert len(names) == len(set(names)) and set(names) == set(_lib.parse_header())
    assert {'int', 'size_t'} < {ret for ret, _, _ in protos}
    ret, _, args = next(p for p in protos if p[1] == 'rgda_abi_version')
    assert ret == 'int' and args == []
