"""CPU-only: the C-ABI library loads and exports every symbol include/pcacc.h declares, and the ctypes binding agrees with the header's prototypes
(no compute calls)."""
import ast
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared():
    text = open(os.path.join(ROOT, 'include', 'pcacc.h')).read()
    text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    return sorted(set(re.findall(r'\b(pcacc_[a-z0-9_]+)\s*\(', text)))


def test_header_declares_entry_points():
    names = _declared()
    assert 'pcacc_voxelize' in names and 'pcacc_pillar_scatter' in names and 'pcacc_chamfer_forward' in names
    assert len(names) >= 20


def test_library_exports_every_declared_symbol():
    import __graft_entry__ as g
    g.build()
    from pcaccumulation_amd import native
    assert os.path.exists(native.LIB_PATH)
    lib = ctypes.CDLL(native.LIB_PATH)
    for name in _declared():
        assert hasattr(lib, name), name
    lib.pcacc_target.restype = ctypes.c_char_p
    assert lib.pcacc_target() == b'gfx950'
    assert sorted(native.EXPORTS + ['pcacc_target']) == _declared()


def _prototypes():
    """{entry point: [parameter, ...]} from the header's text (a parse of this file's own: it does not read back what native computed)."""
    text = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'pcacc.h')).read(), flags=re.S)
    protos = {}
    for m in re.finditer(r'\b(pcacc_[a-z0-9_]+)\s*\(', text):
        params = text[m.end():text.index(')', m.end())]
        protos[m.group(1)] = [] if params.strip() == 'void' else [p.strip() for p in params.split(',')]
    return protos


_WIDTH = {'int': ctypes.c_int, 'int32_t': ctypes.c_int32, 'int64_t': ctypes.c_int64, 'uint64_t': ctypes.c_uint64, 'size_t': ctypes.c_size_t,
          'float': ctypes.c_float, 'double': ctypes.c_double}


def test_every_entry_point_has_the_prototypes_argtypes():
    """After native.lib() each declared entry point carries argtypes of its prototype's length, pointer for pointer and width for width."""
    import __graft_entry__ as g
    g.build()
    from pcaccumulation_amd import native
    lib = native.lib()
    protos = _prototypes()
    assert sorted(protos) == _declared()
    assert len(protos['pcacc_voxelize']) == 15 and len(protos['pcacc_reload_switches']) == 0 and len(protos['pcacc_target']) == 0
    for name, params in protos.items():
        fn = getattr(lib, name)
        assert fn.argtypes is not None, name
        assert len(fn.argtypes) == len(params), (name, len(fn.argtypes), len(params))
        assert fn.restype is (ctypes.c_char_p if name == 'pcacc_target' else ctypes.c_int), name
        for got, p in zip(fn.argtypes, params):
            want = ctypes.c_void_p if '*' in p else _WIDTH[' '.join(p.replace('const', ' ').split()[:-1])]
            assert got is want, (name, p, got)


def native_call_mismatches(path, protos):
    """An ast walk over the binding: every use of a `.pcacc_x` attribute is attributed to a call and the call's argument count compared with the
    prototype's (ctypes refuses too few arguments at run time, never too many).  -> list of complaints, empty when all agree.  Attributed are
      lib().pcacc_x(a, ...)                               a direct call
      _workspace(lib().pcacc_x_workspace_bytes, dev, ...)  the helper appends the byref(size) argument itself: sizes + 1
      fn = lib().pcacc_a if ... else lib().pcacc_b        then fn(a, ...) in the same function, against both prototypes
      _lib.pcacc_target.restype / .argtypes                the loader's own assignment."""
    tree = ast.parse(open(path).read())
    bad, seen = [], set()

    def own(node):
        return [a for a in ast.walk(node) if isinstance(a, ast.Attribute) and a.attr.startswith('pcacc_')]

    def compare(name, n_args, call):
        if any(isinstance(a, ast.Starred) for a in call.args) or call.keywords:
            bad.append('%s line %d: starred / keyword arguments cannot be counted' % (name, call.lineno))
        elif name not in protos:
            bad.append('%s line %d: not declared in include/pcacc.h' % (name, call.lineno))
        elif n_args != len(protos[name]):
            bad.append('%s line %d: %d arguments, the prototype has %d' % (name, call.lineno, n_args, len(protos[name])))

    for scope in [n for n in ast.walk(tree) if isinstance(n, ast.FunctionDef)]:
        aliases = {}
        nodes = list(ast.walk(scope))
        for node in nodes:
            if isinstance(node, ast.Assign) and len(node.targets) == 1 and isinstance(node.targets[0], ast.Name) and own(node.value) \
                    and not isinstance(node.value, ast.Call):
                aliases[node.targets[0].id] = own(node.value)
        for node in nodes:
            if not isinstance(node, ast.Call):
                continue
            f = node.func
            if isinstance(f, ast.Attribute) and f.attr.startswith('pcacc_'):
                seen.add(f)
                compare(f.attr, len(node.args), node)
            elif isinstance(f, ast.Name) and f.id == '_workspace' and node.args and own(node.args[0]) == [node.args[0]]:
                seen.add(node.args[0])
                compare(node.args[0].attr, len(node.args) - 2 + 1, node)
            elif isinstance(f, ast.Name) and f.id in aliases:
                for a in aliases[f.id]:
                    seen.add(a)
                    compare(a.attr, len(node.args), node)
    for a in own(tree):
        if a not in seen and a.attr != 'pcacc_target':
            bad.append('%s line %d: a use of an entry point this walk cannot attribute to a call' % (a.attr, a.lineno))
    return bad


def test_every_native_call_has_the_prototypes_argument_count():
    protos = _prototypes()
    path = os.path.join(ROOT, 'pcaccumulation_amd', 'native.py')
    assert native_call_mismatches(path, protos) == []
    called = set(re.findall(r'\.(pcacc_[a-z0-9_]+)\b', open(path).read()))
    assert len(called) >= 150, 'the walk found only %d entry points in use: it is looking at the wrong file' % len(called)


def test_no_cpu_fallback():
    """The product path refuses CPU tensors instead of silently computing on the host."""
    import torch
    from pcaccumulation_amd import native
    with pytest.raises(native.NativeError):
        native.rigid_transform(torch.zeros(4, 3), torch.zeros(4, dtype=torch.int32), torch.zeros(1, 16))


def test_product_does_not_import_oracle():
    pkg = os.path.join(ROOT, 'pcaccumulation_amd')
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith('.py'):
                src = open(os.path.join(dirpath, f)).read()
                assert not re.search(r'^\s*(import oracle|from oracle)', src, flags=re.M), f
