"""The surface of the ctypes binding against tests/golden/binding_surface.json, which tools/binding_surface.py wrote BEFORE the
binding was split into one module per concern: every name plslam_amd.capi exposed, every class member and signature, the
layout of every struct, the prototype of every ABI symbol and the constants are still there and equal.  No GPU needed."""
import ast
import importlib.util
import json
import os

import plslam_amd
from plslam_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# what the split changed on purpose, path in the document -> the value it has now (None: the name is gone)
EXPECTED = {
    # load() takes every return type from the prototype itself
    ("capi", "_RESTYPES"): None,
    # close() is Handle's for every handle class: the same call without arguments, the annotation of three of them went
    ("capi", "GbaPlan", "members", "close"): "(self)",
    ("capi", "LcBatch", "members", "close"): "(self)",
    ("capi", "PgoPlan", "members", "close"): "(self)",
}


def _surface():
    spec = importlib.util.spec_from_file_location("binding_surface", os.path.join(ROOT, "tools", "binding_surface.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return json.loads(json.dumps(mod.surface()))           # (tuples -> lists, as in the committed file)


def _differences(want, got, path=()):
    if isinstance(want, dict) and isinstance(got, dict):
        for k, v in want.items():
            if k not in got:
                yield path + (k,), None
            else:
                yield from _differences(v, got[k], path + (k,))
    elif want != got:
        yield path, got


def test_surface_is_the_committed_one():
    want = json.load(open(os.path.join(ROOT, "tests", "golden", "binding_surface.json")))
    assert len(want["structs"]) == 26 and len(want["symbols"]) == 153 and len(want["all"]) == 25
    assert dict(_differences(want, _surface())) == EXPECTED


def test_abi_symbols_are_the_registered_prototypes():
    L = plslam_amd.load()
    assert plslam_amd.ABI_SYMBOLS == plslam_amd.capi.ABI_SYMBOLS == tuple(_lib.PROTOTYPES)
    assert len(set(plslam_amd.ABI_SYMBOLS)) == len(plslam_amd.ABI_SYMBOLS) == 153
    for name, (argtypes, restype) in _lib.PROTOTYPES.items():
        f = getattr(L, name)
        assert list(f.argtypes) == list(argtypes) and f.restype is restype, name


def test_a_prototype_stated_after_load_is_applied_at_once():
    L = plslam_amd.load()
    was = _lib.PROTOTYPES["plslam_abi_version"]
    try:
        _lib.proto("plslam_abi_version", [], _lib.C.c_uint)
        assert L.plslam_abi_version.restype is _lib.C.c_uint and L.plslam_abi_version() == _lib.ABI_VERSION
    finally:
        _lib.proto("plslam_abi_version", *was)


def test_no_struct_is_defined_inside_a_function():
    pkg, found = os.path.join(ROOT, "plslam_amd"), []
    for f in sorted(os.listdir(pkg)):
        if not f.endswith(".py"):
            continue
        tree = ast.parse(open(os.path.join(pkg, f)).read())
        for fn in ast.walk(tree):
            if isinstance(fn, (ast.FunctionDef, ast.AsyncFunctionDef)):
                for node in ast.walk(fn):
                    if isinstance(node, ast.ClassDef) and any("Structure" in ast.unparse(b) for b in node.bases):
                        found.append(f"{f}:{node.lineno} {node.name}")
    assert not found, found
