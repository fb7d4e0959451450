#!/usr/bin/env python3
"""The surface of the ctypes binding as one JSON document: what plslam_amd.capi exposes (names, class members, signatures),
plslam_amd.__all__, the layout of every ctypes struct, the prototype of every ABI symbol and the module-level constants.
Needs the built library, not a GPU.  tests/test_binding_surface_cpu.py compares it with tests/golden/binding_surface.json.

    python tools/binding_surface.py > tests/golden/binding_surface.json
"""
from __future__ import annotations

import ctypes as C
import inspect
import json
import os
import re
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

CONSTANTS = re.compile(r"^(OK|E[A-Z]+|ABI_VERSION|MAX_TRAIN_ROWS|\w+_MAX_\w+|\w+_STOP_\w+|SCAN_\w+|BOW_\w+|GBA_LIST_NAMES|\w+_DTYPE)$")


def _signature(f):
    try:
        return str(inspect.signature(f))
    except (TypeError, ValueError):
        return None


def _members(cls) -> dict:
    """every member a class has and object has not (plus __init__) -> its signature, None for what is not callable"""
    out = {}
    for name in dir(cls):
        if name in dir(object) and name != "__init__":
            continue
        m = inspect.getattr_static(cls, name)
        f = m.__func__ if isinstance(m, (staticmethod, classmethod)) else m
        out[name] = _signature(f) if callable(f) else None
    return out


def _type_name(t):
    return None if t is None else t.__name__


def _struct(cls) -> dict:
    fields = [[n, _type_name(t), getattr(cls, n).offset, getattr(cls, n).size] for n, t in cls._fields_]
    return {"sizeof": C.sizeof(cls), "fields": fields}


def _constant(v):
    if hasattr(v, "descr"):                                  # a numpy dtype
        return json.loads(json.dumps(v.descr))
    return list(v) if isinstance(v, tuple) else v


def surface() -> dict:
    import plslam_amd
    from plslam_amd import capi
    L = plslam_amd.load()
    names, structs, constants = {}, {}, {}
    for name, v in sorted(vars(capi).items()):
        if name.startswith("__"):
            continue
        if inspect.isclass(v):
            names[name] = {"kind": "class", "members": _members(v)}
            if issubclass(v, C.Structure) and v is not C.Structure:
                structs[name] = _struct(v)
        elif inspect.isfunction(v):
            names[name] = {"kind": "function", "signature": _signature(v)}
        else:
            names[name] = {"kind": "other"}
            if CONSTANTS.match(name):
                constants[name] = _constant(v)
    symbols = {s: {"argtypes": [_type_name(t) for t in getattr(L, s).argtypes], "restype": _type_name(getattr(L, s).restype)}
               for s in plslam_amd.ABI_SYMBOLS}
    return {"capi": names, "all": sorted(plslam_amd.__all__), "structs": structs, "symbols": symbols, "constants": constants}


if __name__ == "__main__":
    json.dump(surface(), sys.stdout, indent=1, sort_keys=True)
    sys.stdout.write("\n")
