"""Loading libplslam_hip.so, and the one place a prototype of include/plslam_hip.h is applied.

Every concern module of the binding states its entry points with proto() beside the wrappers that call them; load() applies
them all to the library once.  Handle is the life cycle every library object shares.  There is NO CPU fallback: if the HIP
library is missing load() raises, and without a gfx950 device ``Context()`` raises ``PlslamError(PLSLAM_ENODEV)``.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libplslam_hip.so")
# experiment builds of the SAME library (tools/build_exp.py: timing-only variants of one kernel) are loaded through
# this variable by the tools under tools/; the product, the tests and bench.py never set it
if os.environ.get("PLSLAM_HIP_LIB_EXPERIMENT"):
    LIB_PATH = os.path.abspath(os.environ["PLSLAM_HIP_LIB_EXPERIMENT"])

OK, EINVAL, ENODEV, EHIP, ENOMEM, ERANGE, ENOTSUP = 0, -1, -2, -3, -4, -5, -6
ABI_VERSION = 5          # include/plslam_hip.h: PLSLAM_ABI_VERSION


class PlslamError(RuntimeError):
    def __init__(self, code: int, where: str, detail: str = ""):
        self.code = code
        super().__init__(f"{where}: {code} ({detail})")


class Cam(C.Structure):
    """plslam_cam (here, below every concern module: the prototypes of four of them take it by address)"""
    _fields_ = [("fx", C.c_double), ("fy", C.c_double), ("cx", C.c_double), ("cy", C.c_double),
                ("b", C.c_double), ("width", C.c_int32), ("height", C.c_int32)]


def make_cam(fx, fy, cx, cy, b=0.0, width=0, height=0) -> Cam:
    return Cam(float(fx), float(fy), float(cx), float(cy), float(b), int(width), int(height))


_lib = None
PROTOTYPES = {}         # name -> (argtypes, restype) of every entry point include/plslam_hip.h declares, in the order stated


def proto(name, argtypes, restype=C.c_int) -> None:
    """State the prototype of one entry point (at import, beside its wrapper).  Nothing is looked up per call: the wrappers
    call the bound function `self._L.plslam_x(...)`, which carries the prototype from load() on."""
    PROTOTYPES[name] = (argtypes, restype)
    if _lib is not None:
        _apply(_lib, name)


# name -> (header, argtypes, restype) of the entry points that OTHER headers of include/ declare (plslam_track.h): stated with
# proto_in() beside their wrappers and applied by load() in the same way.  PROTOTYPES stays the surface of plslam_hip.h alone.
HEADER_PROTOTYPES = {}


def proto_in(header, name, argtypes, restype=C.c_int) -> None:
    """proto() for an entry point that include/<header> declares."""
    if name in PROTOTYPES:
        raise ValueError(f"{name} is declared by include/plslam_hip.h")
    HEADER_PROTOTYPES[name] = (header, argtypes, restype)
    if _lib is not None:
        _apply(_lib, name)


def _apply(L, name) -> None:
    f = getattr(L, name)
    f.argtypes, f.restype = PROTOTYPES[name] if name in PROTOTYPES else HEADER_PROTOTYPES[name][1:]


proto("plslam_strerror", [C.c_int], C.c_char_p)
proto("plslam_last_error", [], C.c_char_p)
proto("plslam_abi_version", [])


def _preload_shared_hip_runtime() -> None:
    """PyTorch-ROCm wheels bundle their own libamdhip64.so.  A process must run ONE HIP runtime: if
    this library pulled in /opt/rocm's copy first and torch initialised its own afterwards, torch
    would find no GPU.  When torch is installed, load ITS runtime first (without importing torch) so
    that the dynamic loader resolves our DT_NEEDED libamdhip64 to the same copy."""
    import glob
    import importlib.util
    if "torch" in __import__("sys").modules:
        return                                   # torch already brought its runtime in
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    if spec is None or not spec.submodule_search_locations:
        return
    libdir = os.path.join(list(spec.submodule_search_locations)[0], "lib")
    for name in ("libamdhip64.so", "libamdhip64.so.*"):
        for path in sorted(glob.glob(os.path.join(libdir, name))):
            try:
                C.CDLL(path, mode=C.RTLD_GLOBAL)
                return
            except OSError:
                continue


def load() -> C.CDLL:
    """dlopen libplslam_hip.so and declare prototypes.  Fails loudly if it was not built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; "
            "g.build()'` (hipcc --offload-arch=gfx950).  There is no CPU fallback.")
    _preload_shared_hip_runtime()
    L = C.CDLL(LIB_PATH)
    L.plslam_abi_version.restype = C.c_int
    L.plslam_abi_version.argtypes = []
    if L.plslam_abi_version() != ABI_VERSION:
        raise RuntimeError(f"libplslam_hip.so has ABI version {L.plslam_abi_version()}, these bindings were written for {ABI_VERSION} "
                           "(struct layouts differ: rebuild with plslam_amd/build.py)")
    for name in (*PROTOTYPES, *HEADER_PROTOTYPES):
        _apply(L, name)
    _lib = L
    return L


def _check(code: int, where: str) -> None:
    if code != OK:
        L = load()
        raise PlslamError(code, where, f"{L.plslam_strerror(code).decode()}; "
                                       f"{L.plslam_last_error().decode()}")


def _arr(a, dt, shape=None):
    a = np.ascontiguousarray(a, dtype=dt)
    if shape is not None:
        a = a.reshape(shape)
    return a


_from_buffer, _addressof = C.c_char.from_buffer, C.addressof


def _p(a):
    """The address of a contiguous array as an int (every bound function declares void* arguments), None for None.  Through the
    buffer protocol: `a.ctypes.data_as(...)` builds a ctypes helper object per call -- 2 us each, 20 us of a matchGrid call's 58.
    For the same reason nothing stands in front of a bound function: no per-call wrapper, decorator or __getattr__."""
    if a is None:
        return None
    try:
        return _addressof(_from_buffer(a))
    except (TypeError, ValueError, BufferError):          # a read-only or an empty array
        return a.ctypes.data


def _hip_memcpy_dtod(dst: int, src: int, nbytes: int) -> int:
    """Device-to-device copy through the HIP runtime (tests: an in-place update of a plan's device state)."""
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    hip.hipMemcpy.restype = C.c_int
    return hip.hipMemcpy(C.c_void_p(dst), C.c_void_p(src), C.c_size_t(nbytes), 3)      # hipMemcpyDeviceToDevice


class Handle:
    """An object of the library that belongs to a context: a plan, a batch, a database, the context itself.  Every
    plslam_*_destroy reads handle->ctx, so a handle is destroyed only while its context is open; once the context is closed
    the handle is only dropped.  The handle object keeps its context object alive."""

    def _open(self, ctx, destroy_name, handle) -> None:
        self._L, self._destroy, self._h = ctx._L, getattr(ctx._L, destroy_name), handle
        if ctx is not self:                      # (a context is its own context: storing it would make it a reference cycle)
            self._ctx = ctx

    @property
    def handle(self):
        return self._h

    def close(self):
        h, ctx = getattr(self, "_h", None), getattr(self, "_ctx", self)     # (no _h: the create call raised)
        live = bool(h) and bool(ctx.handle)
        self._h = None
        if live:
            self._destroy(h)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
