"""desc_list / dir_list / pts_list and the representative descriptor of the device-resident map (plslam_map_lists,
include/plslam_hip.h): the side lists in the observation order of the image, carried through plslam_map_insert_* and
plslam_lc_fuse_run on the device, the representative refreshed for exactly the landmarks the reference refreshes.

Three parts: the ctypes structs; DeviceMapLists (torch buffers per kind with capacities), DeviceRows (a keyframe's / a fusion's
rows on the device) and MapLists, the three calls; and the SEEDED generators synthetic_lists / keyframe_rows / tuple_rows with
representative(), the rule of MapPoint::updateAverageDescDir (src/mapFeatures.cpp:51-84) in numpy for the generators."""
from __future__ import annotations

import ctypes as C

import numpy as np

from ._lib import _check, proto
from .synth import random_desc

_vp = C.c_void_p
FIELDS = ("desc", "dir", "pts", "med_idx", "med_desc", "refreshed")
# per field: (dtype, columns, per observation (else per landmark))
_SHAPE = dict(desc=(np.uint8, 32, True), dir=(np.float64, 3, True), pts=(np.float64, 4, True), med_idx=(np.int32, 1, False),
              med_desc=(np.uint8, 32, False), refreshed=(np.uint8, 1, False))


class MapListsKind(C.Structure):
    _fields_ = [(k, _vp) for k in FIELDS]


class MapListsStruct(C.Structure):
    _fields_ = [("points", MapListsKind), ("lines", MapListsKind)]


class MapInsertRows(C.Structure):
    _fields_ = [(k, _vp) for k in ("desc1", "desc2", "pts1", "pts2")]


class LcFuseRows(C.Structure):
    _fields_ = [(k, _vp) for k in ("desc0", "desc1", "pts0", "pts1")]


proto("plslam_map_lists_refresh", [_vp, _vp, _vp])
proto("plslam_map_insert_carry", [_vp, _vp, _vp, _vp, _vp, _vp, _vp])
proto("plslam_lc_fuse_carry", [_vp, _vp, _vp, _vp, _vp, _vp, _vp])


def _fields_of(kind):
    return [f for f in FIELDS if f != "pts" or kind == "lines"]


class DeviceMapLists:
    """The lists of a map on the device with room to grow: `lists` (the dict synthetic_lists returns; None: nothing to upload)
    padded to the capacities in landmarks / observations per kind -- those of the DeviceMapImage they go with.  blank: every
    buffer is filled with that BYTE instead (a destination whose every live row the call must write).  .struct is the
    plslam_map_lists; .counts[kind] = (n, n_obs) says how much of the buffers is live (set by MapLists' calls)."""

    def __init__(self, lists=None, pt_cap=None, pt_obs_cap=None, ls_cap=None, ls_obs_cap=None, device: int = 0, blank=None):
        import torch
        self._t, self.counts = {}, {}
        dev = torch.device("cuda", device)
        kinds = []
        for kind, cap, ocap in (("points", pt_cap, pt_obs_cap), ("lines", ls_cap, ls_obs_cap)):
            L = (lists or {}).get(kind) or {}
            n = int(np.asarray(L["med_idx"]).size) if "med_idx" in L else 0
            n_obs = int(np.asarray(L["desc"]).reshape(-1, 32).shape[0]) if "desc" in L else 0
            cap, ocap = max(n if cap is None else int(cap), 0), max(n_obs if ocap is None else int(ocap), 0)
            self.counts[kind] = (0, 0) if blank is not None else (min(n, cap), min(n_obs, ocap))
            ptrs = {}
            for f in _fields_of(kind):
                dt, w, per_obs = _SHAPE[f]
                rows = ocap if per_obs else cap
                a = np.zeros((max(rows, 1), w), dt)               # (an empty array still gets an address)
                if blank is not None:
                    a.view(np.uint8)[:] = blank
                elif f in L:
                    src = np.asarray(L[f], dt).reshape(-1, w)[:rows]
                    a[:src.shape[0]] = src
                t = torch.from_numpy(a).to(dev)
                self._t[f"{kind}.{f}"] = (t, rows, w)
                ptrs[f] = t.data_ptr()
            kinds.append(MapListsKind(*[ptrs.get(f) for f in FIELDS]))
        self.struct = MapListsStruct(*kinds)
        self.caps = dict(points=(self._t["points.med_idx"][1], self._t["points.desc"][1]), lines=(self._t["lines.med_idx"][1], self._t["lines.desc"][1]))
        torch.cuda.synchronize(dev)

    def ptr(self, name: str) -> int:
        return self._t[name][0].data_ptr()

    def raw(self, name: str) -> np.ndarray:
        """the whole buffer, capacity and all, as rows (waits for the device: the calls that write it only enqueue)"""
        import torch
        t, rows, w = self._t[name]
        torch.cuda.synchronize(t.device)
        a = t.cpu().numpy()[:rows].copy()
        return a.reshape(-1) if w == 1 else a

    def host(self, name: str) -> np.ndarray:
        """the array's LIVE part (n landmarks / n_obs observations as .counts says)"""
        kind, f = name.split(".")
        n, n_obs = self.counts[kind]
        return self.raw(name)[:n_obs if _SHAPE[f][2] else n]

    def host_lists(self) -> dict:
        return {kind: {f: self.host(f"{kind}.{f}") for f in _fields_of(kind)} for kind in ("points", "lines")}


class DeviceRows:
    """A keyframe's rows (insert: desc1 / desc2, lines pts1 / pts2) or a fusion's per-tuple rows (desc0 / desc1, pts0 / pts1) on the
    device: rows = dict(points / lines: dict of host arrays, or None)."""

    def __init__(self, rows, names, struct, device: int = 0):
        import torch
        dev = torch.device("cuda", device)
        self._keep, self.structs = [], []
        for kind in ("points", "lines"):
            R = (rows or {}).get(kind)
            if R is None:
                self.structs.append(None)
                continue
            p = []
            for f in names:
                a = R.get(f)
                if a is None or (f.startswith("pts") and kind == "points"):
                    p.append(None)
                    continue
                dt, w = (np.uint8, 32) if f.startswith("desc") else (np.float64, 4)
                a = np.ascontiguousarray(a, dt).reshape(-1, w)
                t = torch.from_numpy(a.copy() if a.size else np.zeros((1, w), dt)).to(dev)
                self._keep.append(t)
                p.append(t.data_ptr())
            self.structs.append(struct(*p))
        torch.cuda.synchronize(dev)

    def addresses(self):
        return [C.addressof(s) if s is not None else None for s in self.structs]


def insert_rows(rows, device: int = 0) -> DeviceRows:
    return DeviceRows(rows, ("desc1", "desc2", "pts1", "pts2"), MapInsertRows, device)


def fuse_rows(rows, device: int = 0) -> DeviceRows:
    return DeviceRows(rows, ("desc0", "desc1", "pts0", "pts1"), LcFuseRows, device)


class MapLists:
    """The three calls.  Each one ENQUEUES on the context's stream; sync() waits (the host() of a DeviceMapLists does too)."""

    def __init__(self, ctx: Context):
        self._L, self._ctx = ctx._L, ctx

    def refresh(self, image, lists: DeviceMapLists) -> None:
        """plslam_map_lists_refresh: med_idx / med_desc of every landmark of `image` from lists.desc"""
        _check(self._L.plslam_map_lists_refresh(self._ctx.handle, C.addressof(image.struct), C.addressof(lists.struct)),
               "plslam_map_lists_refresh")
        lists.counts = {k: (L.n, L.n_obs) for k, L in (("points", image.struct.points), ("lines", image.struct.lines))}

    def _carry(self, fn, name, handle, src, src_lists, dst, dst_lists, rows: DeviceRows):
        _check(fn(handle, C.addressof(src.struct), C.addressof(src_lists.struct), C.addressof(dst.struct), C.addressof(dst_lists.struct),
                  *rows.addresses()), name)
        dst_lists.counts = {k: (L.n, L.n_obs) for k, L in (("points", dst.struct.points), ("lines", dst.struct.lines))}

    def insert_carry(self, mi, src, src_lists, dst, dst_lists, rows) -> None:
        """plslam_map_insert_carry after mi.kf2kf / mi.map2kf(src, dst, kf); rows: insert_rows(...) or the dict it takes"""
        rows = rows if isinstance(rows, DeviceRows) else insert_rows(rows, self._ctx.device)
        self._carry(self._L.plslam_map_insert_carry, "plslam_map_insert_carry", mi._h, src, src_lists, dst, dst_lists, rows)
        self._keep = rows

    def fuse_carry(self, lf, src, src_lists, dst, dst_lists, rows) -> None:
        """plslam_lc_fuse_carry after lf.run(src, dst, lc); rows: fuse_rows(...) or the dict it takes"""
        rows = rows if isinstance(rows, DeviceRows) else fuse_rows(rows, self._ctx.device)
        self._carry(self._L.plslam_lc_fuse_carry, "plslam_lc_fuse_carry", lf._h, src, src_lists, dst, dst_lists, rows)
        self._keep = rows

    def sync(self) -> None:
        import torch
        torch.cuda.synchronize(torch.device("cuda", self._ctx.device))


# ---- the seeded generators ----------------------------------------------------------------------------------------------------
_POP = np.array([bin(i).count("1") for i in range(256)], np.int32)


def representative(desc, off):
    """MapPoint::updateAverageDescDir's descriptor part (src/mapFeatures.cpp:51-84) for CSR lists: per landmark the row whose
    sorted distances have the smallest element int(1 + 0.5 (n - 1)), the first row on ties -> (med_idx (n,) int32: -1 for an empty
    list, med_desc (n, 32)).  Landmarks of one length are worked together."""
    desc, off = np.asarray(desc, np.uint8).reshape(-1, 32), np.asarray(off, np.int64)
    lens = np.diff(off)
    idx = np.full(lens.size, -1, np.int32)
    idx[lens == 1] = 0
    for n in np.unique(lens[lens > 1]):
        lm = np.flatnonzero(lens == n)
        k = int(1 + 0.5 * (n - 1))
        for c0 in range(0, lm.size, 4096):                        # (bounded working set: lm x n x n x 32 bytes)
            sel = lm[c0:c0 + 4096]
            rows = desc[off[sel][:, None] + np.arange(n)[None, :]]                   # (L, n, 32)
            D = _POP[rows[:, :, None, :] ^ rows[:, None, :, :]].sum(axis=3)          # (L, n, n)
            idx[sel] = np.argmin(np.sort(D, axis=2)[:, :, k], axis=1)                # (argmin: the first of equal values)
    med = np.zeros((lens.size, 32), np.uint8)
    has = idx >= 0
    med[has] = desc[off[:-1][has] + idx[has]]
    return idx, med


def _unit(rng, n):
    v = rng.standard_normal((n, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def _noise(rng, n, clustered):
    if clustered:                                                 # four patterns: equal rows and equal distances are common
        return np.packbits(rng.random((4, 256)) < 0.08, axis=1)[rng.integers(0, 4, n)]
    return np.packbits(rng.random((n, 256)) < 0.08, axis=1)


def synthetic_lists(m, seed=1, clustered=False, with_med=True) -> dict:
    """the lists of the map m (plslam_amd.local_map.synthetic_map or any image dict): per kind desc (n_obs, 32): a base row per
    landmark with a few flipped bits per observation (clustered: the flips come from four patterns, so that distance ties occur),
    dir (n_obs, 3) unit vectors, lines pts (n_obs, 4), and med_idx / med_desc = representative() (with_med=False: zeros, for a
    caller that computes them with MapLists.refresh).  The same seed gives the same lists."""
    rng = np.random.Generator(np.random.PCG64(seed))
    out = {}
    for kind in ("points", "lines"):
        ptr = np.asarray(m[kind]["obs_ptr"], np.int64)
        lens, n_obs = np.diff(ptr), int(ptr[-1]) if ptr.size else 0
        desc = np.ascontiguousarray(np.repeat(random_desc(rng, lens.size), lens, axis=0) ^ _noise(rng, n_obs, clustered)).reshape(-1, 32)
        out[kind] = dict(desc=desc, dir=_unit(rng, n_obs))
        if kind == "lines":
            out[kind]["pts"] = rng.uniform(0.0, 700.0, (n_obs, 4))
        out[kind]["med_idx"], out[kind]["med_desc"] = representative(desc, ptr) if with_med else (np.zeros(lens.size, np.int32), np.zeros((lens.size, 32), np.uint8))
    return out


def _rows(rng, n, lines, clustered, names):
    pool = random_desc(rng, 3)
    out = {}
    for f in names[:2]:
        out[f] = pool[rng.integers(0, 3, n)] ^ _noise(rng, n, True) if clustered else random_desc(rng, n)
    if lines:
        for f in names[2:]:
            out[f] = rng.uniform(0.0, 700.0, (n, 4))
    return out


def keyframe_rows(kf, seed=1, clustered=False) -> dict:
    """the rows of the keyframes of an insert (plslam_amd.map_insert.synthetic_keyframe's kf, or synthetic_map2kf's): per kind
    desc1 (n_prev, 32) / desc2 (n_curr, 32), lines pts1 / pts2 (x 4); clustered: few distinct rows.  A map2kf kf (no P1) gets
    desc2 / pts2 only; a kind without a table gets None."""
    rng = np.random.Generator(np.random.PCG64(seed))
    out = {}
    for kind in ("points", "lines"):
        K = kf.get(kind)
        if K is None:
            out[kind] = None
            continue
        n2 = np.asarray(K["P2"]).shape[0]
        r = _rows(rng, n2, kind == "lines", clustered, ("desc2", "desc2", "pts2", "pts2"))
        if K.get("P1") is not None:
            r.update(_rows(rng, np.asarray(K["P1"]).shape[0], kind == "lines", clustered, ("desc1", "desc1", "pts1", "pts1")))
        out[kind] = r
    return out


def tuple_rows(lc, seed=1, clustered=False) -> dict:
    """the per-tuple rows of a fusion (plslam_amd.lc_fuse.pack_loop_closure's lc): per kind desc0 / desc1 (m, 32), lines pts0 /
    pts1 (m, 4); a kind without tuples gets None"""
    rng = np.random.Generator(np.random.PCG64(seed))
    out = {}
    for kind in ("points", "lines"):
        K = lc.get(kind)
        out[kind] = None if K is None else _rows(rng, np.asarray(K["tuples"]).reshape(-1, 4).shape[0], kind == "lines", clustered,
                                                 ("desc0", "desc1", "pts0", "pts1"))
    return out
