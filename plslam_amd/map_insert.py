"""A keyframe's matches into the device-resident map (plslam_map_insert_*, include/plslam_hip.h): the four insertion loops of
MapHandler::addKeyFrame (src/mapHandler.cpp:280-360, :428-527, :601-629, :716-749) over the CSR image of plslam_amd.local_map,
out of place.

Three parts: the ctypes structs; DeviceMapImage, a DeviceMapIndex with capacities (a source or a destination of an insert; LocalMap
takes it as it takes a DeviceMapIndex) and MapInsert, the handle; and the SEEDED generators synthetic_keyframe /
synthetic_map2kf, which append a keyframe to a synthetic_map and make the tables with a requested mix of branches."""
from __future__ import annotations

import ctypes as C

import numpy as np

from ._lib import Handle, _check, _p, proto
from .local_map import FEAT_NULL, LOOKBACK_TILE, DeviceMapIndex, MapIndex  # noqa: F401 (LOOKBACK_TILE: for the case tables)

MAX_TABLE = 65536         # include/plslam_hip.h: PLSLAM_MAP_INSERT_MAX_TABLE

_vp, _i32 = C.c_void_p, C.c_int32
_KIND_WIDTHS = dict(valid=1, inlier=1, X=None, obs_ptr=1, obs_kf=1, obs_val=None)


class MapInsertKind(C.Structure):
    _fields_ = [("table", _vp), ("n_table", _i32), ("n_prev", _i32), ("n_curr", _i32), ("P1", _vp), ("obs1", _vp), ("P2", _vp),
                ("obs2", _vp)]


class MapInsertDst(C.Structure):
    _fields_ = [("map", MapIndex), ("pt_cap", _i32), ("pt_obs_cap", _i32), ("ls_cap", _i32), ("ls_obs_cap", _i32)]


class MapInsertKindCounts(C.Structure):
    _fields_ = [(k, _i32) for k in ("n_events", "n_new", "n_appended", "n_skipped")]


class MapInsertCounts(C.Structure):
    _fields_ = [("points", MapInsertKindCounts), ("lines", MapInsertKindCounts)]


class MapInsertEvents(C.Structure):
    _fields_ = [("pt_ev", _vp), ("ls_ev", _vp), ("pt_dir", _vp), ("ls_dir", _vp), ("stream", _vp), ("pt_obs_src", _vp),
                ("ls_obs_src", _vp)]


def insert_bounds(m, kf, mode: str) -> dict:
    """the capacities an insert of `kf` into `m` needs, from the tables alone (m = entries i2 >= 0): kf2kf n + m landmarks and
    n_obs + 2 m observations, map2kf n and n_obs + m"""
    out = {}
    for kind, tag in (("points", "pt"), ("lines", "ls")):
        t = (kf.get(kind) or {}).get("table")
        e = 0 if t is None else int((np.asarray(t) >= 0).sum())
        out[tag + "_cap"] = int(m[kind]["n"]) + (e if mode == "kf2kf" else 0)
        out[tag + "_obs_cap"] = int(np.asarray(m[kind]["obs_kf"]).size) + (2 if mode == "kf2kf" else 1) * e
    return out


class DeviceMapImage(DeviceMapIndex):
    """A map image on the device with room to grow: the arrays of `m` uploaded (DeviceMapIndex's upload) padded to the given
    capacities in landmarks / observations per kind.  .struct is the plslam_map_index (as DeviceMapIndex's), .dst the
    plslam_map_insert_dst over the same buffers.  blank: the landmark and observation arrays and feat_idx are filled with
    `blank` instead of m's values (a destination whose every byte the call must write)."""

    def __init__(self, m, pt_cap=None, pt_obs_cap=None, ls_cap=None, ls_obs_cap=None, device: int = 0, blank=None):
        caps = {}
        padded = dict(n_map_kf=m["n_map_kf"], kf_valid=m["kf_valid"], x_kf_w=m["x_kf_w"])
        for kind, cap, ocap in (("points", pt_cap, pt_obs_cap), ("lines", ls_cap, ls_obs_cap)):
            k = m[kind]
            n, n_obs = int(np.asarray(k["valid"]).size), int(np.asarray(k["obs_kf"]).size)
            cap, ocap = max(n if cap is None else int(cap), 0), max(n_obs if ocap is None else int(ocap), 0)
            caps[kind] = (cap, ocap, n, n_obs)
            dl, dv = np.asarray(k["X"]).reshape(n, -1).shape[1] if n else (3 if kind == "points" else 6), 2 if kind == "points" else 3

            def pad(a, rows, width, dt):
                out = np.zeros((rows, width), dt)
                if blank is not None:
                    out[:] = blank
                else:
                    a = np.asarray(a, dt).reshape(-1, width)[:rows]
                    out[:a.shape[0]] = a
                return out

            feat_idx = np.asarray(k["feat_idx"], np.int32)
            padded[kind] = dict(valid=pad(k["valid"], cap, 1, np.uint8), inlier=pad(k["inlier"], cap, 1, np.uint8),
                                X=pad(k["X"], cap, dl, np.float64), obs_ptr=pad(k["obs_ptr"], cap + 1, 1, np.int32),
                                obs_kf=pad(k["obs_kf"], ocap, 1, np.int32), obs_val=pad(k["obs_val"], ocap, dv, np.float64),
                                feat_ptr=k["feat_ptr"], feat_idx=np.full_like(feat_idx, blank) if blank is not None else feat_idx)
        super().__init__(padded, device)
        s = self.struct
        self._widths = {}
        for kind, L in (("points", s.points), ("lines", s.lines)):
            cap, ocap, n, n_obs = caps[kind]
            L.n, L.n_obs = (0, 0) if blank is not None else (min(n, cap), min(n_obs, ocap))
            self._widths[kind] = (padded[kind]["X"].shape[1], padded[kind]["obs_val"].shape[1])
        self.dst = MapInsertDst(s, caps["points"][0], caps["points"][1], caps["lines"][0], caps["lines"][1])
        self.struct = self.dst.map                       # (a view of the dst's own copy: what the call updates)

    def host(self, name: str) -> np.ndarray:
        """the array's LIVE part (n landmarks / n_obs observations as the struct now says), shaped as the map dict's"""
        t, size = self._t[name]
        a = t.cpu().numpy()[:size].copy()
        if "." not in name:
            return a
        kind, f = name.split(".")
        L = self.struct.points if kind == "points" else self.struct.lines
        dl, dv = self._widths[kind]
        rows = dict(valid=L.n, inlier=L.n, X=L.n * dl, obs_ptr=L.n + 1, obs_kf=L.n_obs, obs_val=L.n_obs * dv).get(f, size)
        a = a[:rows]
        return a.reshape(-1, dl) if f == "X" else a.reshape(-1, dv) if f == "obs_val" else a

    def raw(self, name: str) -> np.ndarray:
        """the whole buffer, capacity and all"""
        t, size = self._t[name]
        return t.cpu().numpy()[:size].copy()

    def host_map(self, like) -> dict:
        """the image as a map dict (row and the other host-only entries from `like`)"""
        m = {k: v for k, v in like.items() if k not in ("points", "lines")}
        for kind in ("points", "lines"):
            m[kind] = {f: self.host(f"{kind}.{f}") for f in ("valid", "inlier", "X", "obs_ptr", "obs_kf", "obs_val", "feat_ptr", "feat_idx")}
            m[kind]["n"] = int(m[kind]["valid"].size)
        return m


def _kind_struct(k, mode):
    """-> (MapInsertKind or None, the arrays kept alive)"""
    if not k or k.get("table") is None:
        return None, ()
    tab = np.ascontiguousarray(k["table"], np.int32).reshape(-1)
    P2, o2 = np.ascontiguousarray(k["P2"], np.float64), np.ascontiguousarray(k["obs2"], np.float64)
    keep = [tab, P2, o2]
    s = MapInsertKind(_p(tab) if tab.size else None, tab.size, 0, P2.shape[0], None, None, _p(P2) if P2.size else None,
                      _p(o2) if o2.size else None)
    if mode == "kf2kf":
        P1, o1 = np.ascontiguousarray(k["P1"], np.float64), np.ascontiguousarray(k["obs1"], np.float64)
        keep += [P1, o1]
        s.n_prev, s.P1, s.obs1 = P1.shape[0], (_p(P1) if P1.size else None), (_p(o1) if o1.size else None)
    return s, keep


proto("plslam_map_insert_create", [_vp, C.POINTER(_vp)])
proto("plslam_map_insert_kf2kf", [_vp, _vp, _vp, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp])
proto("plslam_map_insert_map2kf", [_vp, _vp, _vp, _i32, _vp, _vp, _vp, _vp, _vp])
proto("plslam_map_insert_device_buffers", [_vp, _vp])
proto("plslam_map_insert_download", [_vp, _vp])
proto("plslam_map_insert_destroy", [_vp], None)


class MapInsert(Handle):
    """plslam_map_insert: the handle that owns the scratch and the event records of kf2kf / map2kf."""

    def __init__(self, ctx: Context):
        h = C.c_void_p()
        _check(ctx._L.plslam_map_insert_create(ctx.handle, C.byref(h)), "plslam_map_insert_create")
        self._open(ctx, "plslam_map_insert_destroy", h)
        self._n_ev = (0, 0)
        self._n_obs = (0, 0)

    def _call(self, mode, src, dst: DeviceMapImage, kf) -> dict:
        ks, keep = [], []
        for kind in ("points", "lines"):
            s, k = _kind_struct(kf.get(kind), mode)
            ks.append(s)
            keep.append(k)
        row = np.zeros(src.n_map_kf, np.int32)
        c = MapInsertCounts()
        T2 = np.ascontiguousarray(kf["T2"], np.float64).reshape(16)
        args = [C.addressof(k) if k is not None else None for k in ks] + [_p(row), C.addressof(c)]
        if mode == "kf2kf":
            T1 = np.ascontiguousarray(kf["T1"], np.float64).reshape(16)
            rc = self._L.plslam_map_insert_kf2kf(self._h, C.addressof(src.struct), C.addressof(dst.dst), int(kf["kf1"]), int(kf["kf2"]),
                                                 _p(T1), _p(T2), *args)
        else:
            rc = self._L.plslam_map_insert_map2kf(self._h, C.addressof(src.struct), C.addressof(dst.dst), int(kf["kf2"]), _p(T2), *args)
        _check(rc, "plslam_map_insert_" + mode)
        dst.n_map_kf = dst.struct.n_map_kf
        out = dict(row_delta=row)
        for kind, kc in (("points", c.points), ("lines", c.lines)):
            out[kind] = dict(n_events=kc.n_events, n_new=kc.n_new, n_appended=kc.n_appended, n_skipped=kc.n_skipped)
        self._n_ev = (c.points.n_events, c.lines.n_events)
        self._n_obs = (dst.struct.points.n_obs, dst.struct.lines.n_obs)
        return out

    def kf2kf(self, src, dst: DeviceMapImage, kf) -> dict:
        """kf: dict(kf1, kf2, T1, T2 (4 x 4), points / lines: dict(table, P1, obs1, P2, obs2) or None) -> dict(points / lines: the
        counts, row_delta); dst's struct then describes the new image"""
        return self._call("kf2kf", src, dst, kf)

    def map2kf(self, src, dst: DeviceMapImage, kf) -> dict:
        """kf: dict(kf2, T2, points / lines: dict(table = map_to_kf, P2, obs2) or None)"""
        return self._call("map2kf", src, dst, kf)

    def device_buffers(self) -> dict:
        b = MapInsertEvents()
        _check(self._L.plslam_map_insert_device_buffers(self._h, C.addressof(b)), "plslam_map_insert_device_buffers")
        return {k: (getattr(b, k) or 0) for k, _ in MapInsertEvents._fields_}

    def download(self) -> dict:
        """the records of the last insert: dict(points / lines: dict(ev (n, 4) int32, dir (n, 6) float64, obs_src (n_obs,) int32))"""
        out, b = {}, MapInsertEvents()
        for kind, tag, n, n_obs in (("points", "pt", self._n_ev[0], self._n_obs[0]), ("lines", "ls", self._n_ev[1], self._n_obs[1])):
            out[kind] = dict(ev=np.zeros((n, 4), np.int32), dir=np.zeros((n, 6), np.float64), obs_src=np.zeros(n_obs, np.int32))
            if n:
                setattr(b, tag + "_ev", _p(out[kind]["ev"]))
                setattr(b, tag + "_dir", _p(out[kind]["dir"]))
            if n_obs:
                setattr(b, tag + "_obs_src", _p(out[kind]["obs_src"]))
        _check(self._L.plslam_map_insert_download(self._h, C.addressof(b)), "plslam_map_insert_download")
        return out


# ---- the seeded generators ----------------------------------------------------------------------------------------------------
def _pose(rng):
    q, _ = np.linalg.qr(rng.standard_normal((3, 3)))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = q, rng.uniform(-2.0, 2.0, 3)
    return T


def _positions(rng, n, dl):
    return rng.uniform(-3.0, 3.0, (n, dl)) + np.tile([0.0, 0.0, 8.0], dl // 3)


_MIX = dict(n_new=0, n_exist=0, n_invalid=0, n_out_of_range=0, n_null1=0, n_null2=0, n_same_lm=0, n_same_i2=0, n_empty=0,
            n_i2_out_of_range=0, genuine=0.0)


def synthetic_keyframe(m, n_pt=96, n_ls=32, seed=1, points=None, lines=None):
    """-> (map, kf): `map` is m with keyframe slot kf2 = n_map_kf appended (n_pt / n_ls features at -1, n_null2 of them
    PLSLAM_FEAT_NULL; row gets a 0) and with the matched features appended to kf1 = the LAST slot of m (which must be valid);
    kf = dict(kf1, kf2, T1, T2, points / lines: dict(table = matches_12, P1, obs1, P2, obs2)).  points / lines: the mix, a dict
    of counts of table entries per branch (None: no table for the kind):
      n_new a feature at -1; n_exist a valid landmark; n_invalid a NULL landmark; n_out_of_range an index >= n; n_null1 /
      n_null2 a NULL feature of kf1 / kf2; n_same_lm PAIRS of features that name one valid landmark; n_same_i2 extra n_exist-like
      entries that repeat another entry's i2; n_empty valid landmarks WITHOUT observations; n_i2_out_of_range an i2 beyond the
      keyframe; genuine: the probability that a feature kf1 had before is matched too (whatever it names).
    The entries are shuffled among kf1's appended features.  The same seed gives the same keyframe."""
    rng = np.random.Generator(np.random.PCG64(seed))
    nk = int(m["n_map_kf"])
    kf1, kf2 = nk - 1, nk
    assert m["kf_valid"][kf1]
    out = dict(n_map_kf=nk + 1, kf_valid=np.append(m["kf_valid"], np.uint8(1)), x_kf_w=np.vstack([m["x_kf_w"], rng.standard_normal((1, 6))]),
               row=np.append(m["row"], np.int32(0)))
    kf = dict(kf1=kf1, kf2=kf2, T1=_pose(rng), T2=_pose(rng))
    for kind, n_curr, mix in (("points", n_pt, points), ("lines", n_ls, lines)):
        A = m[kind]
        n, dl, dv = int(A["n"]), A["X"].shape[1], A["obs_val"].shape[1]
        mx = dict(_MIX, **(mix or {}))
        lens = np.diff(A["obs_ptr"])
        ok, bad = np.flatnonzero((A["valid"] == 1) & (lens > 0)), np.flatnonzero(A["valid"] == 0)
        empty = np.flatnonzero((A["valid"] == 1) & (lens == 0))
        n_named = mx["n_exist"] + mx["n_same_lm"] + mx["n_same_i2"]
        assert n_named <= ok.size and mx["n_invalid"] <= bad.size and mx["n_empty"] <= empty.size, (kind, ok.size, bad.size, empty.size)
        named = rng.choice(ok, n_named, replace=False)
        add = np.concatenate([np.full(mx["n_new"], -1), named[:mx["n_exist"]], rng.choice(bad, mx["n_invalid"], replace=False),
                              n + 7 + np.arange(mx["n_out_of_range"]), np.full(mx["n_null1"], FEAT_NULL),
                              np.repeat(named[mx["n_exist"]:mx["n_exist"] + mx["n_same_lm"]], 2), named[mx["n_exist"] + mx["n_same_lm"]:],
                              rng.choice(empty, mx["n_empty"], replace=False), np.full(mx["n_null2"] + mx["n_i2_out_of_range"], -1)]).astype(np.int32)
        # what each appended entry's i2 is: 0 a fresh feature of kf2, 1 another entry's, 2 a NULL feature of kf2, 3 beyond it
        how = np.zeros(add.size, np.int64)
        n_tail = mx["n_null2"] + mx["n_i2_out_of_range"]
        s0 = add.size - n_tail - mx["n_empty"] - mx["n_same_i2"]
        how[s0:s0 + mx["n_same_i2"]] = 1
        how[add.size - n_tail:add.size - mx["n_i2_out_of_range"]] = 2
        how[add.size - mx["n_i2_out_of_range"]:] = 3
        perm = rng.permutation(add.size)
        add, how = add[perm], how[perm]
        f0, f1 = int(A["feat_ptr"][kf1]), int(A["feat_ptr"][kf1 + 1])
        n_old = f1 - f0
        assert f1 == A["feat_idx"].size                             # (kf1 is the last slot: its features end the array)
        gen = rng.random(n_old) < mx["genuine"] if mix is not None else np.zeros(n_old, bool)
        n_prev = n_old + add.size
        n_fresh = int(gen.sum()) + int((how == 0).sum())
        assert n_fresh + mx["n_null2"] <= n_curr, (kind, n_fresh, n_curr)
        null2 = rng.choice(n_curr, mx["n_null2"], replace=False)
        feat2 = np.full(n_curr, -1, np.int32)
        feat2[null2] = FEAT_NULL
        fresh = rng.permutation(np.flatnonzero(feat2 == -1))[:n_fresh]
        table = np.full(n_prev, -1, np.int32)
        table[np.flatnonzero(gen)] = fresh[:int(gen.sum())]
        table[n_old + np.flatnonzero(how == 0)] = fresh[int(gen.sum()):]
        used = table[table >= 0]
        if (how == 1).any():
            table[n_old + np.flatnonzero(how == 1)] = rng.choice(used, int((how == 1).sum()))
        table[n_old + np.flatnonzero(how == 2)] = null2
        table[n_old + np.flatnonzero(how == 3)] = n_curr + 3
        feat_ptr = np.append(A["feat_ptr"], 0).astype(np.int32)
        feat_ptr[kf1 + 1] = f1 + add.size
        feat_ptr[kf2 + 1] = f1 + add.size + n_curr
        out[kind] = dict(A, feat_ptr=feat_ptr, feat_idx=np.concatenate([A["feat_idx"], add, feat2]).astype(np.int32))
        out[kind].pop("_lists", None)
        kf[kind] = None if mix is None else dict(table=table, P1=_positions(rng, n_prev, dl), obs1=rng.uniform(0.0, 700.0, (n_prev, dv)),
                                                 P2=_positions(rng, n_curr, dl), obs2=rng.uniform(0.0, 700.0, (n_curr, dv)))
    return out, kf


def synthetic_map2kf(m, kf, seed=1, points=None, lines=None, candidates=None):
    """-> kf with map_to_kf tables for the map <-> keyframe pass over `m` (a map that has slot kf["kf2"]; P2 / obs2 are kf's own).
    points / lines: dict(n_events, n_same_i2=0, n_null2=0, n_i2_out_of_range=0, n_invalid=0) or None; the landmarks come from
    `candidates` (dict(points, lines) of masks) where given, else from the valid ones; the i2 from kf2's features still at -1."""
    rng = np.random.Generator(np.random.PCG64(seed))
    out = dict(kf2=kf["kf2"], T2=kf["T2"])
    for kind, mix in (("points", points), ("lines", lines)):
        if mix is None or kf.get(kind) is None:
            out[kind] = None
            continue
        A, kf2 = m[kind], kf["kf2"]
        mx = dict(dict(n_events=0, n_same_i2=0, n_null2=0, n_i2_out_of_range=0, n_invalid=0), **mix)
        feat2 = A["feat_idx"][A["feat_ptr"][kf2]:A["feat_ptr"][kf2 + 1]]
        free, null2 = np.flatnonzero(feat2 == -1), np.flatnonzero(feat2 == FEAT_NULL)
        pool = np.flatnonzero(candidates[kind]) if candidates is not None else np.flatnonzero(A["valid"] == 1)
        n_all = mx["n_events"] + mx["n_same_i2"] + mx["n_null2"] + mx["n_i2_out_of_range"]
        assert n_all <= pool.size and mx["n_events"] <= free.size and mx["n_null2"] <= null2.size, (kind, pool.size, free.size, null2.size)
        lms = rng.choice(pool, n_all, replace=False)
        if mx["n_invalid"]:
            lms = np.append(lms, rng.choice(np.flatnonzero(A["valid"] == 0), mx["n_invalid"], replace=False))
        i2 = rng.choice(free, mx["n_events"] + mx["n_invalid"], replace=False)
        vals = np.concatenate([i2[:mx["n_events"]], rng.choice(i2, mx["n_same_i2"]) if mx["n_same_i2"] else i2[:0],
                               rng.choice(null2, mx["n_null2"], replace=False) if mx["n_null2"] else i2[:0],
                               np.full(mx["n_i2_out_of_range"], feat2.size + 3), i2[mx["n_events"]:]])
        table = np.full(int(A["n"]), -1, np.int32)
        table[lms] = vals
        out[kind] = dict(table=table, P2=kf[kind]["P2"], obs2=kf[kind]["obs2"])
    return out
