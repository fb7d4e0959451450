"""The local map on the device (plslam_local_map_*, include/plslam_hip.h): formLocalMap, the candidate mask of the map <->
keyframe drivers, the gather of localBundleAdjustment and removeBadMapLandmarks (src/mapHandler.cpp:836-968, :547, :1225-1321,
:2705-2786) over a device-resident CSR image of the map.

Two parts: the ctypes binding (DeviceMapIndex uploads a map image with torch and keeps it alive; LocalMap wraps the handle) and a
SEEDED synthetic map generator, synthetic_map, which makes the image as host arrays: keyframes with NULL slots, landmarks with
0..k observations, NULL landmarks still named by features, NULL features, duplicate feature indices and a full_graph row."""
from __future__ import annotations

import ctypes as C

import numpy as np

from ._lib import Handle, _check, _p, proto

FEAT_NULL = -2            # include/plslam_hip.h: PLSLAM_FEAT_NULL
LOOKBACK_TILE = 256       # plslam_amd/csrc/map_image.hpp: MAP_TILE, the items one workgroup of a scan over the image takes

_vp, _i32 = C.c_void_p, C.c_int32


class MapLandmarks(C.Structure):
    _fields_ = [("n", _i32), ("n_obs", _i32), ("valid", _vp), ("inlier", _vp), ("X", _vp), ("obs_ptr", _vp), ("obs_kf", _vp),
                ("obs_val", _vp), ("n_feat", _i32), ("feat_ptr", _vp), ("feat_idx", _vp)]


class MapIndex(C.Structure):
    _fields_ = [("n_map_kf", _i32), ("kf_valid", _vp), ("x_kf_w", _vp), ("points", MapLandmarks), ("lines", MapLandmarks)]


_U8 = ("kf_local", "pt_local", "ls_local", "pt_candidate", "ls_candidate", "pt_removed", "ls_removed")
_I32 = ("kf_list", "pt_list", "ls_list", "pt_obs", "ls_obs", "pt_lm_loc", "pt_kf_loc", "pt_pose_slot", "ls_lm_loc", "ls_kf_loc",
        "ls_pose_slot")
_F64 = ("pt_obs_uv", "ls_l_obs", "X_aux")
_U8_APPLY = ("pt_moved", "ls_moved")       # behind `stream`: appended to plslam_local_map_buffers


class LocalMapBuffers(C.Structure):
    _fields_ = [(k, _vp) for k in _U8 + _I32 + _F64] + [("stream", _vp)] + [(k, _vp) for k in _U8_APPLY]


class LocalMapLbaDst(C.Structure):
    _fields_ = [("pt_X", _vp), ("pt_inlier", _vp), ("ls_X", _vp), ("ls_inlier", _vp)]


class LocalMapCounts(C.Structure):
    _fields_ = [(k, _i32) for k in ("n_kf_local", "n_pt_local", "n_ls_local", "nkf", "npt", "nls", "n_pt_obs", "n_ls_obs", "empty",
                                    "n_pt_removed", "n_ls_removed", "n_pt_moved", "n_ls_moved")]


_KIND_DTYPES = dict(valid=np.uint8, inlier=np.uint8, X=np.float64, obs_ptr=np.int32, obs_kf=np.int32, obs_val=np.float64,
                    feat_ptr=np.int32, feat_idx=np.int32)


class DeviceMapIndex:
    """A map image (the dict synthetic_map returns, or any with the same arrays) uploaded once; .struct is the plslam_map_index
    over the device copies, which the caller owns across keyframes.  host() brings the arrays cull writes back."""

    def __init__(self, m, device: int = 0):
        import torch
        self._t = {}
        dev = torch.device("cuda", device)

        def up(name, a, dt):
            a = np.ascontiguousarray(a, dtype=dt).reshape(-1)
            t = torch.from_numpy(a.copy() if a.size else np.zeros(1, dt)).to(dev)      # (an empty array still gets an address)
            self._t[name] = (t, a.size)
            return t.data_ptr()

        self.n_map_kf = int(m["n_map_kf"])
        kinds = []
        for kind in ("points", "lines"):
            k = m[kind]
            p = {f: up(f"{kind}.{f}", k[f], dt) for f, dt in _KIND_DTYPES.items()}
            n, n_obs, n_feat = int(np.asarray(k["valid"]).size), int(np.asarray(k["obs_kf"]).size), int(np.asarray(k["feat_idx"]).size)
            kinds.append(MapLandmarks(n, n_obs, p["valid"], p["inlier"], p["X"], p["obs_ptr"], p["obs_kf"], p["obs_val"], n_feat,
                                      p["feat_ptr"], p["feat_idx"]))
        self.struct = MapIndex(self.n_map_kf, up("kf_valid", m["kf_valid"], np.uint8), up("x_kf_w", m["x_kf_w"], np.float64),
                               kinds[0], kinds[1])
        torch.cuda.synchronize(dev)

    def ptr(self, name: str) -> int:
        return self._t[name][0].data_ptr()

    def host(self, name: str) -> np.ndarray:
        t, n = self._t[name]
        return t.cpu().numpy()[:n].copy()


_f64 = C.c_double
proto("plslam_local_map_create", [_vp, C.POINTER(_vp)])     # (every struct goes by address)
proto("plslam_local_map_form", [_vp, _vp, _i32, _vp, _i32, _i32, _vp])
proto("plslam_local_map_form_all", [_vp, _vp, _vp])
proto("plslam_local_map_candidates", [_vp, _vp, _i32])
proto("plslam_local_map_gather", [_vp, _vp, _vp])
proto("plslam_local_map_cull", [_vp, _vp, _i32, _i32, _vp])
proto("plslam_local_map_apply_lba", [_vp, _vp, _vp, _f64, _vp])
proto("plslam_local_map_apply_gba", [_vp, _vp, _vp])
proto("plslam_local_map_device_buffers", [_vp, _vp])
proto("plslam_local_map_download", [_vp, _vp])
proto("plslam_local_map_destroy", [_vp], None)


class LocalMap(Handle):
    """plslam_local_map: the handle that owns the scratch and the outputs of form / candidates / gather / cull."""

    def __init__(self, ctx: Context):
        h = C.c_void_p()
        _check(ctx._L.plslam_local_map_create(ctx.handle, C.byref(h)), "plslam_local_map_create")
        self._open(ctx, "plslam_local_map_destroy", h)
        self._dims = None
        self._counts = {}

    def form(self, index: DeviceMapIndex, anchor_kf: int, row, min_lm_cov_graph: int, min_kf_local_map: int) -> dict:
        row = np.ascontiguousarray(row, np.int32).reshape(index.n_map_kf)
        c = LocalMapCounts()
        _check(self._L.plslam_local_map_form(self._h, C.addressof(index.struct), int(anchor_kf), _p(row), int(min_lm_cov_graph),
                                             int(min_kf_local_map), C.addressof(c)), "plslam_local_map_form")
        s = index.struct
        self._dims = dict(kf=s.n_map_kf, pt=s.points.n, ls=s.lines.n)
        self._counts = dict(n_kf_local=c.n_kf_local, n_pt_local=c.n_pt_local, n_ls_local=c.n_ls_local)
        return dict(self._counts)

    def form_all(self, index: DeviceMapIndex) -> dict:
        """The flags of the GLOBAL bundle adjustment's gather (:1995-2092): every non-NULL keyframe and landmark.  It overwrites
        the flags of the last form: cull / candidates afterwards need a new form."""
        c = LocalMapCounts()
        _check(self._L.plslam_local_map_form_all(self._h, C.addressof(index.struct), C.addressof(c)), "plslam_local_map_form_all")
        s = index.struct
        self._dims = dict(kf=s.n_map_kf, pt=s.points.n, ls=s.lines.n)
        self._counts = dict(n_kf_local=c.n_kf_local, n_pt_local=c.n_pt_local, n_ls_local=c.n_ls_local)
        return dict(self._counts)

    def candidates(self, index: DeviceMapIndex, kf2_idx: int) -> None:
        _check(self._L.plslam_local_map_candidates(self._h, C.addressof(index.struct), int(kf2_idx)), "plslam_local_map_candidates")

    def gather(self, index: DeviceMapIndex) -> dict:
        c = LocalMapCounts()
        _check(self._L.plslam_local_map_gather(self._h, C.addressof(index.struct), C.addressof(c)), "plslam_local_map_gather")
        g = dict(nkf=c.nkf, npt=c.npt, nls=c.nls, n_pt_obs=c.n_pt_obs, n_ls_obs=c.n_ls_obs, empty=bool(c.empty))
        self._counts.update(g)
        return g

    def cull(self, index: DeviceMapIndex, max_kf_idx: int, min_lm_obs: int) -> dict:
        c = LocalMapCounts()
        _check(self._L.plslam_local_map_cull(self._h, C.addressof(index.struct), int(max_kf_idx), int(min_lm_obs), C.addressof(c)),
               "plslam_local_map_cull")
        return dict(n_pt_removed=c.n_pt_removed, n_ls_removed=c.n_ls_removed)

    def apply_lba(self, plan, index: DeviceMapIndex, moved_th: float = 0.01) -> dict:
        """The write-back of the local BA (:1828-1855) from `plan`'s resident landmarks into `index`'s own X / inlier arrays, in
        place: a listed landmark that moved by more than moved_th loses its inlier flag, every listed landmark takes the plan's
        estimate.  -> dict(n_pt_moved, n_ls_moved); the masks: download("pt_moved", "ls_moved")."""
        dst = LocalMapLbaDst(index.ptr("points.X"), index.ptr("points.inlier"), index.ptr("lines.X"), index.ptr("lines.inlier"))
        c = LocalMapCounts()
        _check(self._L.plslam_local_map_apply_lba(self._h, plan._h, C.addressof(dst), float(moved_th), C.addressof(c)),
               "plslam_local_map_apply_lba")
        return dict(n_pt_moved=c.n_pt_moved, n_ls_moved=c.n_ls_moved)

    def apply_gba(self, plan, index: DeviceMapIndex) -> None:
        """The write-back of the global BA (:2681-2697) from the GbaPlan's resident landmarks into `index`'s own X arrays, in
        place: every listed landmark takes the plan's estimate; inlier is not touched."""
        dst = LocalMapLbaDst(index.ptr("points.X"), None, index.ptr("lines.X"), None)
        _check(self._L.plslam_local_map_apply_gba(self._h, plan._h, C.addressof(dst)), "plslam_local_map_apply_gba")

    def device_buffers(self) -> dict:
        b = LocalMapBuffers()
        _check(self._L.plslam_local_map_device_buffers(self._h, C.addressof(b)), "plslam_local_map_device_buffers")
        return {k: (getattr(b, k) or 0) for k, _ in LocalMapBuffers._fields_}

    def download(self, *names) -> dict:
        """The named arrays (all of the calls made so far when none is named) as host arrays of their true lengths."""
        d, c = self._dims, self._counts
        if not names:
            names = _U8 + ((_I32 + _F64) if "nkf" in c else ())
        shape = dict(kf_local=(d["kf"],), pt_local=(d["pt"],), ls_local=(d["ls"],), pt_candidate=(d["pt"],), ls_candidate=(d["ls"],),
                     pt_removed=(d["pt"],), ls_removed=(d["ls"],))
        if "nkf" in c:
            po, lo = c["n_pt_obs"], c["n_ls_obs"]
            shape.update(kf_list=(c["nkf"],), pt_list=(c["npt"],), ls_list=(c["nls"],), pt_obs=(po, 6), ls_obs=(lo, 6), pt_lm_loc=(po,),
                         pt_kf_loc=(po,), pt_pose_slot=(po,), ls_lm_loc=(lo,), ls_kf_loc=(lo,), ls_pose_slot=(lo,), pt_obs_uv=(po, 2),
                         ls_l_obs=(lo, 3), X_aux=(6 * c["nkf"] + 3 * c["npt"] + 6 * c["nls"],), pt_moved=(c["npt"],),
                         ls_moved=(c["nls"],))
        out, b = {}, LocalMapBuffers()
        for k in names:
            dt = np.uint8 if k in _U8 + _U8_APPLY else np.int32 if k in _I32 else np.float64
            out[k] = np.zeros(shape[k], dt)
            setattr(b, k, _p(out[k]) if out[k].size else None)
        _check(self._L.plslam_local_map_download(self._h, C.addressof(b)), "plslam_local_map_download")
        return out


def anchor_lists(m, kind):
    """The reference's map_points_kf_idx / map_lines_kf_idx (kind = "points" / "lines") derived from an image dict: slot k lists,
    ascending, the valid landmarks with a non-empty observation list whose FIRST observer is k -- what the containers hold at any
    time in the code the reference runs ("Loop-closure correction on the image").  A first observer outside
    [0, n_map_kf) is listed nowhere.  -> (anchor_ptr (n_map_kf + 1,) int32, anchor_idx int32): plslam_lc_landmarks' CSR."""
    K, nk = m[kind], int(m["n_map_kf"])
    valid, ptr = np.asarray(K["valid"]).reshape(-1), np.asarray(K["obs_ptr"], np.int64).reshape(-1)
    obs_kf = np.asarray(K["obs_kf"], np.int64).reshape(-1)
    n = valid.size
    b, e = ptr[:n], ptr[1:n + 1]
    ok = (valid != 0) & (b >= 0) & (e > b) & (e <= obs_kf.size)
    first = np.full(n, -1, np.int64)
    first[ok] = obs_kf[b[ok]]
    ok &= (first >= 0) & (first < nk)
    j = np.flatnonzero(ok)
    j = j[np.argsort(first[j], kind="stable")]                     # per slot ascending: new indices only grow
    anchor_ptr = np.zeros(nk + 1, np.int32)
    anchor_ptr[1:] = np.cumsum(np.bincount(first[j], minlength=nk))
    return anchor_ptr, j.astype(np.int32)


# ---- the seeded generator -----------------------------------------------------------------------------------------------------
def _kind(rng, n_kf, n, dl, dv, kf_valid, max_obs, null_lm_frac, outlier_frac, n_unmatched, n_null_feat, n_dup, no_obs_frac):
    nobs = rng.integers(1, max_obs + 1, n) if n else np.zeros(0, np.int64)
    nobs[rng.random(n) < no_obs_frac] = 0                                   # a landmark with an empty observation list
    obs_ptr = np.zeros(n + 1, np.int32)
    obs_ptr[1:] = np.cumsum(nobs)
    obs_lm = np.repeat(np.arange(n, dtype=np.int32), nobs)
    obs_kf = rng.integers(0, n_kf, obs_lm.size).astype(np.int32)            # (NULL slots included: a keyframe removed later)
    order = np.lexsort((obs_kf, obs_lm))                                    # list order: ascending keyframes per landmark
    obs_kf = obs_kf[order]
    obs_val = rng.uniform(0.0, 700.0, (obs_lm.size, dv))
    valid = (rng.random(n) >= null_lm_frac).astype(np.uint8)                # a NULL landmark keeps its features' indices
    inlier = (rng.random(n) >= outlier_frac).astype(np.uint8)
    X = rng.uniform(-20.0, 20.0, (n, dl))
    # the features: one per observation in a non-NULL keyframe, unmatched ones (-1), NULL feature pointers, and duplicates of
    # indices already named in the same keyframe; shuffled inside each keyframe
    ok = np.flatnonzero(kf_valid)
    live = kf_valid[obs_kf].astype(bool) if obs_kf.size else np.zeros(0, bool)
    f_kf, f_idx = [obs_kf[live]], [obs_lm[live]]
    if ok.size:
        f_kf += [rng.choice(ok, n_unmatched).astype(np.int32), rng.choice(ok, n_null_feat).astype(np.int32)]
        f_idx += [np.full(n_unmatched, -1, np.int32), np.full(n_null_feat, FEAT_NULL, np.int32)]
        if f_kf[0].size and n_dup:
            pick = rng.integers(0, f_kf[0].size, n_dup)
            f_kf.append(f_kf[0][pick])
            f_idx.append(f_idx[0][pick])
    f_kf, f_idx = np.concatenate(f_kf).astype(np.int32), np.concatenate(f_idx).astype(np.int32)
    perm = rng.permutation(f_kf.size)
    perm = perm[np.argsort(f_kf[perm], kind="stable")]
    feat_ptr = np.zeros(n_kf + 1, np.int32)
    feat_ptr[1:] = np.cumsum(np.bincount(f_kf, minlength=n_kf))
    return dict(n=n, valid=valid, inlier=inlier, X=X, obs_ptr=obs_ptr, obs_kf=obs_kf, obs_val=obs_val, feat_ptr=feat_ptr,
                feat_idx=f_idx[perm])


def synthetic_map(n_kf=40, n_pt=600, n_ls=150, seed=1, max_obs=5, null_kf=(), null_lm_frac=0.05, outlier_frac=0.1,
                  unmatched_frac=0.2, null_feat_frac=0.05, dup_frac=0.05, no_obs_frac=0.03, cov_max=150):
    """-> dict(n_map_kf, kf_valid (n_kf,) uint8, x_kf_w (n_kf, 6), row (n_kf,) int32 = full_graph[n_kf - 1], points, lines); a kind
    is dict(n, valid, inlier, X, obs_ptr, obs_kf, obs_val, feat_ptr, feat_idx) as plslam_map_index lays it out.  The same seed
    gives the same map.  null_kf: NULL keyframe slots (they keep their observations and lose their features); the fractions are
    of the landmark count (features: of the observation count)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    kf_valid = np.ones(n_kf, np.uint8)
    for k in null_kf:
        kf_valid[k] = 0
    kinds = []
    for n, dl, dv in ((n_pt, 3, 2), (n_ls, 6, 3)):
        nf = n * (1 + max_obs) // 2
        kinds.append(_kind(rng, n_kf, n, dl, dv, kf_valid, max_obs, null_lm_frac, outlier_frac, int(nf * unmatched_frac),
                           int(nf * null_feat_frac), int(nf * dup_frac), no_obs_frac))
    row = rng.integers(0, cov_max + 1, n_kf).astype(np.int32)
    return dict(n_map_kf=n_kf, kf_valid=kf_valid, x_kf_w=rng.standard_normal((n_kf, 6)), row=row, points=kinds[0], lines=kinds[1])
