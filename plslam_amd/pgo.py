"""The loop-closure correction (plslam_pgo_*, plslam_lc_correct_map, include/plslam_hip.h): the ctypes binding (PgoPlan,
correct_map, correct_map_dev, envelope_ldlt_solve) and a seeded generator: a map whose stored poses drifted.

The true keyframes run around a circle of `period` keyframes and carry on into a second lap, so that keyframe k >= period is
back where keyframe k - period was.  The stored poses are the true relative motions composed with small errors (accumulated
odometry drift).  full_graph counts landmarks shared inside a window of consecutive keyframes, so that the nearest neighbours
pass min_lm_cov_graph = 75 and farther ones do not.  Each loop closure (a, b) with b = a + period carries the true relative
pose plus noise, as x with expmap_se3(x) = T_a^-1 T_b: the measurement of the loop edge (src/mapHandler.cpp:4276-4287).
Landmarks are anchored to keyframe slots (map_points_kf_idx / map_lines_kf_idx) as CSR lists, each with a dir_list CSR.

correct_image is the binding of plslam_lc_correct_image: the same correction on a device-resident map image, which needs no
anchor lists (a landmark's anchor is its first observer)."""
from __future__ import annotations

import ctypes as C

import numpy as np

from ._lib import Handle, _arr, _check, _p, proto
from .synth import se3_exp

PGO_STOP_MAX_ITERS, PGO_STOP_TERMINATE = 0, 1


class PgoParams(C.Structure):
    """plslam_pgo_params"""
    _fields_ = [("min_lm_ess_graph", C.c_int32), ("min_lm_cov_graph", C.c_int32), ("max_iters_pgo", C.c_int32),
                ("max_trials", C.c_int32), ("lambda_init", C.c_double)]


class PgoTrial(C.Structure):
    """plslam_pgo_trial: one record per trial of plslam_pgo_optimize"""
    _fields_ = [("iteration", C.c_int32), ("trial", C.c_int32), ("lambda_", C.c_double), ("chi", C.c_double),
                ("chi_new", C.c_double), ("scale", C.c_double), ("rho", C.c_double), ("ok", C.c_int32), ("accepted", C.c_int32)]


class PgoResult(C.Structure):
    """plslam_pgo_result"""
    _fields_ = [("iterations", C.c_int32), ("trials", C.c_int32), ("stop_reason", C.c_int32), ("n_vertices", C.c_int32),
                ("n_active", C.c_int32), ("n_edges", C.c_int32), ("n_lc_edges", C.c_int32), ("env_width", C.c_int32),
                ("env_entries", C.c_int64), ("chi_initial", C.c_double), ("chi_final", C.c_double), ("lambda_", C.c_double)]


class LcLandmarks(C.Structure):
    """plslam_lc_landmarks"""
    _fields_ = [("n", C.c_int32), ("n_anchor", C.c_int32), ("n_dir", C.c_int32), ("anchor_ptr", C.c_void_p),
                ("anchor_idx", C.c_void_p), ("valid", C.c_void_p), ("X", C.c_void_p), ("med_dir", C.c_void_p),
                ("dir_ptr", C.c_void_p), ("dirs", C.c_void_p)]


class LcImageDst(C.Structure):
    """plslam_lc_image_dst: writable device pointers (None: that array is not carried)"""
    _fields_ = [(k, C.c_void_p) for k in ("pt_X", "pt_dir", "pt_med_dir", "ls_X", "ls_dir", "ls_med_dir", "x_kf_w")]


class LcImageCounts(C.Structure):
    _fields_ = [(k, C.c_int32) for k in ("n_pt", "n_ls", "n_pt_dirs", "n_ls_dirs")]


_vp, _i32 = C.c_void_p, C.c_int32
proto("plslam_pgo_plan_create", [_vp, C.POINTER(PgoParams), _i32, _vp, _vp, _i32, _vp, C.POINTER(_vp)])
proto("plslam_pgo_optimize", [_vp] + [_vp] * 7 + [C.POINTER(PgoTrial), _i32, C.POINTER(PgoResult)])
proto("plslam_pgo_plan_destroy", [_vp], None)
proto("plslam_lc_correct_map", [_vp, _i32, _vp, _vp, C.POINTER(LcLandmarks), C.POINTER(LcLandmarks)])
proto("plslam_lc_correct_map_dev", [_vp, _i32, _vp, _vp, C.POINTER(LcLandmarks), C.POINTER(LcLandmarks), _vp])
proto("plslam_lc_correct_image", [_vp, _vp, _vp, _vp, _vp, C.POINTER(LcImageDst), C.POINTER(LcImageCounts)])
proto("plslam_envelope_ldlt_solve", [_vp, _i32, _vp, _vp, _vp, C.POINTER(_i32), C.POINTER(_i32)])


def envelope_ldlt_solve(ctx: Context, A, b):
    """plslam_envelope_ldlt_solve: x with (the lower triangle of A, mirrored) x = b by the envelope L D L^T, in the given
    ordering -> (x, number of zero / non-finite pivots, envelope width)."""
    A = _arr(A, np.float64)
    n = A.shape[0]
    assert A.shape == (n, n)
    bb = _arr(b, np.float64, (n,))
    x, nb, bw = np.empty(n), C.c_int32(0), C.c_int32(0)
    _check(ctx._L.plslam_envelope_ldlt_solve(ctx.handle, n, _p(A), _p(bb), _p(x), C.byref(nb), C.byref(bw)),
           "plslam_envelope_ldlt_solve")
    return x, int(nb.value), int(bw.value)


class PgoPlan(Handle):
    """plslam_pgo_plan: the loop-closure pose graph of the reference (loopClosureOptimizationCovGraphG2O) over one map.

    kf_valid (n,): 0 for a NULL keyframe slot; full_graph (n, n) int32; lc_idx (n_lc, 3)."""

    def __init__(self, ctx: Context, kf_valid, full_graph, lc_idx, min_lm_ess_graph=75, min_lm_cov_graph=75, max_iters_pgo=100,
                 lambda_init=1e-10, max_trials=10):
        v = _arr(kf_valid, np.uint8, (-1,))
        n = v.shape[0]
        fg = _arr(full_graph, np.int32, (n, n))
        lc = _arr(lc_idx, np.int32, (-1, 3))
        self.n_map, self.n_lc = n, lc.shape[0]
        self.params = PgoParams(int(min_lm_ess_graph), int(min_lm_cov_graph), int(max_iters_pgo), int(max_trials),
                                float(lambda_init))
        h = C.c_void_p()
        _check(ctx._L.plslam_pgo_plan_create(ctx.handle, C.byref(self.params), n, _p(v), _p(fg), self.n_lc, _p(lc), C.byref(h)),
               "plslam_pgo_plan_create")
        self._open(ctx, "plslam_pgo_plan_destroy", h)

    def optimize(self, T_kf_w, x_kf_w, lc_pose, trace_cap=4096) -> dict:
        """-> dict(T (n, 4, 4), x (n, 6), T_corr (n, 4, 4), corrected (n,) bool, trace [dict per trial], and the result's
        fields)."""
        n = self.n_map
        T = _arr(T_kf_w, np.float64, (n, 16))
        x = _arr(x_kf_w, np.float64, (n, 6))
        lp = _arr(lc_pose, np.float64, (self.n_lc, 6))
        To, xo, Tc, co = np.empty((n, 4, 4)), np.empty((n, 6)), np.empty((n, 4, 4)), np.empty(n, np.uint8)
        tr = (PgoTrial * max(int(trace_cap), 1))()
        res = PgoResult()
        _check(self._L.plslam_pgo_optimize(self._h, _p(T), _p(x), _p(lp), _p(To), _p(xo), _p(Tc), _p(co), tr, int(trace_cap),
                                           C.byref(res)), "plslam_pgo_optimize")
        trace = [dict(it=t.iteration, trial=t.trial, lam=t.lambda_, chi=t.chi, chi_new=t.chi_new, scale=t.scale, rho=t.rho,
                      ok=bool(t.ok), accepted=bool(t.accepted)) for t in tr[:min(res.trials, int(trace_cap))]]
        out = {f: getattr(res, f) for f, _ in PgoResult._fields_}
        out["lam"] = out.pop("lambda_")
        out.update(T=To, x=xo, T_corr=Tc, corrected=co.astype(bool), trace=trace)
        return out


def _landmarks(lm, dl):
    """host arrays of one kind -> (LcLandmarks over them, the arrays kept alive and written in place)"""
    a = dict(anchor_ptr=_arr(lm["anchor_ptr"], np.int32, (-1,)), anchor_idx=_arr(lm["anchor_idx"], np.int32, (-1,)),
             valid=_arr(lm["valid"], np.uint8, (-1,)), X=np.array(lm["X"], np.float64).reshape(-1, dl),
             med_dir=np.array(lm["med_dir"], np.float64).reshape(-1, 3), dir_ptr=_arr(lm["dir_ptr"], np.int32, (-1,)),
             dirs=np.array(lm["dirs"], np.float64).reshape(-1, 3))
    n = a["valid"].shape[0]
    s = LcLandmarks(n, a["anchor_idx"].shape[0], a["dirs"].shape[0], _p(a["anchor_ptr"]), _p(a["anchor_idx"]), _p(a["valid"]),
                    _p(a["X"]), _p(a["med_dir"]), _p(a["dir_ptr"]), _p(a["dirs"]))
    return s, a


def correct_map(ctx: Context, T_corr, corrected, points=None, lines=None):
    """plslam_lc_correct_map on host arrays: points / lines are dicts (anchor_ptr, anchor_idx, valid, X, med_dir, dir_ptr,
    dirs) as plslam_amd.pgo.anchored_landmarks makes them -> (points, lines) corrected copies (X, med_dir, dirs)."""
    Tc = _arr(T_corr, np.float64, (-1, 16))
    n_map = Tc.shape[0]
    co = _arr(corrected, np.uint8, (n_map,))
    sp = _landmarks(points, 3) if points is not None else None
    sl = _landmarks(lines, 6) if lines is not None else None
    _check(ctx._L.plslam_lc_correct_map(ctx.handle, n_map, _p(Tc), _p(co), C.byref(sp[0]) if sp else None,
                                        C.byref(sl[0]) if sl else None), "plslam_lc_correct_map")
    pick = lambda s: None if s is None else {k: s[1][k] for k in ("X", "med_dir", "dirs")}  # noqa: E731
    return pick(sp), pick(sl)


def correct_map_dev(ctx: Context, n_map_kf, T_corr_ptr, corrected_ptr, points=None, lines=None, stream=0) -> None:
    """plslam_lc_correct_map_dev: points / lines are dicts of device pointers (ints) with the counts n, n_anchor, n_dir."""
    def mk(d):
        return None if d is None else C.byref(LcLandmarks(d["n"], d["n_anchor"], d["n_dir"], d["anchor_ptr"], d["anchor_idx"],
                                                          d["valid"], d["X"], d["med_dir"], d["dir_ptr"], d["dirs"]))
    _check(ctx._L.plslam_lc_correct_map_dev(ctx.handle, int(n_map_kf), C.c_void_p(T_corr_ptr), C.c_void_p(corrected_ptr),
                                            mk(points), mk(lines), C.c_void_p(stream) if stream else None),
           "plslam_lc_correct_map_dev")


# ---- the seeded generator -----------------------------------------------------------------------------------------------------
def _logmap(T):
    R = T[:3, :3]
    c = min(1.0, max(-1.0, (np.trace(R) - 1.0) / 2.0))
    s = np.sqrt(1.0 - c * c)
    th = np.arccos(c)
    w, V = np.zeros(3), np.eye(3)
    if th > 1e-6:
        w = th * np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]]) / (2.0 * s)
        k = w / th
        K = np.array([[0.0, -k[2], k[1]], [k[2], 0.0, -k[0]], [-k[1], k[0], 0.0]])
        V = np.eye(3) + K * (1.0 - c) / th + K @ K * (th - s) / th
    return np.concatenate([np.linalg.solve(V, T[:3, 3]), w])


def _inv(T):
    o = np.eye(4)
    o[:3, :3] = T[:3, :3].T
    o[:3, 3] = -T[:3, :3].T @ T[:3, 3]
    return o


def pose_graph(n_kf=120, n_loops=1, seed=3, period=None, drift=0.003, lc_noise=0.0005, null_slots=(), n_after=3,
               window=4, step=0.3, extra_lc=(), optimized=(), true_poses=None, cov_step=40):
    """-> dict(n_map_kf, kf_valid (n,) uint8, T_kf_w (n, 4, 4) stored, x_kf_w (n, 6) = logmap_se3(T_kf_w), T_true, full_graph
    (n, n) int32, lc_idx (n_lc, 3) int32, lc_pose (n_lc, 6)).

    The loop closures close at n_loops keyframes of the second lap, the last n_after keyframes before the end (those after it
    are the 'later keyframes' of :4358).  extra_lc: more (a, b) entries appended as they are; optimized: indices of LC entries
    whose (2) column is 0 (already optimised; they still make edges).  drift and lc_noise may be 6-vectors (translation, then
    rotation).  true_poses(n_kf, period, step) -> (n_kf, 4, 4) replaces the planar circle; it must return to its start after
    `period` keyframes.  cov_step: the shared-landmark count falls by this much per keyframe of distance, over `window`."""
    rng = np.random.Generator(np.random.PCG64(seed))
    period = period or (max(8, int(round(n_kf * 0.8))) | 1)     # odd: no keyframe at a rotation of exactly pi
    assert n_kf > period + n_after
    R = period * step / (2 * np.pi)
    T_true = np.zeros((n_kf, 4, 4))
    for k in range(n_kf):
        th = 2 * np.pi * k / period
        T = se3_exp(np.array([0.0, 0.0, 0.0, 0.0, th, 0.0]))
        T[:3, 3] = [R * (1 - np.cos(th)), 0.02 * np.sin(3 * th), R * np.sin(th)]
        T_true[k] = T
    if true_poses is not None:
        T_true = np.asarray(true_poses(n_kf, period, step), np.float64).reshape(n_kf, 4, 4)
    drift, lc_noise = np.asarray(drift, np.float64), np.asarray(lc_noise, np.float64)
    T_kf_w = np.zeros_like(T_true)
    T_kf_w[0] = T_true[0]
    for k in range(1, n_kf):
        rel = _inv(T_true[k - 1]) @ T_true[k]
        T_kf_w[k] = T_kf_w[k - 1] @ rel @ se3_exp(drift * rng.standard_normal(6))
    x_kf_w = np.stack([_logmap(T) for T in T_kf_w])
    valid = np.ones(n_kf, np.uint8)
    for k in null_slots:
        valid[k] = 0
    fg = np.zeros((n_kf, n_kf), np.int32)
    for i in range(n_kf):
        for j in range(i + 1, min(n_kf, i + window + 1)):
            c = int(200 - cov_step * (j - i) + rng.integers(-12, 13))
            fg[i, j] = fg[j, i] = max(c, 0)
    fg[valid == 0, :] = 0
    fg[:, valid == 0] = 0
    last = n_kf - 1 - n_after
    bs = set()
    for b in np.linspace(max(period, last - 12 * (n_loops - 1)), last, n_loops).round().astype(int):
        while b > period and not (valid[b] and valid[b - period]):       # a loop closes between two non-NULL keyframes
            b -= 1
        bs.add(int(b))
    bs = sorted(bs)
    pairs = [(b - period, b) for b in bs] + [tuple(p) for p in extra_lc]
    lc_idx = np.array([[a, b, 1] for a, b in pairs], np.int32).reshape(-1, 3)
    for k in optimized:
        lc_idx[k, 2] = 0
    lc_pose = np.stack([_logmap(_inv(T_true[a]) @ T_true[b] @ se3_exp(lc_noise * rng.standard_normal(6))) for a, b in pairs])
    return dict(n_map_kf=n_kf, kf_valid=valid, T_kf_w=T_kf_w, x_kf_w=x_kf_w, T_true=T_true, full_graph=fg, lc_idx=lc_idx,
                lc_pose=lc_pose)


def anchored_landmarks(n_kf, n_lm, n_dir=4, seed=5, line=False, null_frac=0.02, n_double=8, kf_valid=None, vary_dirs=True):
    """Landmarks anchored to keyframe slots -> dict(anchor_ptr (n_kf + 1,), anchor_idx, valid (n_lm,) uint8, X (n_lm, 3 or 6),
    med_dir (n_lm, 3), dir_ptr (n_lm + 1,), dirs (m, 3)).  Each landmark is anchored at one slot (no NULL slot); n_double of
    them are listed under a second, later slot too (as after removeRedundantKFs); null_frac of them are NULL.  Each has 0 ..
    n_dir dir_list entries (exactly n_dir with vary_dirs=False)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    ok = np.flatnonzero(np.ones(n_kf, bool) if kf_valid is None else np.asarray(kf_valid).astype(bool))
    home = np.sort(rng.choice(ok, n_lm))
    lists = [[] for _ in range(n_kf)]
    for j, k in enumerate(home):
        lists[k].append(j)
    for j in rng.choice(n_lm, min(n_double, n_lm), replace=False):
        later = ok[ok > home[j]]
        if later.size:
            lists[int(rng.choice(later))].append(int(j))
    ptr = np.zeros(n_kf + 1, np.int32)
    ptr[1:] = np.cumsum([len(x) for x in lists])
    idx = np.array([j for x in lists for j in x], np.int32)
    valid = (rng.random(n_lm) >= null_frac).astype(np.uint8)
    X = rng.uniform(-20.0, 20.0, (n_lm, 6 if line else 3))
    med = rng.standard_normal((n_lm, 3))
    med /= np.linalg.norm(med, axis=1, keepdims=True)
    nd = rng.integers(0, n_dir + 1, n_lm) if vary_dirs else np.full(n_lm, n_dir)
    dptr = np.zeros(n_lm + 1, np.int32)
    dptr[1:] = np.cumsum(nd)
    dirs = rng.standard_normal((int(dptr[-1]), 3))
    return dict(anchor_ptr=ptr, anchor_idx=idx, valid=valid, X=X, med_dir=med, dir_ptr=dptr, dirs=dirs)


def correct_image(ctx, index, T_corr, corrected, x_kf_w=None, lists=None, med_dir=None) -> dict:
    """plslam_lc_correct_image, in place on a device-resident map: index is a DeviceMapIndex / DeviceMapImage (its X arrays, and
    its x_kf_w where x_kf_w -- the (n_map_kf, 6) x of PgoPlan.optimize -- is given), lists a DeviceMapLists whose dir rows are
    carried (None: no dir), med_dir a dict(points=, lines=) of device addresses of (n, 3) arrays (None: not carried).  T_corr
    (n_map_kf, 4, 4) and corrected (n_map_kf,) are host arrays, as PgoPlan.optimize returns them.
    -> dict(n_pt, n_ls, n_pt_dirs, n_ls_dirs): the corrected landmarks and the transformed dir rows."""
    n = int(index.struct.n_map_kf)
    Tc = _arr(T_corr, np.float64, (n, 16))
    co = _arr(np.asarray(corrected).astype(np.uint8), np.uint8, (n,))
    xn = None if x_kf_w is None else _arr(x_kf_w, np.float64, (n, 6))
    med = med_dir or {}
    dst = LcImageDst(index.ptr("points.X"), lists.ptr("points.dir") if lists is not None else None, med.get("points"),
                     index.ptr("lines.X"), lists.ptr("lines.dir") if lists is not None else None, med.get("lines"),
                     index.ptr("x_kf_w") if xn is not None else None)
    c = LcImageCounts()
    _check(ctx._L.plslam_lc_correct_image(ctx.handle, C.addressof(index.struct), _p(Tc), _p(co), _p(xn), C.byref(dst), C.byref(c)),
           "plslam_lc_correct_image")
    return {k: getattr(c, k) for k, _ in LcImageCounts._fields_}
