"""The global bundle adjustment (plslam_gba_*, include/plslam_hip.h): the ctypes binding (GbaPlan, dense_ldlt_solve) and a seeded
map generator, trajectory_map: a trajectory-shaped map.

synth.local_map gives every landmark random keyframes, so every keyframe pair is covisible and the reduced camera system is
dense.  Here the keyframes lie on a closed circular trajectory and each landmark is seen by a window of consecutive keyframes,
so covisibility is banded; with loop=True windows may wrap past the last keyframe to the first ones (the loop revisit that
links the two ends).  The lists are laid out as MapHandler::globalBundleAdjustment builds them (src/mapHandler.cpp:1995-2099):
keyframe 0 is not optimised (its observations carry keyframe local index -1), every landmark is an unknown with all its
observations, in landmark order."""
from __future__ import annotations

import ctypes as C

import numpy as np

from ._lib import Cam, Handle, _arr, _check, _p, proto
from .synth import EUROC, se3_exp

GBA_MAX_KEYFRAMES = 4096  # include/plslam_hip.h: PLSLAM_GBA_MAX_KEYFRAMES
GBA_STOP_MAX_ITERS, GBA_STOP_ERR, GBA_STOP_DX = 0, 1, 2


class GbaSolve(C.Structure):
    """plslam_gba_solve: one record per solve of plslam_gba_optimize"""
    _fields_ = [("lambda_", C.c_double), ("err_raw", C.c_double), ("err", C.c_double), ("dx_norm", C.c_double),
                ("n_singular", C.c_int32), ("n_bad_pivots", C.c_int32), ("accepted", C.c_int32), ("reserved", C.c_int32)]


class GbaListSizes(C.Structure):
    """plslam_gba_list_sizes"""
    _fields_ = [(k, C.c_int32) for k in ("nkf", "npt", "nls", "n_pt_obs", "n_ls_obs", "nblk", "nchunk", "n_pairs", "n_lpo", "n_llo",
                                         "n_kpo", "n_klo")]


GBA_LIST_NAMES = ("blk", "chk", "pair", "plm", "pkf", "llm", "lkf", "kpp", "kpo", "klp", "klo", "lpp", "lpo", "llp", "llo")


class GbaLists(C.Structure):
    """plslam_gba_lists: host pointers, NULL = skip"""
    _fields_ = [(k, C.c_void_p) for k in GBA_LIST_NAMES]


class GbaResult(C.Structure):
    """plslam_gba_result"""
    _fields_ = [("iters", C.c_int32), ("n_solves", C.c_int32), ("stop_reason", C.c_int32), ("reserved", C.c_int32),
                ("err", C.c_double), ("err_prev", C.c_double), ("lambda_", C.c_double), ("hmax", C.c_double)]


_vp, _i32, _f64 = C.c_void_p, C.c_int32, C.c_double
for _name in ("plslam_gba_plan_create", "plslam_gba_plan_create_dev"):
    proto(_name, [_vp, C.POINTER(Cam), _f64, _i32, _i32, _vp, _i32, _i32, _vp, _vp, _i32, _vp, _vp, _i32, C.POINTER(_vp)])
proto("plslam_gba_plan_list_sizes", [_vp, C.POINTER(GbaListSizes)])
proto("plslam_gba_plan_lists", [_vp, _vp])
proto("plslam_gba_optimize", [_vp, _f64, _f64, _i32] + [_vp] * 8 + [C.POINTER(GbaSolve), C.POINTER(GbaResult)])
proto("plslam_gba_optimize_dev", [_vp, _f64, _f64, _i32] + [_vp] * 6 + [C.POINTER(GbaSolve), C.POINTER(GbaResult)])
proto("plslam_gba_plan_destroy", [_vp], None)
proto("plslam_dense_ldlt_solve", [_vp, _i32, _vp, _vp, _vp, C.POINTER(_i32)])


class GbaPlan(Handle):
    """plslam_gba_plan: the global bundle adjustment of the reference (levMarquardtOptimizationGBA) over one map.

    pt_obs / ls_obs: the reference's Vector6i rows (n, 6) -- landmark map index, landmark local index, observation index,
    keyframe map index, keyframe local index (-1: keyframe 0), inlier flag; pt_uv (n, 2) / ls_l (n, 3) the observations;
    kf_list[k]: the map index of optimised keyframe k."""

    def __init__(self, ctx: Context, cam: Cam, n_map_kf, kf_list, npt, nls, pt_obs, pt_uv, ls_obs, ls_l, homog_th=1e-7):
        kl = _arr(kf_list, np.int32, (-1,))
        po, lo = _arr(pt_obs, np.int32, (-1, 6)), _arr(ls_obs, np.int32, (-1, 6))
        uv, ll = _arr(pt_uv, np.float64, (-1, 2)), _arr(ls_l, np.float64, (-1, 3))
        self.dims = (int(n_map_kf), kl.shape[0], int(npt), int(nls))
        h = C.c_void_p()
        _check(ctx._L.plslam_gba_plan_create(ctx.handle, C.byref(cam), float(homog_th), int(n_map_kf), kl.shape[0], _p(kl),
                                             int(npt), int(nls), _p(po), _p(uv), po.shape[0], _p(lo), _p(ll), lo.shape[0],
                                             C.byref(h)), "plslam_gba_plan_create")
        self._open(ctx, "plslam_gba_plan_destroy", h)

    @classmethod
    def from_device(cls, ctx: Context, cam: Cam, n_map_kf, nkf, d_kf_list, npt, nls, d_pt_obs, d_pt_uv, n_pt_obs, d_ls_obs, d_ls_l,
                    n_ls_obs, homog_th=1e-7):
        """plslam_gba_plan_create_dev: the same plan from DEVICE columns (addresses as ints), e.g. what LocalMap.form_all +
        .gather leave in LocalMap.device_buffers(): kf_list, pt_obs, pt_obs_uv, ls_obs, ls_l_obs."""
        self = cls.__new__(cls)
        self.dims = (int(n_map_kf), int(nkf), int(npt), int(nls))
        h = C.c_void_p()
        _check(ctx._L.plslam_gba_plan_create_dev(ctx.handle, C.byref(cam), float(homog_th), int(n_map_kf), int(nkf),
                                                 d_kf_list or None, int(npt), int(nls), d_pt_obs or None, d_pt_uv or None,
                                                 int(n_pt_obs), d_ls_obs or None, d_ls_l or None, int(n_ls_obs), C.byref(h)),
               "plslam_gba_plan_create_dev")
        self._open(ctx, "plslam_gba_plan_destroy", h)
        return self

    def lists(self) -> dict:
        """The plan's lists as host arrays (plslam_gba_plan_lists): blk (nblk, 4), chk (nchunk, 4), pair (n, 2), plm / pkf /
        llm / lkf and the eight CSR arrays -- of a host-built or a device-built plan."""
        z = GbaListSizes()
        _check(self._L.plslam_gba_plan_list_sizes(self._h, C.byref(z)), "plslam_gba_plan_list_sizes")
        shape = dict(blk=(z.nblk, 4), chk=(z.nchunk, 4), pair=(z.n_pairs, 2), plm=(z.n_pt_obs,), pkf=(z.n_pt_obs,), llm=(z.n_ls_obs,),
                     lkf=(z.n_ls_obs,), kpp=(z.nkf + 1,), kpo=(z.n_kpo,), klp=(z.nkf + 1,), klo=(z.n_klo,), lpp=(z.npt + 1,),
                     lpo=(z.n_lpo,), llp=(z.nls + 1,), llo=(z.n_llo,))
        out, b = {}, GbaLists()
        for k in GBA_LIST_NAMES:
            out[k] = np.zeros(shape[k], np.int32)
            setattr(b, k, _p(out[k]) if out[k].size else None)
        _check(self._L.plslam_gba_plan_lists(self._h, C.addressof(b)), "plslam_gba_plan_lists")
        return out

    def _result(self, tr, res, **state) -> dict:
        trace = [dict(lam=t.lambda_, err_raw=t.err_raw, err=t.err, dx_norm=t.dx_norm, n_singular=t.n_singular,
                      n_bad_pivots=t.n_bad_pivots, accepted=bool(t.accepted)) for t in tr[:res.n_solves]]
        return dict(state, trace=trace, iters=res.iters, n_solves=res.n_solves, stop_reason=res.stop_reason, err=res.err,
                    err_prev=res.err_prev, lam=res.lambda_, hmax=res.hmax)

    def optimize(self, T_kf_w, x_kf, Xw, Lw, lambda_lm=0.00001, lambda_k=10.0, max_iters=15) -> dict:
        """The LM loop -> dict(x_kf (nkf, 6), T (nkf, 4, 4), Xw (npt, 3), Lw (nls, 6), trace (one dict per solve), iters,
        n_solves, stop_reason, err, err_prev, lam, hmax)."""
        n_map, nkf, npt, nls = self.dims
        T = _arr(T_kf_w, np.float64, (n_map, 16))
        x = _arr(x_kf, np.float64, (nkf, 6))
        X, Lm = _arr(Xw, np.float64, (npt, 3)), _arr(Lw, np.float64, (nls, 6))
        xo, To, Xo, Lo = np.empty((nkf, 6)), np.empty((nkf, 4, 4)), np.empty((npt, 3)), np.empty((nls, 6))
        tr = (GbaSolve * max(int(max_iters), 1))()
        res = GbaResult()
        _check(self._L.plslam_gba_optimize(self._h, float(lambda_lm), float(lambda_k), int(max_iters), _p(T), _p(x), _p(X),
                                           _p(Lm), _p(xo), _p(To), _p(Xo), _p(Lo), tr, C.byref(res)), "plslam_gba_optimize")
        return self._result(tr, res, x_kf=xo, T=To, Xw=Xo, Lw=Lo)

    def optimize_dev(self, T_kf_w, d_x_kf, d_Xw, d_Lw, lambda_lm=0.00001, lambda_k=10.0, max_iters=15) -> dict:
        """plslam_gba_optimize_dev: the same loop with x_kf / Xw / Lw as DEVICE addresses (for the gather: X_aux, X_aux + 48 nkf,
        X_aux + 48 nkf + 24 npt bytes); T_kf_w stays a host array.  -> optimize's dict without Xw / Lw: the landmarks stay
        resident in the plan (LocalMap.apply_gba writes them into the map image)."""
        n_map, nkf, _, _ = self.dims
        T = _arr(T_kf_w, np.float64, (n_map, 16))
        xo, To = np.empty((nkf, 6)), np.empty((nkf, 4, 4))
        tr = (GbaSolve * max(int(max_iters), 1))()
        res = GbaResult()
        _check(self._L.plslam_gba_optimize_dev(self._h, float(lambda_lm), float(lambda_k), int(max_iters), _p(T), d_x_kf or None,
                                               d_Xw or None, d_Lw or None, _p(xo), _p(To), tr, C.byref(res)),
               "plslam_gba_optimize_dev")
        return self._result(tr, res, x_kf=xo, T=To)


def dense_ldlt_solve(ctx: Context, A, b):
    """plslam_dense_ldlt_solve: x with (the lower triangle of A, mirrored) x = b on the device -> (x, number of zero /
    non-finite pivots)."""
    A = _arr(A, np.float64)
    n = A.shape[0]
    assert A.shape == (n, n)
    bb = _arr(b, np.float64, (n,))
    x, nb = np.empty(n), C.c_int32(0)
    _check(ctx._L.plslam_dense_ldlt_solve(ctx.handle, n, _p(A), _p(bb), _p(x), C.byref(nb)), "plslam_dense_ldlt_solve")
    return x, int(nb.value)


# ---- the seeded generator -----------------------------------------------------------------------------------------------------

def trajectory_map(n_kf=400, n_pt=40000, n_ls=6000, obs_per_lm=4, loop=True, seed=11, noise_px=1.0, pose_noise=0.002,
                   n_unobserved=0, cam=EUROC, step=0.3):
    """-> dict(n_map_kf, kf_list (nkf,), T_kf_w (n_kf, 16) stored poses, x_kf (nkf, 6) the optimised keyframes' x_kf_w,
    Xw (n_pt, 3), Lw (n_ls, 6), pt_obs / ls_obs (n, 6) int32 Vector6i rows, pt_uv (n, 2), ls_l (n, 3)).

    n_unobserved: that many points and lines in the middle of the lists get no observation (their blocks are singular)."""
    assert n_kf >= 2 and 1 <= obs_per_lm <= n_kf
    rng = np.random.Generator(np.random.PCG64(seed))
    fx, fy, cx, cy = cam["fx"], cam["fy"], cam["cx"], cam["cy"]
    W, H = cam["width"], cam["height"]
    # a full circle from 100 keyframes on (the last keyframe comes back next to the first), an arc of that circle below
    R = max(n_kf, 100) * step / (2 * np.pi)
    x_true = np.zeros((n_kf, 6))
    for k in range(n_kf):
        th = k * step / R
        # camera k on a circle in the x-z plane, optical axis (z) along the tangent (sin th, 0, cos th): a rotation by th about y
        x_true[k, 3:] = [0.0, th, 0.0]
        T = se3_exp(np.concatenate([[0.0, 0.0, 0.0], x_true[k, 3:]]))
        T[:3, 3] = [R * (1 - np.cos(th)), 0.0, R * np.sin(th)]
        x_true[k] = np.concatenate([np.linalg.solve(_V(x_true[k, 3:]), T[:3, 3]), x_true[k, 3:]])
    T_true = np.stack([se3_exp(x) for x in x_true])
    # stored poses and the estimates the optimisation starts from: both near the truth, not equal to each other
    x_est = x_true + pose_noise * rng.standard_normal(x_true.shape)
    T_kf_w = np.stack([se3_exp(x_true[k] + pose_noise * rng.standard_normal(6)) for k in range(n_kf)])

    def windows(n):
        last = n_kf if loop else n_kf - obs_per_lm + 1
        s = rng.integers(0, last, n)
        return (s[:, None] + np.arange(obs_per_lm)[None, :]) % n_kf

    def in_front(kfs, n):
        """points 4..12 m in front of the middle keyframe of each window, inside its image"""
        mid = kfs[:, obs_per_lm // 2]
        z = rng.uniform(4.0, 12.0, n)
        u = rng.uniform(0.2 * W, 0.8 * W, n)
        v = rng.uniform(0.2 * H, 0.8 * H, n)
        Pc = np.stack([(u - cx) / fx * z, (v - cy) / fy * z, z], axis=1)
        Tm = T_true[mid]
        return np.einsum("nab,nb->na", Tm[:, :3, :3], Pc) + Tm[:, :3, 3]

    def project(k, X):
        Ti = np.linalg.inv(T_true[k])
        Xc = X @ Ti[:3, :3].T + Ti[:3, 3]
        return np.stack([cx + fx * Xc[:, 0] / Xc[:, 2], cy + fy * Xc[:, 1] / Xc[:, 2]], axis=1)

    def unobserved(n):
        m = np.zeros(n, bool)
        if n_unobserved and n > 2:
            m[rng.choice(np.arange(1, n - 1), size=min(n_unobserved, n - 2), replace=False)] = True
        return m

    kf_pt = windows(n_pt)
    Xw_true = in_front(kf_pt, n_pt) if n_pt else np.zeros((0, 3))
    kf_ls = windows(n_ls)
    P = in_front(kf_ls, n_ls) if n_ls else np.zeros((0, 3))
    Q = P + rng.uniform(-1.0, 1.0, (n_ls, 3)) * np.array([1.0, 1.0, 0.3])
    skip_pt, skip_ls = unobserved(n_pt), unobserved(n_ls)

    def obs_rows(kfs, skip):
        rows = []
        for j in range(kfs.shape[0]):
            if skip[j]:
                continue
            for i, k in enumerate(kfs[j]):
                rows.append((j, j, i, int(k), int(k) - 1, 1))
        return np.array(rows, np.int32).reshape(-1, 6)

    pt_obs, ls_obs = obs_rows(kf_pt, skip_pt), obs_rows(kf_ls, skip_ls)
    uv = np.empty((pt_obs.shape[0], 2))
    l_obs = np.empty((ls_obs.shape[0], 3))
    for k in range(n_kf):
        sel = pt_obs[:, 3] == k
        uv[sel] = project(k, Xw_true[pt_obs[sel, 1]])
        sel = ls_obs[:, 3] == k
        p = project(k, P[ls_obs[sel, 1]])
        q = project(k, Q[ls_obs[sel, 1]])
        if sel.any():
            p = p + noise_px * rng.standard_normal(p.shape)
            q = q + noise_px * rng.standard_normal(q.shape)
            ln = np.cross(np.concatenate([p, np.ones((p.shape[0], 1))], 1), np.concatenate([q, np.ones((q.shape[0], 1))], 1))
            ln /= np.sqrt(ln[:, 0:1] ** 2 + ln[:, 1:2] ** 2)      # normalised 2D line equation (include/mapFeatures.h:93)
            l_obs[sel] = ln
    uv += noise_px * rng.standard_normal(uv.shape)
    Xw = Xw_true + 0.02 * rng.standard_normal(Xw_true.shape)
    Lw = np.concatenate([P, Q], axis=1) + 0.02 * rng.standard_normal((n_ls, 6))
    return dict(n_map_kf=n_kf, kf_list=np.arange(1, n_kf, dtype=np.int32), T_kf_w=T_kf_w.reshape(n_kf, 16),
                x_kf=x_est[1:].copy(), Xw=Xw, Lw=Lw, pt_obs=pt_obs, pt_uv=uv, ls_obs=ls_obs, ls_l=l_obs, npt=n_pt, nls=n_ls)


def map_image(m):
    """The arrays of a plslam_map_index (the dict plslam_amd.local_map.DeviceMapIndex takes) whose global-BA gather
    (LocalMap.form_all + .gather) gives back a trajectory_map-shaped dict m: kf_list, the six Vector6i columns, pt_uv, ls_l, Xw, Lw.

    Every landmark is valid and an inlier, landmark j of the image is local landmark j; kf_valid marks kf_list plus slot 0;
    obs_ptr counts column 1; x_kf_w holds x_kf at the optimised slots (NaN elsewhere: nothing reads it).  No features: the GBA
    gather reads none.  Precondition (asserted): the rows are grouped by ascending landmark local index, column 0 equals column 1,
    column 2 counts from 0 within the landmark and column 4 is the position of column 3 in kf_list, or -1."""
    n_map = int(m["n_map_kf"])
    kf_list = np.asarray(m["kf_list"], np.int32)
    assert kf_list.size and (np.diff(kf_list) > 0).all() and kf_list[0] >= 1 and kf_list[-1] < n_map, "kf_list: ascending slots above 0"
    kf_valid = np.zeros(n_map, np.uint8)
    kf_valid[0] = 1
    kf_valid[kf_list] = 1
    inv = np.full(n_map, -1, np.int32)
    inv[kf_list] = np.arange(kf_list.size, dtype=np.int32)
    x_kf_w = np.full((n_map, 6), np.nan)
    x_kf_w[kf_list] = np.asarray(m["x_kf"], np.float64).reshape(-1, 6)

    def kind(obs, val, X, dv):
        obs = np.asarray(obs, np.int32).reshape(-1, 6)
        n = X.shape[0]
        lm = obs[:, 1]
        assert ((lm >= 0) & (lm < n)).all() and (np.diff(lm) >= 0).all(), "rows grouped by ascending landmark local index"
        assert (obs[:, 0] == lm).all(), "landmark map index == local index"
        obs_ptr = np.zeros(n + 1, np.int32)
        obs_ptr[1:] = np.cumsum(np.bincount(lm, minlength=n))
        assert (obs[:, 2] == np.arange(obs.shape[0]) - obs_ptr[lm]).all(), "column 2 counts within the landmark"
        assert ((obs[:, 3] >= 0) & (obs[:, 3] < n_map)).all() and (obs[:, 4] == inv[obs[:, 3]]).all(), "column 4 is kf_list's position"
        assert (obs[:, 5] == 1).all()
        return dict(n=n, valid=np.ones(n, np.uint8), inlier=np.ones(n, np.uint8), X=np.asarray(X, np.float64).copy(), obs_ptr=obs_ptr,
                    obs_kf=obs[:, 3].copy(), obs_val=np.asarray(val, np.float64).reshape(-1, dv).copy(),
                    feat_ptr=np.zeros(n_map + 1, np.int32), feat_idx=np.zeros(0, np.int32))

    return dict(n_map_kf=n_map, kf_valid=kf_valid, x_kf_w=x_kf_w, points=kind(m["pt_obs"], m["pt_uv"], np.asarray(m["Xw"]).reshape(-1, 3), 2),
                lines=kind(m["ls_obs"], m["ls_l"], np.asarray(m["Lw"]).reshape(-1, 6), 3))


def covisible_blocks(m):
    """The set of lower covisible keyframe blocks (k1 >= k2, local indices) the map's observations produce."""
    out = set()
    for obs in (m["pt_obs"], m["ls_obs"]):
        if obs.shape[0] == 0:
            continue
        order = np.argsort(obs[:, 1], kind="stable")
        o = obs[order]
        starts = np.flatnonzero(np.r_[True, o[1:, 1] != o[:-1, 1]])
        for a, b in zip(starts, np.r_[starts[1:], o.shape[0]]):
            ks = [int(k) for k in o[a:b, 4] if k >= 0]
            for k1 in ks:
                for k2 in ks:
                    if k1 >= k2:
                        out.add((k1, k2))
    return out


def _V(w):
    th = np.linalg.norm(w)
    if th < 1e-6:
        return np.eye(3)
    s = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]]) / th
    return np.eye(3) + s * (1 - np.cos(th)) / th + s @ s * (th - np.sin(th)) / th
