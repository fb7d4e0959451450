"""plslam_lba_plan (include/plslam_hip.h): the local bundle adjustment over lists uploaded or built once -- one H / g build per
call, the Schur step and the back substitution, or the reference's whole LM loop on the device in one call."""
from __future__ import annotations

import ctypes as C

import numpy as np

from ._lib import Cam, Handle, _arr, _check, _p, proto

LBA_STOP_MAX_ITERS, LBA_STOP_ERR, LBA_STOP_DX, LBA_STOP_NOT_PD = 0, 1, 2, 3
LBA_SOLVE_MAX_N6 = 120   # plslam_amd/csrc/lba_lm_dev.hip: the largest reduced system the one-workgroup solve takes


class LbaLmParams(C.Structure):
    """plslam_lba_lm_params"""
    _fields_ = [("lambda_lba_lm", C.c_double), ("lambda_lba_k", C.c_double), ("max_iters_lba", C.c_int32), ("reserved", C.c_int32),
                ("min_error_change", C.c_double), ("min_error", C.c_double)]


class LbaSolve(C.Structure):
    """plslam_lba_solve: one record per H / g build of plslam_lba_plan_optimize_dev"""
    _fields_ = [("lambda_", C.c_double), ("err_raw", C.c_double), ("err", C.c_double), ("dx_norm", C.c_double),
                ("n_singular", C.c_int32), ("n_bad_pivots", C.c_int32), ("applied", C.c_int32), ("reserved", C.c_int32)]


class LbaResult(C.Structure):
    """plslam_lba_result"""
    _fields_ = [("iters", C.c_int32), ("n_builds", C.c_int32), ("stop_reason", C.c_int32), ("n_enqueued_passes", C.c_int32),
                ("err", C.c_double), ("err_prev", C.c_double), ("lambda_", C.c_double), ("hmax", C.c_double)]


class _ListSizes(C.Structure):
    """plslam_lba_list_sizes"""
    _fields_ = [(k, C.c_int32) for k in ("nkf", "npt", "nls", "n_pt_obs", "n_ls_obs", "n_kf_ids", "max_chunks", "schur_ready",
                                         "nblk", "n_pairs", "schur_chunks")]


_LIST_NAMES = ("pt_ptr", "pt_ids", "ls_ptr", "ls_ids", "kf_ptr", "kf_ids", "pt_lm_loc", "pt_pose_slot", "pt_kf_loc", "pt_obs_uv",
               "ls_lm_loc", "ls_pose_slot", "ls_kf_loc", "ls_l_obs", "blk_ptr", "pairs")


class _Lists(C.Structure):
    """plslam_lba_lists: host pointers, NULL = skip"""
    _fields_ = [(k, C.c_void_p) for k in _LIST_NAMES]


class _HostState(C.Structure):
    """plslam_lba_host_state"""
    _fields_ = [("T_kf_w", C.c_void_p), ("Xw", C.c_void_p), ("Lw", C.c_void_p), ("g", C.c_void_p),
                ("n_pose_slots", C.c_int32), ("npt", C.c_int32), ("nls", C.c_int32), ("n", C.c_int64)]


class _DeviceState(C.Structure):
    """plslam_lba_state"""
    _fields_ = [("T_kf_w", C.c_void_p), ("Xw", C.c_void_p), ("Lw", C.c_void_p), ("n_pose_slots", C.c_int32),
                ("npt", C.c_int32), ("nls", C.c_int32), ("stream", C.c_void_p)]


_vp, _i32, _f64 = C.c_void_p, C.c_int32, C.c_double
proto("plslam_lba_plan_create", [_vp, C.POINTER(Cam), _f64, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _i32, _vp, _vp, _vp, _vp,
                                 _i32, C.POINTER(_vp)])
proto("plslam_lba_plan_create_dev", [_vp, C.POINTER(Cam), _f64, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _i32, _vp, _vp, _vp, _vp,
                                     _i32, _vp, _vp, _i32, C.POINTER(_vp)])
proto("plslam_lba_plan_list_sizes", [_vp, C.c_int, _vp])
proto("plslam_lba_plan_lists", [_vp, _vp])
proto("plslam_lba_plan_iterate_dev", [_vp, _vp, _vp, _vp, C.c_int, _vp, _vp])
proto("plslam_lba_plan_iterate_resident", [_vp, C.c_int, _vp])
proto("plslam_lba_plan_diag_max", [_vp, _vp])
proto("plslam_lba_plan_schur", [_vp, C.c_double, _vp, _vp, _vp])
proto("plslam_lba_plan_backsub", [_vp, _vp, C.c_int, _vp, _vp])
proto("plslam_lba_plan_set_poses", [_vp, _vp])
proto("plslam_lba_plan_iterate_schur", [_vp, C.c_int, C.c_double, _vp, _vp, _vp, _vp])
proto("plslam_lba_plan_apply_step", [_vp, _vp, _vp, C.c_int, _vp])
proto("plslam_lba_plan_optimize_dev", [_vp, C.POINTER(LbaLmParams), _vp, _vp, _i32, _vp, _vp, _vp, C.POINTER(LbaResult)])
proto("plslam_lba_plan_get_landmarks", [_vp, _vp, _vp])
proto("plslam_lba_plan_host_state", [_vp, _vp])
proto("plslam_lba_plan_device_state", [_vp, _vp])
proto("plslam_lba_plan_device_blocks", [_vp, _vp])
proto("plslam_lba_plan_blocks", [_vp] * 8)
proto("plslam_lba_plan_iterate", [_vp, _vp, _vp, _vp, C.c_int, _vp, _vp, _vp, _vp, _vp, _vp, _vp])
proto("plslam_lba_plan_rows", [_vp] * 9)
proto("plslam_lba_plan_destroy", [_vp], None)


class LbaPlan(Handle):
    """plslam_lba_plan: observation lists uploaded once, iterate(T_kf_w, Xw, Lw) per LM iteration."""

    def __init__(self, ctx: Context, cam: Cam, homog_th, n_pose_slots, nkf, npt, nls, pt_lm, pt_slot, pt_kf_loc,
                 pt_obs_uv, ls_lm, ls_slot, ls_kf_loc, ls_l_obs):
        a = [_arr(x, np.int32) for x in (pt_lm, pt_slot, pt_kf_loc)]
        b = [_arr(x, np.int32) for x in (ls_lm, ls_slot, ls_kf_loc)]
        uv, lo = _arr(pt_obs_uv, np.float64, (-1, 2)), _arr(ls_l_obs, np.float64, (-1, 3))
        self.dims = (int(nkf), int(npt), int(nls), uv.shape[0], lo.shape[0], int(n_pose_slots))
        h = C.c_void_p()
        _check(ctx._L.plslam_lba_plan_create(ctx.handle, C.byref(cam), float(homog_th), int(n_pose_slots), int(nkf),
                                             int(npt), int(nls), _p(a[0]), _p(a[1]), _p(a[2]), _p(uv), uv.shape[0],
                                             _p(b[0]), _p(b[1]), _p(b[2]), _p(lo), lo.shape[0], C.byref(h)),
               "plslam_lba_plan_create")
        self._open(ctx, "plslam_lba_plan_destroy", h)

    COMPAT_ITER_PASS, COMPAT_GBA = 1, 2
    DIST_TILE = 1024        # plslam_amd/csrc/distribute_dev.hpp: the items one workgroup of the device-side list builder takes

    @classmethod
    def from_device(cls, ctx: Context, cam: Cam, homog_th, n_pose_slots, nkf, npt, nls, pt_lm, pt_slot, pt_kf_loc, pt_obs_uv,
                    n_pt_obs, ls_lm, ls_slot, ls_kf_loc, ls_l_obs, n_ls_obs, d_Xw=0, d_Lw=0, first_estimate_slot=-1):
        """plslam_lba_plan_create_dev: the eight observation columns and d_Xw / d_Lw are DEVICE pointers (ints, 0 = NULL), e.g.
        the entries of LocalMap.device_buffers(); the lists are built on the device.  first_estimate_slot >= 0 rewrites the slot
        of every point observation of an optimised keyframe to first_estimate_slot + kf_loc."""
        self = cls.__new__(cls)
        self.dims = (int(nkf), int(npt), int(nls), int(n_pt_obs), int(n_ls_obs), int(n_pose_slots))
        h = C.c_void_p()
        q = lambda a: C.c_void_p(int(a)) if a else None                          # noqa: E731
        _check(ctx._L.plslam_lba_plan_create_dev(ctx.handle, C.byref(cam), float(homog_th), int(n_pose_slots), int(nkf), int(npt),
                                                 int(nls), q(pt_lm), q(pt_slot), q(pt_kf_loc), q(pt_obs_uv), int(n_pt_obs),
                                                 q(ls_lm), q(ls_slot), q(ls_kf_loc), q(ls_l_obs), int(n_ls_obs), q(d_Xw), q(d_Lw),
                                                 int(first_estimate_slot), C.byref(h)), "plslam_lba_plan_create_dev")
        self._open(ctx, "plslam_lba_plan_destroy", h)
        return self

    def lists(self, prepare_schur=False) -> dict:
        """The plan's lists as host arrays (plslam_lba_plan_lists): pt_ptr / pt_ids, ls_ptr / ls_ids, kf_ptr / kf_ids, the
        observation columns as the plan stores them, max_chunks; once the Schur lists exist (prepare_schur=True builds them):
        blk_ptr, pairs (n, 4) and schur_chunks."""
        z = _ListSizes()
        _check(self._L.plslam_lba_plan_list_sizes(self._h, int(bool(prepare_schur)), C.addressof(z)), "plslam_lba_plan_list_sizes")
        i32, f64 = np.int32, np.float64
        out = dict(pt_ptr=np.zeros(z.npt + 1, i32), pt_ids=np.zeros(z.n_pt_obs, i32), ls_ptr=np.zeros(z.nls + 1, i32),
                   ls_ids=np.zeros(z.n_ls_obs, i32), kf_ptr=np.zeros(z.nkf + 1, i32), kf_ids=np.zeros(z.n_kf_ids, i32),
                   pt_lm_loc=np.zeros(z.n_pt_obs, i32), pt_pose_slot=np.zeros(z.n_pt_obs, i32), pt_kf_loc=np.zeros(z.n_pt_obs, i32),
                   pt_obs_uv=np.zeros((z.n_pt_obs, 2), f64), ls_lm_loc=np.zeros(z.n_ls_obs, i32), ls_pose_slot=np.zeros(z.n_ls_obs, i32),
                   ls_kf_loc=np.zeros(z.n_ls_obs, i32), ls_l_obs=np.zeros((z.n_ls_obs, 3), f64))
        if z.schur_ready:
            out.update(blk_ptr=np.zeros(z.nblk + 1, i32), pairs=np.zeros((z.n_pairs, 4), i32))
        b = _Lists()
        for k, a in out.items():
            setattr(b, k, _p(a) if a.size else None)
        _check(self._L.plslam_lba_plan_lists(self._h, C.addressof(b)), "plslam_lba_plan_lists")
        out["max_chunks"] = int(z.max_chunks)
        if z.schur_ready:
            out["schur_chunks"] = int(z.schur_chunks)
        return out

    def iterate_dev(self, T_kf_w, Xw, Lw, compat_flags=0, want_g=True, g_out=None):
        """One iteration with the blocks left on the device -> (err, g or None).  With the arrays of host_state() as T_kf_w /
        Xw / Lw / g_out the call copies nothing on the host."""
        nkf, npt, nls, npo, nlo, nslot = self.dims
        T = _arr(T_kf_w, np.float64, (-1, 16))
        X, Lm = _arr(Xw, np.float64, (-1, 3)), _arr(Lw, np.float64, (-1, 6))
        if want_g and g_out is not None:
            assert g_out.dtype == np.float64 and g_out.flags.c_contiguous and g_out.size == 6 * nkf + 3 * npt + 6 * nls
            g = g_out
        else:
            g = np.empty(6 * nkf + 3 * npt + 6 * nls) if want_g else None
        err = np.empty(1)
        _check(self._L.plslam_lba_plan_iterate_dev(self._h, _p(T), _p(X), _p(Lm), int(compat_flags),
                                                   _p(g) if want_g else None, _p(err)), "plslam_lba_plan_iterate_dev")
        return float(err[0]), g

    def iterate_resident(self, compat_flags=0) -> float:
        """One iteration on the state already on the device (uploaded by an earlier iterate / iterate_dev, updated in place
        by a device-side solver: device_state()) -> err."""
        err = np.empty(1)
        _check(self._L.plslam_lba_plan_iterate_resident(self._h, int(compat_flags), _p(err)), "plslam_lba_plan_iterate_resident")
        return float(err[0])

    def diag_max(self) -> float:
        """max |H(i,i)| over the blocks of the last iteration (the reference's lambda *= Hmax)."""
        h = np.empty(1)
        _check(self._L.plslam_lba_plan_diag_max(self._h, _p(h)), "plslam_lba_plan_diag_max")
        return float(h[0])

    def schur(self, lam: float):
        """The reduced camera system of the last iteration's blocks for the damping `lam` -> (S (6 nkf, 6 nkf), b (6 nkf),
        number of singular landmark blocks)."""
        nkf = self.dims[0]
        S, b, ns = np.empty((6 * nkf, 6 * nkf)), np.empty(6 * nkf), np.zeros(1, np.int32)
        _check(self._L.plslam_lba_plan_schur(self._h, float(lam), _p(S), _p(b), _p(ns)), "plslam_lba_plan_schur")
        return S, b, int(ns[0])

    def backsub(self, dpose, apply=False, want=True):
        """The landmark steps for the pose step `dpose` -> (dX_pt (npt, 3), dX_ls (nls, 6)) or None; apply=True also adds them
        to the resident landmarks."""
        nkf, npt, nls = self.dims[:3]
        dp = _arr(dpose, np.float64, (6 * nkf,))
        dxp, dxl = (np.empty((npt, 3)), np.empty((nls, 6))) if want else (None, None)
        _check(self._L.plslam_lba_plan_backsub(self._h, _p(dp), int(bool(apply)), _p(dxp) if want else None,
                                               _p(dxl) if want else None), "plslam_lba_plan_backsub")
        return (dxp, dxl) if want else None

    def set_poses(self, T_kf_w) -> None:
        T = _arr(T_kf_w, np.float64, (-1, 16))
        assert T.shape[0] == self.dims[5]
        _check(self._L.plslam_lba_plan_set_poses(self._h, _p(T)), "plslam_lba_plan_set_poses")

    def iterate_schur(self, lam: float, compat_flags: int = 0):
        """iterate_resident + schur(lam) behind one synchronisation -> (err, S, b, number of singular landmark blocks)."""
        nkf = self.dims[0]
        err, S, b, ns = np.empty(1), np.empty((6 * nkf, 6 * nkf)), np.empty(6 * nkf), np.zeros(1, np.int32)
        _check(self._L.plslam_lba_plan_iterate_schur(self._h, int(compat_flags), float(lam), _p(err), _p(S), _p(b), _p(ns)),
               "plslam_lba_plan_iterate_schur")
        return float(err[0]), S, b, int(ns[0])

    def apply_step(self, dpose, T_kf_w=None, apply=True) -> float:
        """backsub(dpose, apply) + set_poses(T_kf_w, None: leave them) behind one synchronisation -> sum of squares of the
        landmark steps."""
        nkf = self.dims[0]
        dp = _arr(dpose, np.float64, (6 * nkf,))
        T = None
        if T_kf_w is not None:
            T = _arr(T_kf_w, np.float64, (-1, 16))
            assert T.shape[0] == self.dims[5]
        ss = np.empty(1)
        _check(self._L.plslam_lba_plan_apply_step(self._h, _p(dp), _p(T) if T is not None else None, int(bool(apply)), _p(ss)),
               "plslam_lba_plan_apply_step")
        return float(ss[0])

    def optimize_dev(self, T_slots, x_kf, first_estimate_slot, lambda_lm=1e-5, lambda_k=10.0, max_iters=15, min_error_change=1e-7,
                     min_error=1e-7) -> dict:
        """plslam_lba_plan_optimize_dev: the whole LM loop of the local BA on the device, one synchronisation.  T_slots
        (n_pose_slots, 16): the stored T_kf_w, in the estimate slots too; x_kf (nkf, 6).  The landmarks must be resident and stay in
        the plan (get_landmarks, LocalMap.apply_lba).  -> dict(x_kf (nkf, 6), T (nkf, 4, 4), the trace arrays lam / err_raw / err /
        dx_norm / n_singular / n_bad_pivots / applied (one entry per H / g build), iters, n_builds, stop_reason,
        n_enqueued_passes, err_last, err_prev, lam_last, hmax)."""
        nkf, nslot = self.dims[0], self.dims[5]
        T = _arr(T_slots, np.float64, (nslot, 16))
        x = _arr(x_kf, np.float64, (nkf, 6))
        prm = LbaLmParams(float(lambda_lm), float(lambda_k), int(max_iters), 0, float(min_error_change), float(min_error))
        xo, To = np.empty((nkf, 6)), np.empty((nkf, 4, 4))
        tr = (LbaSolve * max(int(max_iters), 1))()
        res = LbaResult()
        _check(self._L.plslam_lba_plan_optimize_dev(self._h, C.byref(prm), _p(T), _p(x), int(first_estimate_slot), _p(xo), _p(To),
                                                    C.cast(tr, C.c_void_p), C.byref(res)), "plslam_lba_plan_optimize_dev")
        rec = tr[:res.n_builds]
        return dict(x_kf=xo, T=To, lam=np.array([t.lambda_ for t in rec]), err_raw=np.array([t.err_raw for t in rec]),
                    err=np.array([t.err for t in rec]), dx_norm=np.array([t.dx_norm for t in rec]),
                    n_singular=np.array([t.n_singular for t in rec], np.int32), n_bad_pivots=np.array([t.n_bad_pivots for t in rec], np.int32),
                    applied=np.array([t.applied for t in rec], np.int32), iters=res.iters, n_builds=res.n_builds,
                    stop_reason=res.stop_reason, n_enqueued_passes=res.n_enqueued_passes, err_last=res.err, err_prev=res.err_prev,
                    lam_last=res.lambda_, hmax=res.hmax)

    def get_landmarks(self):
        """The resident landmarks (after backsub(apply=True)) -> (Xw (npt, 3), Lw (nls, 6)); also refreshes the page-locked images
        of host_state()."""
        nkf, npt, nls, npo, nlo, nslot = self.dims
        X, Lm = np.empty((npt, 3)), np.empty((nls, 6))
        _check(self._L.plslam_lba_plan_get_landmarks(self._h, _p(X), _p(Lm)), "plslam_lba_plan_get_landmarks")
        return X, Lm

    def host_state(self) -> dict:
        """The plan's page-locked images as numpy views (T_kf_w (n_pose_slots, 16), Xw (npt, 3), Lw (nls, 6), g (n,)): a
        solver that keeps its state in them passes them to iterate_dev(..., g_out=g) and nothing is staged.  The views die with
        the plan."""
        st = _HostState()
        _check(self._L.plslam_lba_plan_host_state(self._h, C.byref(st)), "plslam_lba_plan_host_state")

        def view(ptr, shape):
            n = int(np.prod(shape))
            if n == 0:
                return np.empty(shape)
            return np.ctypeslib.as_array(C.cast(ptr, C.POINTER(C.c_double)), shape=(n,)).reshape(shape)
        return dict(T_kf_w=view(st.T_kf_w, (st.n_pose_slots, 16)), Xw=view(st.Xw, (st.npt, 3)), Lw=view(st.Lw, (st.nls, 6)),
                    g=view(st.g, (st.n,)))

    def device_state(self) -> dict:
        """Device pointers (ints) of T_kf_w / Xw / Lw, their row counts and the plan's HIP stream."""
        st = _DeviceState()
        _check(self._L.plslam_lba_plan_device_state(self._h, C.byref(st)), "plslam_lba_plan_device_state")
        return {k: getattr(st, k) for k, _ in _DeviceState._fields_}

    def blocks(self):
        """Download the blocks of the last iteration (the arrays plslam_lba_plan_device_blocks names)."""
        nkf, npt, nls, npo, nlo, _ = self.dims
        g, Hp = np.empty(6 * nkf + 3 * npt + 6 * nls), np.empty((nkf, 6, 6))
        Hpt, Hls = np.empty((npt, 3, 3)), np.empty((nls, 6, 6))
        Wp, Wl = np.empty((npo, 3, 6)), np.empty((nlo, 6, 6))
        err = np.empty(1)
        _check(self._L.plslam_lba_plan_blocks(self._h, _p(g), _p(Hp), _p(Hpt), _p(Hls), _p(Wp), _p(Wl), _p(err)),
               "plslam_lba_plan_blocks")
        return dict(g=g, H_pose=Hp, H_pt=Hpt, H_ls=Hls, W_pt=Wp, W_ls=Wl, err=float(err[0]))

    def iterate(self, T_kf_w, Xw, Lw, compat_iter_pass=False):
        nkf, npt, nls, npo, nlo, nslot = self.dims
        T = _arr(T_kf_w, np.float64, (-1, 16))
        X, Lm = _arr(Xw, np.float64, (-1, 3)), _arr(Lw, np.float64, (-1, 6))
        assert T.shape[0] == nslot and X.shape[0] == npt and Lm.shape[0] == nls
        N = 6 * nkf + 3 * npt + 6 * nls
        g, Hp = np.empty(N), np.empty((nkf, 6, 6))
        Hpt, Hls = np.empty((npt, 3, 3)), np.empty((nls, 6, 6))
        Wp, Wl = np.empty((npo, 3, 6)), np.empty((nlo, 6, 6))
        err = np.empty(1)
        _check(self._L.plslam_lba_plan_iterate(self._h, _p(T), _p(X), _p(Lm), int(compat_iter_pass), _p(g), _p(Hp),
                                               _p(Hpt), _p(Hls), _p(Wp), _p(Wl), _p(err)), "plslam_lba_plan_iterate")
        return dict(g=g, H_pose=Hp, H_pt=Hpt, H_ls=Hls, W_pt=Wp, W_ls=Wl, err=float(err[0]))

    def rows(self):
        nkf, npt, nls, npo, nlo, _ = self.dims
        pr = [np.empty((npo, 6)), np.empty((npo, 3)), np.empty(npo), np.empty(npo)]
        lr = [np.empty((nlo, 6)), np.empty((nlo, 6)), np.empty(nlo), np.empty(nlo)]
        _check(self._L.plslam_lba_plan_rows(self._h, *[_p(x) for x in pr + lr]), "plslam_lba_plan_rows")
        return pr, lr
