"""plslam_ctx and the calls made on it directly (include/plslam_hip.h): the host-pointer calls (numpy in, numpy out), the
loop-closure verification and the device-pointer forms; page-locked host arrays.  Plumbing only: no algorithm, and NO CPU
fallback."""
from __future__ import annotations

import ctypes as C

import numpy as np

from ._lib import ENOMEM, Cam, Handle, PlslamError, _arr, _check, _p, load, make_cam, proto  # noqa: F401 (Cam, make_cam: their home for callers)
from .loop_closure import LcKeyframe, LcParams, LcResult, _lc_kf_arrays, _lc_kf_record
from .match import MatchPlan

SCAN_AUTO, SCAN_LANE_PER_QUERY, SCAN_WAVE_PER_QUERY, SCAN_SYMMETRIC, SCAN_MFMA = 0, 1, 2, 3, 4

# plslam_lbd_line as a numpy record
LBD_LINE_DTYPE = np.dtype([("num_pixels", np.int32), ("sx", np.float32), ("sy", np.float32), ("ex", np.float32),
                           ("ey", np.float32), ("direction", np.float32)])


class FastMatching(C.Structure):
    """plslam_fast_matching"""
    _fields_ = [("enabled", C.c_int32), ("grid_cols", C.c_int32), ("grid_rows", C.c_int32), ("ws", C.c_int32),
                ("inv_width", C.c_double), ("inv_height", C.c_double), ("nnr_grid", C.c_double),
                ("line_sim_th", C.c_double)]


def _fast_matching(fm) -> FastMatching:
    """fm: dict with the fields of plslam_fast_matching"""
    return FastMatching(int(fm["enabled"]), int(fm["grid_cols"]), int(fm["grid_rows"]), int(fm["ws"]),
                        float(fm["inv_width"]), float(fm["inv_height"]), float(fm["nnr_grid"]),
                        float(fm.get("line_sim_th", 0.75)))


_vp, _i32, _f64 = C.c_void_p, C.c_int32, C.c_double
proto("plslam_ctx_create", [C.c_int, C.POINTER(_vp)])
proto("plslam_ctx_destroy", [_vp], None)
proto("plslam_ctx_set_option", [_vp, C.c_char_p, C.c_int])
proto("plslam_ctx_get_option", [_vp, C.c_char_p, C.POINTER(C.c_int)])
proto("plslam_ctx_device_info", [_vp, C.POINTER(_i32), C.POINTER(_i32), C.POINTER(_i32), C.c_char_p, _i32])
proto("plslam_lba_reduced_ldlt_solve", [_vp, _i32, _vp, _vp, _vp, C.POINTER(_i32)])
proto("plslam_pinned_alloc", [C.c_size_t], C.c_void_p)
proto("plslam_pinned_free", [_vp], None)
# ---- host-pointer calls (numpy in, numpy out) ------------------------------------------
proto("plslam_knn2_hamming256", [_vp, _vp, _i32, _vp, _i32, _vp, _vp])
proto("plslam_match", [_vp, _vp, _i32, _vp, _i32, C.c_float, C.c_int, _vp, C.POINTER(_i32)])
proto("plslam_match_prior", [_vp, _vp, _i32, _vp, _i32, C.c_float, C.c_int, _vp, C.POINTER(_i32)])
proto("plslam_match_grid", [_vp, _vp, _i32, _vp, _i32, _vp, _vp, _i32, _i32, _vp, _i32, _vp, _vp, _f64, _vp, _f64, C.c_int, _vp, C.POINTER(_i32)])
proto("plslam_pose_gn_accumulate", [_vp, C.POINTER(Cam), _f64, _vp, _vp, _vp, _vp, _i32, _vp, _vp, _vp, _i32, _vp, _vp, _vp, _vp])
# ---- K25: loop-closure verification (MapHandler::isLoopClosure) --------------------------------------------------
proto("plslam_loop_closure_verify", [_vp, C.POINTER(LcParams), C.POINTER(LcKeyframe), C.POINTER(LcKeyframe), C.POINTER(LcResult),
                                     _vp, _vp, _vp, _vp])
proto("plslam_loop_closure_verify_dev", [_vp, C.POINTER(LcParams), C.POINTER(LcKeyframe), C.POINTER(LcKeyframe), _vp, _vp, _vp, _vp, _vp, _vp])
proto("plslam_relpose_robust_gn", [_vp, C.POINTER(LcParams), _vp, _vp, _i32, _vp, _vp, _i32, C.POINTER(LcResult), _vp, _vp])
proto("plslam_relpose_robust_gn_batched_dev", [_vp, C.POINTER(LcParams), _vp, _vp, _vp, _vp, _vp, _vp, _i32, _vp, _vp, _vp, _vp])
proto("plslam_stereo_point_gate", [_vp, _vp, _i32, _vp, _vp, _i32, _f64, _f64, _vp, _vp, C.POINTER(_i32)])
proto("plslam_stereo_line_gate", [_vp, _vp, _i32, _vp, _vp, _i32, _f64, _f64, _f64, _f64, _vp, _vp, C.POINTER(_i32)])
proto("plslam_match_batched", [_vp, _vp, _vp, _vp, _vp, _i32, C.c_float, C.c_int, _vp, _vp])
proto("plslam_lba_point_rows", [_vp, C.POINTER(Cam), _f64, _vp, _i32, _vp, _i32, _vp, _vp, _vp, _i32, _vp, _vp, _vp, _vp])
proto("plslam_lba_line_rows", [_vp, C.POINTER(Cam), _f64, C.c_int, _vp, _i32, _vp, _i32, _vp, _vp, _vp, _i32, _vp, _vp, _vp, _vp])
proto("plslam_lba_assemble", [_vp, _i32, _i32, _i32, _vp, _vp, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp])
for _name in ("plslam_map2kf_point_gate", "plslam_map2kf_line_gate"):
    proto(_name, [_vp, C.POINTER(Cam), _vp, _vp, _vp, _i32, _vp, _i32, _f64, _vp, C.POINTER(_i32)])
for _name in ("plslam_map_point_visible", "plslam_map_line_visible"):
    proto(_name, [_vp, C.POINTER(Cam), _vp, _vp, _i32, _vp])
proto("plslam_median_desc_batched", [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p])
proto("plslam_median_desc_batched_dev", [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p])
proto("plslam_lbd_binarise", [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p])
proto("plslam_lbd_binarise_dev", [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p])
proto("plslam_lbd_compute", [_vp, _vp, _vp, _i32, _i32, _vp, _i32, _i32, _vp])
proto("plslam_lbd_compute_dev", [_vp, _vp, _vp, _i32, _i32, _vp, _i32, _i32, _vp, _vp])
for _name in ("plslam_map2kf_match_points", "plslam_map2kf_match_lines"):
    proto(_name, [_vp, C.POINTER(Cam), _vp, _vp, _vp, _vp, _i32, _vp, _vp, _vp, _i32, C.c_float, C.c_int, _f64, _i32, _vp, C.POINTER(_i32)])
for _name in ("plslam_map2kf_match_points_fast", "plslam_map2kf_match_points_dev"):
    proto(_name, [_vp, C.POINTER(Cam), _vp, _vp, _vp, _vp, _i32, _vp, _vp, _vp, _i32, C.c_float, C.c_int, _f64, _i32, C.POINTER(FastMatching), _vp,
                  C.POINTER(_i32), C.POINTER(_i32)])
for _name in ("plslam_map2kf_match_lines_fast", "plslam_map2kf_match_lines_dev"):
    proto(_name, [_vp, C.POINTER(Cam), _vp, _vp, _vp, _vp, _i32, _vp, _vp, _vp, _vp, _i32, C.c_float, C.c_int, _f64, _i32, C.POINTER(FastMatching), _vp,
                  C.POINTER(_i32), C.POINTER(_i32)])
for _name in ("plslam_kf2kf_match_points", "plslam_kf2kf_match_lines", "plslam_kf2kf_match_points_dev", "plslam_kf2kf_match_lines_dev"):
    proto(_name, [_vp, C.POINTER(Cam), _vp, _vp, _vp, _i32, _vp, _vp, _i32, C.c_float, C.c_int, _i32, C.POINTER(FastMatching), _vp, C.POINTER(_i32),
                  C.POINTER(_i32)])
# ---- device-pointer calls ----------------------------------------------------------------
proto("plslam_lba_point_rows_dev", [_vp, C.POINTER(Cam), _f64, _vp, _vp, _vp, _vp, _vp, _i32, _vp, _vp, _vp, _vp, _vp])
proto("plslam_lba_line_rows_dev", [_vp, C.POINTER(Cam), _f64, C.c_int, _vp, _vp, _vp, _vp, _vp, _i32, _vp, _vp, _vp, _vp, _vp])
proto("plslam_lba_point_rows_dev_n", [_vp, C.POINTER(Cam), _f64, _vp, _i32, _vp, _vp, _vp, _vp, _i32, _vp, _vp, _vp, _vp, _vp])
proto("plslam_lba_line_rows_dev_n", [_vp, C.POINTER(Cam), _f64, C.c_int, _vp, _i32, _vp, _vp, _vp, _vp, _i32, _vp, _vp, _vp, _vp, _vp])
proto("plslam_stereo_point_gate_dev", [_vp, _vp, _i32, _vp, _vp, _i32, _f64, _f64, _vp, _vp, _vp, _vp])
proto("plslam_stereo_line_gate_dev", [_vp, _vp, _i32, _vp, _vp, _i32, _f64, _f64, _f64, _f64, _vp, _vp, _vp, _vp])


class Context(Handle):
    """plslam_ctx: one HIP device, one stream, scratch pools."""

    def __init__(self, device: int = 0):
        self._L = load()
        h = C.c_void_p()
        _check(self._L.plslam_ctx_create(int(device), C.byref(h)), "plslam_ctx_create")
        self._open(self, "plslam_ctx_destroy", h)
        self.device = int(device)

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def set_option(self, key: str, value: int) -> None:
        _check(self._L.plslam_ctx_set_option(self._h, key.encode(), int(value)), "plslam_ctx_set_option")

    def get_option(self, key: str) -> int:
        v = C.c_int()
        _check(self._L.plslam_ctx_get_option(self._h, key.encode(), C.byref(v)), "plslam_ctx_get_option")
        return v.value

    def lba_reduced_ldlt_solve(self, A, b):
        """plslam_lba_reduced_ldlt_solve: the local BA's solve kernel alone -- x with (the lower triangle of A, mirrored) x = b by
        L D L^T without pivoting -> (x, number of pivots that are <= 0 or not finite)."""
        A = _arr(A, np.float64)
        n = A.shape[0]
        assert A.shape == (n, n)
        bb = _arr(b, np.float64, (n,))
        x, nb = np.empty(n), C.c_int32(0)
        _check(self._L.plslam_lba_reduced_ldlt_solve(self._h, n, _p(A), _p(bb), _p(x), C.byref(nb)), "plslam_lba_reduced_ldlt_solve")
        return x, int(nb.value)

    def device_info(self) -> dict:
        cu, clk, lds = C.c_int32(), C.c_int32(), C.c_int32()
        name = C.create_string_buffer(256)
        _check(self._L.plslam_ctx_device_info(self._h, C.byref(cu), C.byref(clk), C.byref(lds), name, 256),
               "plslam_ctx_device_info")
        return {"cu_count": cu.value, "clock_khz": clk.value, "lds_bytes": lds.value,
                "name": name.value.decode()}

    # ---- host-pointer calls (numpy in, numpy out) ------------------------------------------
    def knn2(self, q, t):
        q = _arr(q, np.uint8, (-1, 32))
        t = _arr(t, np.uint8, (-1, 32))
        idx = np.empty((q.shape[0], 2), np.int32)
        dist = np.empty((q.shape[0], 2), np.int32)
        _check(self._L.plslam_knn2_hamming256(self._h, _p(q), q.shape[0], _p(t), t.shape[0], _p(idx),
                                              _p(dist)), "plslam_knn2_hamming256")
        return idx, dist

    def match(self, d1, d2, nnr: float, mutual: bool = True):
        """StVO::match(desc1, desc2, nnr, matches_12) -> (matches_12, n_matches)."""
        d1 = _arr(d1, np.uint8, (-1, 32))
        d2 = _arr(d2, np.uint8, (-1, 32))
        m12 = np.empty(d1.shape[0], np.int32)
        n = C.c_int32()
        _check(self._L.plslam_match(self._h, _p(d1), d1.shape[0], _p(d2), d2.shape[0], float(nnr),
                                    int(bool(mutual)), _p(m12), C.byref(n)), "plslam_match")
        return m12, n.value

    def match_prior(self, d1, d2, nnr: float, mutual: bool, prior):
        """StVO::match on a matches_12 that already holds entries (the fall-back after matchGrid) -> (matches_12, n)."""
        d1 = _arr(d1, np.uint8, (-1, 32))
        d2 = _arr(d2, np.uint8, (-1, 32))
        m12 = np.array(prior, np.int32, copy=True)
        if m12.shape != (d1.shape[0],):
            raise ValueError("prior must hold one entry per row of d1")
        n = C.c_int32()
        _check(self._L.plslam_match_prior(self._h, _p(d1), d1.shape[0], _p(d2), d2.shape[0], float(nnr),
                                          int(bool(mutual)), _p(m12), C.byref(n)), "plslam_match_prior")
        return m12, n.value

    def match_grid(self, centres, d1, cell_start, cell_items, cols, rows, d2, window, nnr, mutual=True, dir1=None,
                   dir2=None, sim_th=0.0):
        """StVO::matchGrid (points: one window centre per row; lines: two + directions) -> (matches_12, n)."""
        d1 = _arr(d1, np.uint8, (-1, 32))
        d2 = _arr(d2, np.uint8, (-1, 32))
        n1 = d1.shape[0]
        cen = _arr(centres, np.int32).reshape(n1, -1, 2) if n1 else np.zeros((0, 1, 2), np.int32)
        cs, items = _arr(cell_start, np.int32), _arr(cell_items, np.int32)
        w = _arr(window, np.int32, (4,))
        a = _arr(dir1, np.float64, (-1, 2)) if dir1 is not None else None
        b = _arr(dir2, np.float64, (-1, 2)) if dir2 is not None else None
        m12 = np.empty(n1, np.int32)
        n = C.c_int32()
        _check(self._L.plslam_match_grid(self._h, _p(cen), cen.shape[1], _p(d1), n1, _p(cs), _p(items), int(cols),
                                         int(rows), _p(d2), d2.shape[0], _p(a) if a is not None else None,
                                         _p(b) if b is not None else None, float(sim_th), _p(w), float(nnr),
                                         int(bool(mutual)), _p(m12), C.byref(n)), "plslam_match_grid")
        return m12, n.value

    def pose_gn_accumulate(self, cam, homog_th, T_inc, P, pl_obs, pt_inlier, sPeP, le_obs, ls_inlier):
        """computeRelativePoseGN iteration body -> (H[6,6], g[6], e, (N_p, N_l))."""
        T = _arr(T_inc, np.float64, (16,))
        P, po = _arr(P, np.float64, (-1, 3)), _arr(pl_obs, np.float64, (-1, 2))
        S, lo = _arr(sPeP, np.float64, (-1, 6)), _arr(le_obs, np.float64, (-1, 3))
        pi, li = _arr(pt_inlier, np.uint8), _arr(ls_inlier, np.uint8)
        H, g, e, n = np.empty((6, 6)), np.empty(6), np.empty(1), np.empty(2, np.int32)
        _check(self._L.plslam_pose_gn_accumulate(self._h, C.byref(cam), float(homog_th), _p(T), _p(P), _p(po), _p(pi),
                                                 P.shape[0], _p(S), _p(lo), _p(li), S.shape[0], _p(H), _p(g), _p(e), _p(n)),
               "plslam_pose_gn_accumulate")
        return H, g, float(e[0]), (int(n[0]), int(n[1]))

    # ---- K25: loop-closure verification (MapHandler::isLoopClosure) --------------------------------------------------
    _lc_kf_arrays = staticmethod(_lc_kf_arrays)     # (their home is plslam_amd.loop_closure; the names stay for callers)
    _lc_kf_record = staticmethod(_lc_kf_record)

    def loop_closure_verify(self, params, kf0, kf1):
        """isLoopClosure(kf0, kf1) -> (result dict, pt_corr[common_pt, 4], pt_inlier, ls_corr[common_ls, 4], ls_inlier).
        kf0 / kf1: dicts with pdesc, P, pl, pt_idx (or None), ldesc, sPeP, le, ls_idx (or None)."""
        a0, a1 = _lc_kf_arrays(kf0), _lc_kf_arrays(kf1)
        r0, r1 = _lc_kf_record(a0), _lc_kf_record(a1)
        n0p, n0l = a0["P"].shape[0], a0["sPeP"].shape[0]
        pc, pi = np.zeros((n0p, 4), np.int32), np.zeros(n0p, np.uint8)
        lc, li = np.zeros((n0l, 4), np.int32), np.zeros(n0l, np.uint8)
        res = LcResult()
        _check(self._L.plslam_loop_closure_verify(self._h, C.byref(params), C.byref(r0), C.byref(r1), C.byref(res), _p(pc),
                                                  _p(pi), _p(lc), _p(li)), "plslam_loop_closure_verify")
        d = res.as_dict()
        return d, pc[:d["common_pt"]], pi[:d["common_pt"]].astype(bool), lc[:d["common_ls"]], li[:d["common_ls"]].astype(bool)

    def loop_closure_verify_dev(self, params, kf0_dev, kf1_dev, result_ptr, pt_corr_ptr, pt_inlier_ptr, ls_corr_ptr,
                                ls_inlier_ptr, stream=None):
        """Device-pointer form.  kf0_dev / kf1_dev: dicts of device addresses (ints) for pdesc, P, pl, pt_idx, ldesc, sPeP, le,
        ls_idx plus the counts n_pt, n_ls; result_ptr: device memory of sizeof(LcResult) bytes.  Enqueued behind `stream`
        (None = the context's stream), no synchronisation."""
        recs = [LcKeyframe(*(C.c_void_p(k.get(n) or 0) for n in ("pdesc", "P", "pl", "pt_idx")), int(k["n_pt"]), int(k["n_ls"]),
                           *(C.c_void_p(k.get(n) or 0) for n in ("ldesc", "sPeP", "le", "ls_idx"))) for k in (kf0_dev, kf1_dev)]
        _check(self._L.plslam_loop_closure_verify_dev(self._h, C.byref(params), C.byref(recs[0]), C.byref(recs[1]),
                                                      C.c_void_p(result_ptr), C.c_void_p(pt_corr_ptr), C.c_void_p(pt_inlier_ptr),
                                                      C.c_void_p(ls_corr_ptr), C.c_void_p(ls_inlier_ptr),
                                                      C.c_void_p(stream or 0)), "plslam_loop_closure_verify_dev")

    def relpose_robust_gn(self, params, P, pl_obs, sPeP, le_obs):
        """computeRelativePoseRobustGN on given correspondences -> (result dict, pt_inlier, ls_inlier)"""
        P, po = _arr(P, np.float64, (-1, 3)), _arr(pl_obs, np.float64, (-1, 2))
        S, lo = _arr(sPeP, np.float64, (-1, 6)), _arr(le_obs, np.float64, (-1, 3))
        pi, li = np.zeros(P.shape[0], np.uint8), np.zeros(S.shape[0], np.uint8)
        res = LcResult()
        _check(self._L.plslam_relpose_robust_gn(self._h, C.byref(params), _p(P), _p(po), P.shape[0], _p(S), _p(lo), S.shape[0],
                                                C.byref(res), _p(pi), _p(li)), "plslam_relpose_robust_gn")
        return res.as_dict(), pi.astype(bool), li.astype(bool)

    def relpose_robust_gn_batched_dev(self, params, P_ptr, pl_ptr, pt_off_ptr, sPeP_ptr, le_ptr, ls_off_ptr, B, results_ptr,
                                      pt_inlier_ptr, ls_inlier_ptr, stream=None):
        """computeRelativePoseRobustGN for B problems over concatenated device arrays (K54); pt_off / ls_off: B + 1 int32
        offsets in device memory; results_ptr: B x sizeof(LcResult) bytes.  Enqueued behind `stream`, no synchronisation."""
        _check(self._L.plslam_relpose_robust_gn_batched_dev(
            self._h, C.byref(params), *(C.c_void_p(v or 0) for v in (P_ptr, pl_ptr, pt_off_ptr, sPeP_ptr, le_ptr, ls_off_ptr)),
            int(B), C.c_void_p(results_ptr or 0), C.c_void_p(pt_inlier_ptr or 0), C.c_void_p(ls_inlier_ptr or 0),
            C.c_void_p(stream or 0)), "plslam_relpose_robust_gn_batched_dev")

    def stereo_point_gate(self, m12, kp_l, kp_r, max_dist_epip, min_disp):
        """StereoFrame::matchStereoPoints gates -> (stereo_12, disp, n_stereo)."""
        m12 = _arr(m12, np.int32)
        a, b = _arr(kp_l, np.float32, (-1, 2)), _arr(kp_r, np.float32, (-1, 2))
        out, disp = np.empty(m12.shape[0], np.int32), np.empty(m12.shape[0], np.float64)
        n = C.c_int32()
        _check(self._L.plslam_stereo_point_gate(self._h, _p(m12), m12.shape[0], _p(a), _p(b), b.shape[0],
                                                float(max_dist_epip), float(min_disp), _p(out), _p(disp), C.byref(n)),
               "plslam_stereo_point_gate")
        return out, disp, n.value

    def stereo_line_gate(self, m12, seg_l, seg_r, min_disp, line_horiz_th, stereo_overlap_th, ls_min_disp_ratio):
        """StereoFrame::matchStereoLines gates -> (stereo_12, disp_se[n, 2], n_stereo)."""
        m12 = _arr(m12, np.int32)
        a, b = _arr(seg_l, np.float32, (-1, 4)), _arr(seg_r, np.float32, (-1, 4))
        out, disp = np.empty(m12.shape[0], np.int32), np.empty((m12.shape[0], 2), np.float64)
        n = C.c_int32()
        _check(self._L.plslam_stereo_line_gate(self._h, _p(m12), m12.shape[0], _p(a), _p(b), b.shape[0], float(min_disp),
                                               float(line_horiz_th), float(stereo_overlap_th), float(ls_min_disp_ratio),
                                               _p(out), _p(disp), C.byref(n)), "plslam_stereo_line_gate")
        return out, disp, n.value

    def match_batched(self, d1, off1, d2, off2, nnr: float, mutual: bool = True):
        d1 = _arr(d1, np.uint8, (-1, 32))
        d2 = _arr(d2, np.uint8, (-1, 32))
        off1 = _arr(off1, np.int32)
        off2 = _arr(off2, np.int32)
        B = off1.shape[0] - 1
        m12 = np.empty(int(off1[-1]) if B >= 0 else 0, np.int32)
        nm = np.empty(max(B, 0), np.int32)
        _check(self._L.plslam_match_batched(self._h, _p(d1), _p(off1), _p(d2), _p(off2), B, float(nnr),
                                            int(bool(mutual)), _p(m12), _p(nm)), "plslam_match_batched")
        return m12, nm

    def lba_point_rows(self, cam: Cam, homog_th, T_kf_w, Xw, obs_uv, lm_loc, kf_slot):
        T = _arr(T_kf_w, np.float64, (-1, 16))
        Xw = _arr(Xw, np.float64, (-1, 3))
        uv = _arr(obs_uv, np.float64, (-1, 2))
        lm, kf = _arr(lm_loc, np.int32), _arr(kf_slot, np.int32)
        n = uv.shape[0]
        Jp, Jl, r, w = np.empty((n, 6)), np.empty((n, 3)), np.empty(n), np.empty(n)
        _check(self._L.plslam_lba_point_rows(self._h, C.byref(cam), float(homog_th), _p(T), T.shape[0],
                                             _p(Xw), Xw.shape[0], _p(uv), _p(lm), _p(kf), n, _p(Jp),
                                             _p(Jl), _p(r), _p(w)), "plslam_lba_point_rows")
        return Jp, Jl, r, w

    def lba_line_rows(self, cam: Cam, homog_th, T_kf_w, Lw, l_obs, lm_loc, kf_slot,
                      compat_iter_pass: bool = False):
        T = _arr(T_kf_w, np.float64, (-1, 16))
        Lw = _arr(Lw, np.float64, (-1,))
        lo = _arr(l_obs, np.float64, (-1, 3))
        lm, kf = _arr(lm_loc, np.int32), _arr(kf_slot, np.int32)
        n = lo.shape[0]
        Jp, Jl, r, w = np.empty((n, 6)), np.empty((n, 6)), np.empty(n), np.empty(n)
        _check(self._L.plslam_lba_line_rows(self._h, C.byref(cam), float(homog_th),
                                            int(bool(compat_iter_pass)), _p(T), T.shape[0], _p(Lw),
                                            Lw.shape[0], _p(lo), _p(lm), _p(kf), n, _p(Jp), _p(Jl),
                                            _p(r), _p(w)), "plslam_lba_line_rows")
        return Jp, Jl, r, w

    def lba_assemble(self, nkf, npt, nls, pt_lm, pt_kf_loc, pt_rows, ls_lm, ls_kf_loc, ls_rows):
        """Block-form normal equations from point rows (Jp, Jl, r, w) and line rows."""
        plm, pkf = _arr(pt_lm, np.int32), _arr(pt_kf_loc, np.int32)
        llm, lkf = _arr(ls_lm, np.int32), _arr(ls_kf_loc, np.int32)
        pr = [_arr(x, np.float64) for x in pt_rows]
        lr = [_arr(x, np.float64) for x in ls_rows]
        npo, nlo = plm.shape[0], llm.shape[0]
        N = 6 * nkf + 3 * npt + 6 * nls
        g, Hp = np.empty(N), np.empty((nkf, 6, 6))
        Hpt, Hls = np.empty((npt, 3, 3)), np.empty((nls, 6, 6))
        Wp, Wl = np.empty((npo, 3, 6)), np.empty((nlo, 6, 6))
        err = np.empty(1)
        _check(self._L.plslam_lba_assemble(self._h, nkf, npt, nls, _p(plm), _p(pkf), npo, _p(pr[0]), _p(pr[1]),
                                           _p(pr[2]), _p(pr[3]), _p(llm), _p(lkf), nlo, _p(lr[0]), _p(lr[1]),
                                           _p(lr[2]), _p(lr[3]), _p(g), _p(Hp), _p(Hpt), _p(Hls), _p(Wp), _p(Wl),
                                           _p(err)), "plslam_lba_assemble")
        return dict(g=g, H_pose=Hp, H_pt=Hpt, H_ls=Hls, W_pt=Wp, W_ls=Wl, err=float(err[0]))

    def _gate(self, fn, name, cam, Twf, LM, lw, m12, feat, fw, th):
        Twf = _arr(Twf, np.float64, (16,))
        LM = _arr(LM, np.float64, (-1, lw))
        m12 = _arr(m12, np.int32)
        feat = _arr(feat, np.float64, (-1, fw))
        mask = np.empty(m12.shape[0], np.uint8)
        n = C.c_int32()
        _check(fn(self._h, C.byref(cam), _p(Twf), _p(LM), _p(m12), m12.shape[0], _p(feat), feat.shape[0],
                  float(th), _p(mask), C.byref(n)), name)
        return mask, n.value

    def map2kf_point_gate(self, cam, Twf, Xw, m12, pl, max_epip):
        return self._gate(self._L.plslam_map2kf_point_gate, "plslam_map2kf_point_gate", cam, Twf, Xw, 3,
                          m12, pl, 2, max_epip)

    def map2kf_line_gate(self, cam, Twf, Lw, m12, le, max_epip):
        return self._gate(self._L.plslam_map2kf_line_gate, "plslam_map2kf_line_gate", cam, Twf, Lw, 6,
                          m12, le, 3, max_epip)

    def map_point_visible(self, cam, Twf, Xw):
        Twf = _arr(Twf, np.float64, (16,))
        Xw = _arr(Xw, np.float64, (-1, 3))
        vis = np.empty(Xw.shape[0], np.uint8)
        _check(self._L.plslam_map_point_visible(self._h, C.byref(cam), _p(Twf), _p(Xw), Xw.shape[0], _p(vis)),
               "plslam_map_point_visible")
        return vis

    def map_line_visible(self, cam, Twf, Lw):
        Twf = _arr(Twf, np.float64, (16,))
        Lw = _arr(Lw, np.float64, (-1, 6))
        vis = np.empty(Lw.shape[0], np.uint8)
        _check(self._L.plslam_map_line_visible(self._h, C.byref(cam), _p(Twf), _p(Lw), Lw.shape[0], _p(vis)),
               "plslam_map_line_visible")
        return vis

    def median_desc_batched(self, desc_lists, offsets, want_desc=True):
        """MapPoint/MapLine::updateAverageDescDir (src/mapFeatures.cpp:51-84, :121-157) for all landmarks
        -> (med_idx[n_lm], med_desc[n_lm, 32] or None)."""
        d = _arr(desc_lists, np.uint8, (-1, 32))
        off = _arr(offsets, np.int32)
        n_lm = off.shape[0] - 1
        idx = np.empty(max(n_lm, 0), np.int32)
        md = np.empty((max(n_lm, 0), 32), np.uint8) if want_desc else None
        _check(self._L.plslam_median_desc_batched(self._h, _p(d), _p(off), n_lm, _p(idx),
                                                  _p(md) if want_desc else C.c_void_p(None)),
               "plslam_median_desc_batched")
        return idx, md

    def median_desc_batched_dev(self, d_desc_ptr, d_off_ptr, n_lm, total, d_idx_ptr, d_med_ptr=0, stream=None):
        """Device-pointer form; enqueues on `stream` (None = the context's stream), no sync."""
        _check(self._L.plslam_median_desc_batched_dev(self._h, C.c_void_p(d_desc_ptr), C.c_void_p(d_off_ptr),
                                                      int(n_lm), int(total), C.c_void_p(d_idx_ptr),
                                                      C.c_void_p(d_med_ptr or None), C.c_void_p(stream or 0)),
               "plslam_median_desc_batched_dev")

    def lbd_binarise(self, lbd_f32):
        """BinaryDescriptor::computeImpl's binary conversion (binary_descriptor_custom.cpp:653-668):
        n x 72 float32 LBD -> n x 32 uint8 rows."""
        f = _arr(lbd_f32, np.float32, (-1, 72))
        out = np.empty((f.shape[0], 32), np.uint8)
        _check(self._L.plslam_lbd_binarise(self._h, _p(f), f.shape[0], _p(out)), "plslam_lbd_binarise")
        return out

    def lbd_compute(self, dx_img, dy_img, lines, width_of_band=7):
        """BinaryDescriptor::computeLBD for the lines of one octave: (height, width) int16 gradient images and a
        structured array of plslam_lbd_line -> (n, 72) float32."""
        dx, dy = _arr(dx_img, np.int16), _arr(dy_img, np.int16)
        ln = np.ascontiguousarray(lines, dtype=LBD_LINE_DTYPE)
        out = np.empty((ln.shape[0], 72), np.float32)
        _check(self._L.plslam_lbd_compute(self._h, _p(dx), _p(dy), dx.shape[1], dx.shape[0], _p(ln), ln.shape[0],
                                          int(width_of_band), _p(out)), "plslam_lbd_compute")
        return out

    def lbd_compute_dev(self, d_dx_ptr, d_dy_ptr, width, height, lines, d_lbd_ptr, width_of_band=7, stream=None):
        """Device-pointer form (gradient images and the output on the device; the line records are host data)."""
        ln = np.ascontiguousarray(lines, dtype=LBD_LINE_DTYPE)
        _check(self._L.plslam_lbd_compute_dev(self._h, C.c_void_p(d_dx_ptr), C.c_void_p(d_dy_ptr), int(width), int(height),
                                              _p(ln), ln.shape[0], int(width_of_band), C.c_void_p(d_lbd_ptr),
                                              C.c_void_p(stream or 0)), "plslam_lbd_compute_dev")

    def lbd_binarise_dev(self, d_lbd_ptr, n, d_desc_ptr, stream=None):
        """Device-pointer form; enqueues on `stream` (None = the context's stream), no sync."""
        _check(self._L.plslam_lbd_binarise_dev(self._h, C.c_void_p(d_lbd_ptr), int(n),
                                               C.c_void_p(d_desc_ptr), C.c_void_p(stream or 0)),
               "plslam_lbd_binarise_dev")

    def map2kf_match(self, kind, cam, Twf, LM, med_desc, candidate, kf_desc, kf_feat, kf_idx, nnr, mutual,
                     max_epip, min_matches):
        """MapHandler::matchMap2KFPoints / matchMap2KFLines (compute part) -> (map_to_kf, n_matches)."""
        lw, fw = (3, 2) if kind == "points" else (6, 3)
        Twf = _arr(Twf, np.float64, (16,))
        LM = _arr(LM, np.float64, (-1, lw))
        md, cand = _arr(med_desc, np.uint8, (-1, 32)), _arr(candidate, np.uint8)
        kd, kf = _arr(kf_desc, np.uint8, (-1, 32)), _arr(kf_feat, np.float64, (-1, fw))
        ki = _arr(kf_idx, np.int32)
        out = np.empty(LM.shape[0], np.int32)
        n = C.c_int32()
        fn = self._L.plslam_map2kf_match_points if kind == "points" else self._L.plslam_map2kf_match_lines
        _check(fn(self._h, C.byref(cam), _p(Twf), _p(LM), _p(md), _p(cand), LM.shape[0], _p(kd), _p(kf), _p(ki),
                  kd.shape[0], float(nnr), int(bool(mutual)), float(max_epip), int(min_matches), _p(out),
                  C.byref(n)), "plslam_map2kf_match_" + kind)
        return out, n.value

    def map2kf_match_fast(self, kind, cam, Twf, LM, med_desc, candidate, kf_desc, kf_feat, kf_idx, nnr, mutual,
                          max_epip, min_matches, fm, kf_seg=None):
        """The drivers with SlamConfig::fastMatching() (matchGrid first, StVO::match when it finds too little)
        -> (map_to_kf, n_matches, used_match).  fm: dict with the fields of plslam_fast_matching."""
        lw, fw = (3, 2) if kind == "points" else (6, 3)
        Twf = _arr(Twf, np.float64, (16,))
        LM = _arr(LM, np.float64, (-1, lw))
        md, cand = _arr(med_desc, np.uint8, (-1, 32)), _arr(candidate, np.uint8)
        kd, kf = _arr(kf_desc, np.uint8, (-1, 32)), _arr(kf_feat, np.float64, (-1, fw))
        ki = _arr(kf_idx, np.int32)
        out = np.empty(LM.shape[0], np.int32)
        F = _fast_matching(fm)
        n, used = C.c_int32(), C.c_int32()
        if kind == "points":
            _check(self._L.plslam_map2kf_match_points_fast(self._h, C.byref(cam), _p(Twf), _p(LM), _p(md), _p(cand),
                                                           LM.shape[0], _p(kd), _p(kf), _p(ki), kd.shape[0], float(nnr),
                                                           int(bool(mutual)), float(max_epip), int(min_matches),
                                                           C.byref(F), _p(out), C.byref(n), C.byref(used)),
                   "plslam_map2kf_match_points_fast")
        else:
            sg = _arr(kf_seg, np.float64, (-1, 4))
            _check(self._L.plslam_map2kf_match_lines_fast(self._h, C.byref(cam), _p(Twf), _p(LM), _p(md), _p(cand),
                                                          LM.shape[0], _p(kd), _p(kf), _p(sg), _p(ki), kd.shape[0],
                                                          float(nnr), int(bool(mutual)), float(max_epip),
                                                          int(min_matches), C.byref(F), _p(out), C.byref(n),
                                                          C.byref(used)), "plslam_map2kf_match_lines_fast")
        return out, n.value, used.value

    def map2kf_match_dev(self, kind, cam, Twf, d_LM, d_med_desc, d_candidate, n_map, kf_desc, kf_feat, kf_idx, nnr, mutual,
                         max_epip, min_matches, fm, kf_seg=None):
        """map2kf_match_fast with the MAP SIDE on the device: d_LM (n_map x 3 | 6 float64), d_med_desc (n_map x 32 uint8),
        d_candidate (n_map uint8) are device addresses (ints); the keyframe side and the results are host arrays."""
        fw = 2 if kind == "points" else 3
        Twf = _arr(Twf, np.float64, (16,))
        kd, kf = _arr(kf_desc, np.uint8, (-1, 32)), _arr(kf_feat, np.float64, (-1, fw))
        ki = _arr(kf_idx, np.int32)
        out = np.empty(int(n_map), np.int32)
        F = _fast_matching(fm)
        n, used = C.c_int32(), C.c_int32()
        if kind == "points":
            _check(self._L.plslam_map2kf_match_points_dev(self._h, C.byref(cam), _p(Twf), int(d_LM), int(d_med_desc),
                                                          int(d_candidate), int(n_map), _p(kd), _p(kf), _p(ki), kd.shape[0],
                                                          float(nnr), int(bool(mutual)), float(max_epip), int(min_matches),
                                                          C.byref(F), _p(out), C.byref(n), C.byref(used)),
                   "plslam_map2kf_match_points_dev")
        else:
            sg = _arr(kf_seg, np.float64, (-1, 4))
            _check(self._L.plslam_map2kf_match_lines_dev(self._h, C.byref(cam), _p(Twf), int(d_LM), int(d_med_desc),
                                                         int(d_candidate), int(n_map), _p(kd), _p(kf), _p(sg), _p(ki),
                                                         kd.shape[0], float(nnr), int(bool(mutual)), float(max_epip),
                                                         int(min_matches), C.byref(F), _p(out), C.byref(n), C.byref(used)),
                   "plslam_map2kf_match_lines_dev")
        return out, n.value, used.value

    def kf2kf_match(self, kind, cam, DT, X_prev, desc_prev, feat_curr, desc_curr, nnr, mutual, min_matches, fm):
        """MapHandler::matchKF2KFPoints / Lines compute part -> (matches_12, n_matches, used_match)."""
        xw, fw = (3, 2) if kind == "points" else (6, 4)
        DT = _arr(DT, np.float64, (16,))
        X = _arr(X_prev, np.float64, (-1, xw))
        dp, dc = _arr(desc_prev, np.uint8, (-1, 32)), _arr(desc_curr, np.uint8, (-1, 32))
        fc = _arr(feat_curr, np.float64, (-1, fw))
        out = np.empty(X.shape[0], np.int32)
        F = _fast_matching(fm)
        n, used = C.c_int32(), C.c_int32()
        fn = self._L.plslam_kf2kf_match_points if kind == "points" else self._L.plslam_kf2kf_match_lines
        _check(fn(self._h, C.byref(cam), _p(DT), _p(X), _p(dp), X.shape[0], _p(fc), _p(dc), fc.shape[0], float(nnr),
                  int(bool(mutual)), int(min_matches), C.byref(F), _p(out), C.byref(n), C.byref(used)),
               "plslam_kf2kf_match_" + kind)
        return out, n.value, used.value

    def kf2kf_match_dev(self, kind, cam, DT, d_X_prev, d_desc_prev, n_prev, feat_curr, d_desc_curr, nnr, mutual, min_matches, fm):
        """kf2kf_match with the ROWS on the device: d_X_prev (n_prev x 3 | 6 float64), d_desc_prev (n_prev x 32 uint8) and
        d_desc_curr (len(feat_curr) x 32 uint8) are device addresses (ints); feat_curr and the results are host arrays."""
        fw = 2 if kind == "points" else 4
        DT = _arr(DT, np.float64, (16,))
        fc = _arr(feat_curr, np.float64, (-1, fw))
        out = np.empty(int(n_prev), np.int32)
        F = _fast_matching(fm)
        n, used = C.c_int32(), C.c_int32()
        fn = self._L.plslam_kf2kf_match_points_dev if kind == "points" else self._L.plslam_kf2kf_match_lines_dev
        _check(fn(self._h, C.byref(cam), _p(DT), int(d_X_prev), int(d_desc_prev), int(n_prev), _p(fc), int(d_desc_curr),
                  fc.shape[0], float(nnr), int(bool(mutual)), int(min_matches), C.byref(F), _p(out), C.byref(n), C.byref(used)),
               "plslam_kf2kf_match_" + kind + "_dev")
        return out, n.value, used.value

    # ---- device-pointer calls ----------------------------------------------------------------
    def lba_point_rows_dev(self, cam, homog_th, T, Xw, uv, lm, kf, nobs, Jp, Jl, r, w, stream=0, n_pose_slots=0):
        """n_pose_slots: how many 4 x 4 matrices T holds (0 = not stated: the kernels gather them from global memory)."""
        _check(self._L.plslam_lba_point_rows_dev_n(self._h, C.byref(cam), float(homog_th), T, int(n_pose_slots), Xw, uv, lm, kf,
                                                   int(nobs), Jp, Jl, r, w, stream or None),
               "plslam_lba_point_rows_dev_n")

    def lba_line_rows_dev(self, cam, homog_th, compat, T, Lw, lo, lm, kf, nobs, Jp, Jl, r, w, stream=0, n_pose_slots=0):
        _check(self._L.plslam_lba_line_rows_dev_n(self._h, C.byref(cam), float(homog_th), int(bool(compat)), T, int(n_pose_slots),
                                                  Lw, lo, lm, kf, int(nobs), Jp, Jl, r, w, stream or None),
               "plslam_lba_line_rows_dev_n")

    def plan(self, problems) -> "MatchPlan":
        return MatchPlan(self, problems)


class PinnedArray:
    """A numpy view of page-locked host memory (plslam_pinned_alloc): what a host-to-host pipeline should be fed from."""

    def __init__(self, ctx: "Context", shape, dtype):
        self._L = ctx._L
        self.nbytes = int(np.prod(shape)) * np.dtype(dtype).itemsize
        self._ptr = self._L.plslam_pinned_alloc(max(self.nbytes, 1))
        if not self._ptr:
            raise PlslamError(ENOMEM, "plslam_pinned_alloc", f"no page-locked host memory for {max(self.nbytes, 1)} bytes")
        self.array = np.ctypeslib.as_array((C.c_uint8 * max(self.nbytes, 1)).from_address(self._ptr))[:self.nbytes] \
            .view(dtype).reshape(shape)

    def close(self):
        if getattr(self, "_ptr", None):
            self.array = None
            self._L.plslam_pinned_free(self._ptr)
            self._ptr = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
