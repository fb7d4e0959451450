"""ctypes binding of include/plslam_hip.h (libplslam_hip.so).

This module is plumbing: it declares the C-ABI entry points and wraps them for numpy
(host-pointer calls) and raw device pointers (plans).  It contains no algorithm and has NO
CPU fallback: if the HIP library is missing it raises, and without a gfx950 device
``Context()`` raises ``PlslamError(PLSLAM_ENODEV)``.
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
SCAN_AUTO, SCAN_LANE_PER_QUERY, SCAN_WAVE_PER_QUERY, SCAN_SYMMETRIC, SCAN_MFMA = 0, 1, 2, 3, 4
MAX_TRAIN_ROWS = 1 << 23

# every symbol include/plslam_hip.h declares (tests check the .so exports all of them)
ABI_VERSION = 5          # include/plslam_hip.h: PLSLAM_ABI_VERSION
ABI_SYMBOLS = (
    "plslam_strerror", "plslam_last_error", "plslam_abi_version",
    "plslam_ctx_create", "plslam_ctx_destroy", "plslam_ctx_set_option", "plslam_ctx_get_option",
    "plslam_ctx_device_info",
    "plslam_knn2_hamming256", "plslam_match", "plslam_match_prior", "plslam_match_batched",
    "plslam_match_plan_create", "plslam_match_plan_run", "plslam_match_plan_run_split", "plslam_match_plan_set_profiling",
    "plslam_match_plan_elapsed", "plslam_match_plan_info", "plslam_match_plan_dump", "plslam_match_plan_key_state", "plslam_match_plan_destroy",
    "plslam_lba_point_rows", "plslam_lba_line_rows", "plslam_lba_point_rows_dev",
    "plslam_lba_line_rows_dev", "plslam_lba_assemble", "plslam_lba_plan_create", "plslam_lba_plan_iterate",
    "plslam_lba_plan_rows", "plslam_lba_plan_destroy", "plslam_lba_plan_iterate_dev", "plslam_lba_plan_device_blocks", "plslam_lba_plan_device_state",
    "plslam_lba_plan_iterate_resident", "plslam_lba_plan_diag_max", "plslam_lba_plan_schur", "plslam_lba_plan_backsub",
    "plslam_lba_plan_set_poses", "plslam_lba_plan_host_state", "plslam_lba_plan_get_landmarks",
    "plslam_lba_plan_iterate_schur", "plslam_lba_plan_apply_step", "plslam_lba_point_rows_dev_n", "plslam_lba_line_rows_dev_n", "plslam_rccl_available",
    "plslam_lba_plan_blocks", "plslam_lba_plan_create_dev", "plslam_lba_plan_list_sizes", "plslam_lba_plan_lists",
    "plslam_lba_plan_optimize_dev", "plslam_lba_reduced_ldlt_solve",
    "plslam_map2kf_point_gate", "plslam_map2kf_line_gate", "plslam_map_point_visible",
    "plslam_map_line_visible", "plslam_map2kf_match_points", "plslam_map2kf_match_lines",
    "plslam_map2kf_match_points_fast", "plslam_map2kf_match_lines_fast", "plslam_map2kf_match_points_dev", "plslam_map2kf_match_lines_dev",
    "plslam_kf2kf_match_points", "plslam_kf2kf_match_lines", "plslam_kf2kf_match_points_dev", "plslam_kf2kf_match_lines_dev",
    "plslam_lbd_binarise", "plslam_lbd_binarise_dev", "plslam_lbd_compute", "plslam_lbd_compute_dev",
    "plslam_median_desc_batched", "plslam_median_desc_batched_dev",
    "plslam_stereo_point_gate", "plslam_stereo_line_gate", "plslam_stereo_point_gate_dev", "plslam_stereo_line_gate_dev",
    "plslam_match_plan_add_stereo_gates", "plslam_match_plan_set_wire16", "plslam_pose_gn_accumulate",
    "plslam_match_pipeline_create", "plslam_match_pipeline_submit", "plslam_match_pipeline_wait",
    "plslam_match_pipeline_destroy", "plslam_pinned_alloc", "plslam_pinned_free",
    "plslam_match_grid", "plslam_grid_plan_create", "plslam_grid_plan_run", "plslam_grid_plan_overflows",
    "plslam_grid_plan_destroy", "plslam_grid_pair_capacity", "plslam_grid_pair_capacity_bound",
    "plslam_gather_match_tables", "plslam_rccl_use", "plslam_match_plan_step_gather", "plslam_match_plan_gather_sync",
    "plslam_bow_vocab_create", "plslam_bow_vocab_destroy", "plslam_bow_transform", "plslam_bow_transform_dev",
    "plslam_bow_db_create", "plslam_bow_db_destroy", "plslam_bow_db_insert", "plslam_bow_db_insert_dev", "plslam_bow_db_size",
    "plslam_bow_db_score",
    "plslam_loop_closure_verify", "plslam_loop_closure_verify_dev", "plslam_relpose_robust_gn",
    "plslam_lc_batch_create", "plslam_lc_batch_destroy", "plslam_lc_batch_verify", "plslam_lc_batch_verify_dev",
    "plslam_relpose_robust_gn_batched_dev",
    "plslam_gba_plan_create", "plslam_gba_optimize", "plslam_gba_plan_destroy", "plslam_dense_ldlt_solve",
    "plslam_gba_plan_create_dev", "plslam_gba_plan_list_sizes", "plslam_gba_plan_lists", "plslam_gba_optimize_dev",
    "plslam_pgo_plan_create", "plslam_pgo_optimize", "plslam_pgo_plan_destroy", "plslam_lc_correct_map",
    "plslam_lc_correct_map_dev", "plslam_envelope_ldlt_solve",
    "plslam_local_map_create", "plslam_local_map_destroy", "plslam_local_map_form", "plslam_local_map_candidates",
    "plslam_local_map_gather", "plslam_local_map_cull", "plslam_local_map_device_buffers", "plslam_local_map_download",
    "plslam_local_map_apply_lba", "plslam_local_map_form_all", "plslam_local_map_apply_gba",
    "plslam_map_insert_create", "plslam_map_insert_destroy", "plslam_map_insert_kf2kf", "plslam_map_insert_map2kf",
    "plslam_map_insert_device_buffers", "plslam_map_insert_download",
    "plslam_lc_fuse_create", "plslam_lc_fuse_destroy", "plslam_lc_fuse_run", "plslam_lc_fuse_device_buffers",
    "plslam_lc_fuse_download",
    "plslam_map_lists_refresh", "plslam_map_insert_carry", "plslam_lc_fuse_carry",
    "plslam_lc_correct_image",
)
BOW_TF_IDF, BOW_TF, BOW_IDF, BOW_BINARY = 0, 1, 2, 3
BOW_L1_NORM = 0
BOW_MAX_SET = 16384      # include/plslam_hip.h: PLSLAM_BOW_MAX_SET
LC_MAX_FEATURES = 16384  # include/plslam_hip.h: PLSLAM_LC_MAX_FEATURES
LC_MAX_ITERS = 10000     # include/plslam_hip.h: PLSLAM_LC_MAX_ITERS
LC_MAX_BATCH = 65536     # include/plslam_hip.h: PLSLAM_LC_MAX_BATCH
GBA_MAX_KEYFRAMES = 4096  # include/plslam_hip.h: PLSLAM_GBA_MAX_KEYFRAMES
GBA_STOP_MAX_ITERS, GBA_STOP_ERR, GBA_STOP_DX = 0, 1, 2
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


class Cam(C.Structure):
    """plslam_cam"""
    _fields_ = [("fx", C.c_double), ("fy", C.c_double), ("cx", C.c_double), ("cy", C.c_double),
                ("b", C.c_double), ("width", C.c_int32), ("height", C.c_int32)]


class MatchProblem(C.Structure):
    """plslam_match_problem (device pointers)"""
    _fields_ = [("d1", C.c_void_p), ("d2", C.c_void_p), ("n1", C.c_int32), ("n2", C.c_int32),
                ("nnr", C.c_float), ("mutual", C.c_int32), ("matches_12", C.c_void_p),
                ("n_matches", C.c_void_p), ("keep_prior", C.c_int32), ("reserved", C.c_int32)]


class StereoGateProblem(C.Structure):
    """plslam_stereo_gate_problem (device pointers)"""
    _fields_ = [("matches_12", C.c_void_p), ("f_l", C.c_void_p), ("f_r", C.c_void_p), ("n_l", C.c_int32),
                ("n_r", C.c_int32), ("lines", C.c_int32), ("pad", C.c_int32), ("max_dist_epip", C.c_double),
                ("min_disp", C.c_double), ("line_horiz_th", C.c_double), ("stereo_overlap_th", C.c_double),
                ("ls_min_disp_ratio", C.c_double), ("stereo_12", C.c_void_p), ("disp", C.c_void_p),
                ("n_stereo", C.c_void_p)]


class GatherStep(C.Structure):
    """plslam_gather_step (include/plslam_hip.h)"""
    _fields_ = [("comm", C.c_void_p), ("nranks", C.c_int32), ("rank", C.c_int32), ("root", C.c_int32), ("wire_bytes", C.c_int32),
                ("send", C.c_void_p), ("n_entries", C.c_int64), ("recv", C.c_void_p), ("wide", C.c_void_p),
                ("scan_stream", C.c_void_p), ("post_stream", C.c_void_p), ("comm_stream", C.c_void_p)]


class ArenaProblem(C.Structure):
    """plslam_arena_problem"""
    _fields_ = [("d1_off", C.c_int64), ("d2_off", C.c_int64), ("n1", C.c_int32), ("n2", C.c_int32), ("nnr", C.c_float),
                ("mutual", C.c_int32), ("out_off", C.c_int64)]


class GridProblem(C.Structure):
    """plslam_grid_problem (device pointers)"""
    _fields_ = [("d1", C.c_void_p), ("d2", C.c_void_p), ("centres1", C.c_void_p), ("cell_start", C.c_void_p),
                ("cell_items", C.c_void_p), ("dir1", C.c_void_p), ("dir2", C.c_void_p),
                ("n1", C.c_int32), ("n2", C.c_int32), ("n_centres", C.c_int32), ("grid_cols", C.c_int32),
                ("grid_rows", C.c_int32), ("n_items", C.c_int32), ("window", C.c_int32 * 4), ("sim_th", C.c_double), ("nnr", C.c_double),
                ("mutual", C.c_int32), ("pair_capacity", C.c_int32), ("matches_12", C.c_void_p),
                ("n_matches", C.c_void_p)]


class FastMatching(C.Structure):
    """plslam_fast_matching"""
    _fields_ = [("enabled", C.c_int32), ("grid_cols", C.c_int32), ("grid_rows", C.c_int32), ("ws", C.c_int32),
                ("inv_width", C.c_double), ("inv_height", C.c_double), ("nnr_grid", C.c_double),
                ("line_sim_th", C.c_double)]


class PlanInfo(C.Structure):
    """plslam_plan_info"""
    _fields_ = [("distance_evals", C.c_int64), ("directed_evals", C.c_int64),
                ("algorithmic_bytes", C.c_int64), ("n_scans", C.c_int32),
                ("scan_blocks", C.c_int32), ("scan_variant", C.c_int32),
                ("scan_block_threads", C.c_int32)]


class BowVocabDesc(C.Structure):
    """plslam_bow_vocab_desc"""
    _fields_ = [("k", C.c_int32), ("L", C.c_int32), ("scoring_type", C.c_int32), ("weighting_type", C.c_int32),
                ("n_nodes", C.c_int32), ("n_words", C.c_int32), ("nodes", C.c_void_p), ("words", C.c_void_p)]


class BowPlStats(C.Structure):
    """plslam_bow_pl_stats"""
    _fields_ = [("n_pt", C.c_int32), ("n_ls", C.c_int32), ("std_pt", C.c_double), ("std_ls", C.c_double)]


class LcParams(C.Structure):
    """plslam_lc_params (plslam_amd.loop_closure.params() builds one from the shipped configuration)"""
    _fields_ = [("cam", Cam), ("homog_th", C.c_double), ("min_ratio_12_p", C.c_float), ("min_ratio_12_l", C.c_float),
                ("mutual", C.c_int32), ("has_points", C.c_int32), ("has_lines", C.c_int32), ("max_iters", C.c_int32),
                ("max_iters_ref", C.c_int32), ("reserved", C.c_int32), ("lc_inlier_ratio", C.c_double),
                ("lc_res", C.c_double), ("lc_unc", C.c_double), ("lc_inl", C.c_double), ("lc_trs", C.c_double),
                ("lc_rot", C.c_double)]


class LcKeyframe(C.Structure):
    """plslam_lc_keyframe"""
    _fields_ = [("pdesc", C.c_void_p), ("P", C.c_void_p), ("pl", C.c_void_p), ("pt_idx", C.c_void_p), ("n_pt", C.c_int32),
                ("n_ls", C.c_int32), ("ldesc", C.c_void_p), ("sPeP", C.c_void_p), ("le", C.c_void_p), ("ls_idx", C.c_void_p)]


class LcResult(C.Structure):
    """plslam_lc_result"""
    _fields_ = [(n, C.c_int32) for n in ("is_lc", "gn_ran", "common_pt", "common_ls", "n_pt_inliers", "n_ls_inliers", "iters_1",
                                          "iters_2", "ok_res", "ok_unc", "ok_inl", "ok_trs", "ok_rot", "reserved")] + \
              [(n, C.c_double) for n in ("inl_ratio_pt", "inl_ratio_ls", "e", "cov_eig", "ratio_inliers", "t", "r")] + \
              [("x_inc", C.c_double * 6), ("T_inc", C.c_double * 16), ("pose_inc", C.c_double * 6), ("H", C.c_double * 36),
               ("g", C.c_double * 6), ("clk_total", C.c_int64), ("clk_serial", C.c_int64)]

    def as_dict(self):
        """the record as plain Python values / numpy arrays (T_inc 4 x 4, H 6 x 6)"""
        d = {}
        for name, _ in self._fields_:
            v = getattr(self, name)
            d[name] = np.ctypeslib.as_array(v).copy() if not isinstance(v, (int, float)) else v
        d["T_inc"] = d["T_inc"].reshape(4, 4)
        d["H"] = d["H"].reshape(6, 6)
        return d


# plslam_bow_node / plslam_bow_word as numpy records
BOW_NODE_DTYPE = np.dtype([("node_id", np.int32), ("parent_id", np.int32), ("weight", np.float64), ("descriptor", np.uint8, 32)])
BOW_WORD_DTYPE = np.dtype([("word_id", np.int32), ("node_id", np.int32)])

# plslam_lbd_line as a numpy record
LBD_LINE_DTYPE = np.dtype([("num_pixels", np.int32), ("sx", np.float32), ("sy", np.float32), ("ex", np.float32),
                           ("ey", np.float32), ("direction", np.float32)])


class PlslamError(RuntimeError):
    def __init__(self, code: int, where: str, detail: str = ""):
        self.code = code
        super().__init__(f"{where}: {code} ({detail})")


_lib = None


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


# every entry point returns an int status except these (load() gives each name of ABI_SYMBOLS its return type from here).
_RESTYPES = {
    "plslam_strerror": C.c_char_p, "plslam_last_error": C.c_char_p,
    "plslam_pinned_alloc": C.c_void_p, "plslam_pinned_free": None,
    "plslam_grid_pair_capacity": C.c_int64, "plslam_grid_pair_capacity_bound": C.c_int64,
    "plslam_ctx_destroy": None, "plslam_match_plan_destroy": None, "plslam_lba_plan_destroy": None,
    "plslam_grid_plan_destroy": None, "plslam_match_pipeline_destroy": None, "plslam_bow_vocab_destroy": None,
    "plslam_bow_db_destroy": None, "plslam_gba_plan_destroy": None, "plslam_pgo_plan_destroy": None,
    "plslam_local_map_destroy": None, "plslam_map_insert_destroy": None, "plslam_lc_fuse_destroy": None,
    "plslam_lc_batch_destroy": None,
}


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
    vp, i32, f64 = C.c_void_p, C.c_int32, C.c_double
    L.plslam_strerror.argtypes = [C.c_int]
    L.plslam_last_error.argtypes = []
    L.plslam_abi_version.restype = C.c_int
    L.plslam_abi_version.argtypes = []
    if L.plslam_abi_version() != ABI_VERSION:
        raise RuntimeError(f"libplslam_hip.so has ABI version {L.plslam_abi_version()}, these bindings were written for {ABI_VERSION} "
                           "(struct layouts differ: rebuild with plslam_amd/build.py)")
    L.plslam_lbd_binarise.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]
    L.plslam_lbd_binarise_dev.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]
    L.plslam_median_desc_batched.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]
    L.plslam_median_desc_batched_dev.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p,
                                                 C.c_void_p, C.c_void_p]
    L.plslam_ctx_create.argtypes = [C.c_int, C.POINTER(vp)]
    L.plslam_ctx_destroy.argtypes = [vp]
    L.plslam_ctx_set_option.argtypes = [vp, C.c_char_p, C.c_int]
    L.plslam_ctx_get_option.argtypes = [vp, C.c_char_p, C.POINTER(C.c_int)]
    L.plslam_ctx_device_info.argtypes = [vp, C.POINTER(i32), C.POINTER(i32), C.POINTER(i32),
                                         C.c_char_p, i32]
    L.plslam_knn2_hamming256.argtypes = [vp, vp, i32, vp, i32, vp, vp]
    L.plslam_match.argtypes = [vp, vp, i32, vp, i32, C.c_float, C.c_int, vp, C.POINTER(i32)]
    L.plslam_match_prior.argtypes = L.plslam_match.argtypes
    L.plslam_match_batched.argtypes = [vp, vp, vp, vp, vp, i32, C.c_float, C.c_int, vp, vp]
    L.plslam_match_plan_create.argtypes = [vp, C.POINTER(MatchProblem), i32, C.POINTER(vp)]
    L.plslam_match_plan_run.argtypes = [vp, vp]
    L.plslam_match_plan_run_split.argtypes = [vp, vp, vp]
    L.plslam_match_plan_set_profiling.argtypes = [vp, C.c_int]
    L.plslam_match_plan_elapsed.argtypes = [vp, C.POINTER(f64), C.POINTER(f64), C.POINTER(C.c_int64)]
    L.plslam_match_plan_info.argtypes = [vp, C.POINTER(PlanInfo)]
    L.plslam_match_plan_dump.argtypes = [vp, vp, C.c_size_t, vp, C.c_size_t, C.POINTER(C.c_size_t),
                                         C.POINTER(C.c_size_t)]
    L.plslam_match_plan_key_state.argtypes = [vp, C.POINTER(C.c_int32)]
    L.plslam_match_plan_destroy.argtypes = [vp]
    L.plslam_lba_point_rows.argtypes = [vp, C.POINTER(Cam), f64, vp, i32, vp, i32, vp, vp, vp, i32,
                                        vp, vp, vp, vp]
    L.plslam_lba_line_rows.argtypes = [vp, C.POINTER(Cam), f64, C.c_int, vp, i32, vp, i32, vp, vp, vp,
                                       i32, vp, vp, vp, vp]
    L.plslam_lba_point_rows_dev.argtypes = [vp, C.POINTER(Cam), f64, vp, vp, vp, vp, vp, i32,
                                            vp, vp, vp, vp, vp]
    L.plslam_lba_line_rows_dev.argtypes = [vp, C.POINTER(Cam), f64, C.c_int, vp, vp, vp, vp, vp, i32,
                                           vp, vp, vp, vp, vp]
    L.plslam_lba_assemble.argtypes = [vp, i32, i32, i32, vp, vp, i32, vp, vp, vp, vp, vp, vp, i32, vp, vp, vp, vp,
                                      vp, vp, vp, vp, vp, vp, vp]
    L.plslam_lba_point_rows_dev_n.argtypes = [vp, C.POINTER(Cam), f64, vp, i32, vp, vp, vp, vp, i32, vp, vp, vp, vp, vp]
    L.plslam_lba_line_rows_dev_n.argtypes = [vp, C.POINTER(Cam), f64, C.c_int, vp, i32, vp, vp, vp, vp, i32, vp, vp, vp, vp, vp]
    L.plslam_lba_plan_create.argtypes = [vp, C.POINTER(Cam), f64, i32, i32, i32, i32, vp, vp, vp, vp, i32, vp, vp, vp, vp,
                                         i32, C.POINTER(vp)]
    L.plslam_lba_plan_iterate.argtypes = [vp, vp, vp, vp, C.c_int, vp, vp, vp, vp, vp, vp, vp]
    L.plslam_lba_plan_rows.argtypes = [vp] * 9
    L.plslam_lba_plan_iterate_dev.argtypes = [vp, vp, vp, vp, C.c_int, vp, vp]
    L.plslam_lba_plan_device_blocks.argtypes = [vp, vp]
    L.plslam_lba_plan_device_state.argtypes = [vp, vp]
    L.plslam_lba_plan_iterate_resident.argtypes = [vp, C.c_int, vp]
    L.plslam_lba_plan_diag_max.argtypes = [vp, vp]
    L.plslam_lba_plan_schur.argtypes = [vp, C.c_double, vp, vp, vp]
    L.plslam_lba_plan_backsub.argtypes = [vp, vp, C.c_int, vp, vp]
    L.plslam_lba_plan_set_poses.argtypes = [vp, vp]
    L.plslam_lba_plan_get_landmarks.argtypes = [vp, vp, vp]
    L.plslam_lba_plan_iterate_schur.argtypes = [vp, C.c_int, C.c_double, vp, vp, vp, vp]
    L.plslam_lba_plan_apply_step.argtypes = [vp, vp, vp, C.c_int, vp]
    L.plslam_lba_plan_host_state.argtypes = [vp, vp]
    L.plslam_lba_plan_blocks.argtypes = [vp] * 8
    L.plslam_lba_plan_destroy.argtypes = [vp]
    L.plslam_lba_plan_create_dev.argtypes = [vp, C.POINTER(Cam), f64, i32, i32, i32, i32, vp, vp, vp, vp, i32, vp, vp, vp, vp, i32,
                                             vp, vp, i32, C.POINTER(vp)]
    L.plslam_lba_plan_list_sizes.argtypes = [vp, C.c_int, vp]
    L.plslam_lba_plan_lists.argtypes = [vp, vp]
    L.plslam_lba_plan_optimize_dev.argtypes = [vp, C.POINTER(LbaLmParams), vp, vp, i32, vp, vp, vp, C.POINTER(LbaResult)]
    L.plslam_lba_reduced_ldlt_solve.argtypes = [vp, i32, vp, vp, vp, C.POINTER(i32)]
    for f in (L.plslam_map2kf_point_gate, L.plslam_map2kf_line_gate):
        f.argtypes = [vp, C.POINTER(Cam), vp, vp, vp, i32, vp, i32, f64, vp, C.POINTER(i32)]
    for f in (L.plslam_map_point_visible, L.plslam_map_line_visible):
        f.argtypes = [vp, C.POINTER(Cam), vp, vp, i32, vp]
    for f in (L.plslam_map2kf_match_points, L.plslam_map2kf_match_lines):
        f.argtypes = [vp, C.POINTER(Cam), vp, vp, vp, vp, i32, vp, vp, vp, i32, C.c_float, C.c_int, f64, i32, vp,
                      C.POINTER(i32)]
    L.plslam_map2kf_match_points_fast.argtypes = [vp, C.POINTER(Cam), vp, vp, vp, vp, i32, vp, vp, vp, i32, C.c_float,
                                                  C.c_int, f64, i32, C.POINTER(FastMatching), vp, C.POINTER(i32),
                                                  C.POINTER(i32)]
    L.plslam_map2kf_match_lines_fast.argtypes = [vp, C.POINTER(Cam), vp, vp, vp, vp, i32, vp, vp, vp, vp, i32, C.c_float,
                                                 C.c_int, f64, i32, C.POINTER(FastMatching), vp, C.POINTER(i32),
                                                 C.POINTER(i32)]
    L.plslam_map2kf_match_points_dev.argtypes = L.plslam_map2kf_match_points_fast.argtypes
    L.plslam_map2kf_match_lines_dev.argtypes = L.plslam_map2kf_match_lines_fast.argtypes
    for f in (L.plslam_kf2kf_match_points, L.plslam_kf2kf_match_lines, L.plslam_kf2kf_match_points_dev,
              L.plslam_kf2kf_match_lines_dev):
        f.argtypes = [vp, C.POINTER(Cam), vp, vp, vp, i32, vp, vp, i32, C.c_float, C.c_int, i32, C.POINTER(FastMatching), vp,
                      C.POINTER(i32), C.POINTER(i32)]
    L.plslam_pose_gn_accumulate.argtypes = [vp, C.POINTER(Cam), f64, vp, vp, vp, vp, i32, vp, vp, vp, i32, vp, vp, vp, vp]
    L.plslam_lbd_compute.argtypes = [vp, vp, vp, i32, i32, vp, i32, i32, vp]
    L.plslam_lbd_compute_dev.argtypes = [vp, vp, vp, i32, i32, vp, i32, i32, vp, vp]
    L.plslam_stereo_point_gate.argtypes = [vp, vp, i32, vp, vp, i32, f64, f64, vp, vp, C.POINTER(i32)]
    L.plslam_stereo_line_gate.argtypes = [vp, vp, i32, vp, vp, i32, f64, f64, f64, f64, vp, vp, C.POINTER(i32)]
    L.plslam_stereo_point_gate_dev.argtypes = [vp, vp, i32, vp, vp, i32, f64, f64, vp, vp, vp, vp]
    L.plslam_stereo_line_gate_dev.argtypes = [vp, vp, i32, vp, vp, i32, f64, f64, f64, f64, vp, vp, vp, vp]
    L.plslam_match_plan_add_stereo_gates.argtypes = [vp, C.POINTER(StereoGateProblem), i32]
    L.plslam_match_plan_set_wire16.argtypes = [vp, vp, vp, C.c_size_t]
    L.plslam_match_pipeline_create.argtypes = [vp, C.c_size_t, C.POINTER(ArenaProblem), i32, C.c_size_t, i32, C.POINTER(vp)]
    L.plslam_match_pipeline_submit.argtypes = [vp, vp, vp, vp]
    L.plslam_match_pipeline_wait.argtypes = [vp]
    L.plslam_match_pipeline_destroy.argtypes = [vp]
    L.plslam_pinned_alloc.argtypes = [C.c_size_t]
    L.plslam_pinned_free.argtypes = [vp]
    L.plslam_match_grid.argtypes = [vp, vp, i32, vp, i32, vp, vp, i32, i32, vp, i32, vp, vp, f64, vp, f64, C.c_int, vp,
                                    C.POINTER(i32)]
    L.plslam_grid_plan_create.argtypes = [vp, C.POINTER(GridProblem), i32, C.POINTER(vp)]
    L.plslam_grid_plan_run.argtypes = [vp, vp]
    L.plslam_grid_plan_overflows.argtypes = [vp, vp, C.POINTER(i32)]
    L.plslam_grid_plan_destroy.argtypes = [vp]
    L.plslam_grid_pair_capacity.argtypes = [vp, i32, i32, vp, i32, i32, vp, C.c_int]
    L.plslam_grid_pair_capacity_bound.argtypes = [i32, i32, vp, i32, i32, vp, C.c_int]
    L.plslam_gather_match_tables.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, vp, C.c_int64, vp, vp]
    L.plslam_rccl_use.argtypes = [C.c_char_p]
    L.plslam_match_plan_step_gather.argtypes = [vp, C.POINTER(GatherStep)]
    L.plslam_match_plan_gather_sync.argtypes = [vp]
    L.plslam_rccl_available.argtypes = []
    L.plslam_bow_vocab_create.argtypes = [vp, C.POINTER(BowVocabDesc), C.POINTER(vp)]
    L.plslam_bow_vocab_destroy.argtypes = [vp]
    L.plslam_bow_transform.argtypes = [vp, vp, vp, i32, vp, vp, vp, vp, vp]
    L.plslam_bow_transform_dev.argtypes = [vp, vp, vp, i32, i32, i32, vp, vp, vp, vp, vp, vp]
    L.plslam_bow_db_create.argtypes = [vp, vp, vp, i32, C.POINTER(vp)]
    L.plslam_bow_db_destroy.argtypes = [vp]
    L.plslam_bow_db_insert.argtypes = [vp, i32, vp, i32, vp, i32, C.POINTER(BowPlStats), vp, vp]
    L.plslam_bow_db_insert_dev.argtypes = [vp, i32, vp, i32, vp, i32, C.POINTER(BowPlStats), vp, vp]
    L.plslam_bow_db_size.argtypes = [vp, C.POINTER(i32)]
    L.plslam_bow_db_score.argtypes = [vp, vp, i32, vp]
    L.plslam_loop_closure_verify.argtypes = [vp, C.POINTER(LcParams), C.POINTER(LcKeyframe), C.POINTER(LcKeyframe),
                                             C.POINTER(LcResult), vp, vp, vp, vp]
    L.plslam_loop_closure_verify_dev.argtypes = [vp, C.POINTER(LcParams), C.POINTER(LcKeyframe), C.POINTER(LcKeyframe), vp,
                                                 vp, vp, vp, vp, vp]
    L.plslam_relpose_robust_gn.argtypes = [vp, C.POINTER(LcParams), vp, vp, i32, vp, vp, i32, C.POINTER(LcResult), vp, vp]
    L.plslam_lc_batch_create.argtypes = [vp, C.POINTER(LcParams), i32, C.POINTER(vp)]
    L.plslam_lc_batch_destroy.argtypes = [vp]
    L.plslam_lc_batch_verify.argtypes = [vp, C.POINTER(LcKeyframe), C.POINTER(LcKeyframe), i32, C.POINTER(LcResult), vp, vp, vp, vp]
    L.plslam_lc_batch_verify_dev.argtypes = [vp, C.POINTER(LcKeyframe), C.POINTER(LcKeyframe), i32, vp, vp, vp, vp, vp, vp]
    L.plslam_relpose_robust_gn_batched_dev.argtypes = [vp, C.POINTER(LcParams), vp, vp, vp, vp, vp, vp, i32, vp, vp, vp, vp]
    L.plslam_gba_plan_create.argtypes = [vp, C.POINTER(Cam), f64, i32, i32, vp, i32, i32, vp, vp, i32, vp, vp, i32, C.POINTER(vp)]
    L.plslam_gba_optimize.argtypes = [vp, f64, f64, i32] + [vp] * 8 + [C.POINTER(GbaSolve), C.POINTER(GbaResult)]
    L.plslam_gba_plan_destroy.argtypes = [vp]
    L.plslam_gba_plan_create_dev.argtypes = [vp, C.POINTER(Cam), f64, i32, i32, vp, i32, i32, vp, vp, i32, vp, vp, i32, C.POINTER(vp)]
    L.plslam_gba_plan_list_sizes.argtypes = [vp, C.POINTER(GbaListSizes)]
    L.plslam_gba_plan_lists.argtypes = [vp, vp]
    L.plslam_gba_optimize_dev.argtypes = [vp, f64, f64, i32] + [vp] * 6 + [C.POINTER(GbaSolve), C.POINTER(GbaResult)]
    L.plslam_dense_ldlt_solve.argtypes = [vp, i32, vp, vp, vp, C.POINTER(i32)]
    L.plslam_pgo_plan_create.argtypes = [vp, C.POINTER(PgoParams), i32, vp, vp, i32, vp, C.POINTER(vp)]
    L.plslam_pgo_optimize.argtypes = [vp] + [vp] * 7 + [C.POINTER(PgoTrial), i32, C.POINTER(PgoResult)]
    L.plslam_pgo_plan_destroy.argtypes = [vp]
    L.plslam_lc_correct_map.argtypes = [vp, i32, vp, vp, C.POINTER(LcLandmarks), C.POINTER(LcLandmarks)]
    L.plslam_lc_correct_map_dev.argtypes = [vp, i32, vp, vp, C.POINTER(LcLandmarks), C.POINTER(LcLandmarks), vp]
    L.plslam_envelope_ldlt_solve.argtypes = [vp, i32, vp, vp, vp, C.POINTER(i32), C.POINTER(i32)]
    # the local map (plslam_amd/local_map.py holds the structs and the wrapper): every struct goes by address
    L.plslam_local_map_create.argtypes = [vp, C.POINTER(vp)]
    L.plslam_local_map_destroy.argtypes = [vp]
    L.plslam_local_map_form.argtypes = [vp, vp, i32, vp, i32, i32, vp]
    L.plslam_local_map_candidates.argtypes = [vp, vp, i32]
    L.plslam_local_map_gather.argtypes = [vp, vp, vp]
    L.plslam_local_map_cull.argtypes = [vp, vp, i32, i32, vp]
    L.plslam_local_map_device_buffers.argtypes = [vp, vp]
    L.plslam_local_map_download.argtypes = [vp, vp]
    L.plslam_local_map_apply_lba.argtypes = [vp, vp, vp, f64, vp]
    L.plslam_local_map_form_all.argtypes = [vp, vp, vp]
    L.plslam_local_map_apply_gba.argtypes = [vp, vp, vp]
    # the map insertion (plslam_amd/map_insert.py): structs by address, host arrays as pointers
    L.plslam_map_insert_create.argtypes = [vp, C.POINTER(vp)]
    L.plslam_map_insert_destroy.argtypes = [vp]
    L.plslam_map_insert_kf2kf.argtypes = [vp, vp, vp, i32, i32, vp, vp, vp, vp, vp, vp]
    L.plslam_map_insert_map2kf.argtypes = [vp, vp, vp, i32, vp, vp, vp, vp, vp]
    L.plslam_map_insert_device_buffers.argtypes = [vp, vp]
    L.plslam_map_insert_download.argtypes = [vp, vp]
    # the loop-closure fusion (plslam_amd/lc_fuse.py)
    L.plslam_lc_fuse_create.argtypes = [vp, C.POINTER(vp)]
    L.plslam_lc_fuse_destroy.argtypes = [vp]
    L.plslam_lc_fuse_run.argtypes = [vp, vp, vp, i32, vp, vp, vp, vp, vp, vp]
    L.plslam_lc_fuse_device_buffers.argtypes = [vp, vp]
    L.plslam_lc_fuse_download.argtypes = [vp, vp]
    # the side lists of the device-resident map (plslam_amd/map_lists.py)
    L.plslam_map_lists_refresh.argtypes = [vp, vp, vp]
    L.plslam_map_insert_carry.argtypes = [vp, vp, vp, vp, vp, vp, vp]
    L.plslam_lc_fuse_carry.argtypes = [vp, vp, vp, vp, vp, vp, vp]
    # the loop-closure correction on the map image (plslam_amd/pgo.py: correct_image)
    L.plslam_lc_correct_image.argtypes = [vp, vp, vp, vp, vp, C.POINTER(LcImageDst), C.POINTER(LcImageCounts)]
    for name in ABI_SYMBOLS:
        getattr(L, name).restype = _RESTYPES.get(name, C.c_int)
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
    buffer protocol: `a.ctypes.data_as(...)` builds a ctypes helper object per call -- 2 us each, 20 us of a matchGrid call's 58."""
    if a is None:
        return None
    try:
        return _addressof(_from_buffer(a))
    except (TypeError, ValueError, BufferError):          # a read-only or an empty array
        return a.ctypes.data


def grid_pair_capacity(centres, cell_start, cols, rows, window, mutual=True, bound=False) -> int:
    """plslam_grid_problem.pair_capacity (pure host code, no device needed): the documented size, or -- bound=True -- an upper
    bound of it from the grid alone (centres: only their shape is used then)."""
    L = load()
    cen = _arr(centres, np.int32)
    cen = cen.reshape(cen.shape[0], -1, 2) if cen.size else cen.reshape(0, 1, 2)
    cs = _arr(cell_start, np.int32)
    w = _arr(window, np.int32, (4,))
    if bound:
        return int(L.plslam_grid_pair_capacity_bound(cen.shape[0], cen.shape[1], _p(cs), int(cols), int(rows), _p(w),
                                                     int(bool(mutual))))
    return int(L.plslam_grid_pair_capacity(_p(cen), cen.shape[0], cen.shape[1], _p(cs), int(cols), int(rows), _p(w),
                                           int(bool(mutual))))


def make_cam(fx, fy, cx, cy, b=0.0, width=0, height=0) -> Cam:
    return Cam(float(fx), float(fy), float(cx), float(cy), float(b), int(width), int(height))


class Context:
    """plslam_ctx: one HIP device, one stream, scratch pools."""

    def __init__(self, device: int = 0):
        self._L = load()
        h = C.c_void_p()
        _check(self._L.plslam_ctx_create(int(device), C.byref(h)), "plslam_ctx_create")
        self._h = h
        self.device = int(device)

    def close(self):
        if getattr(self, "_h", None):
            self._L.plslam_ctx_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    @property
    def handle(self):
        return self._h

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
    @staticmethod
    def _lc_kf_arrays(kf):
        """the host arrays of one keyframe dict (pdesc, P, pl, pt_idx, ldesc, sPeP, le, ls_idx), contiguous and typed"""
        out = {"pdesc": _arr(kf["pdesc"], np.uint8, (-1, 32)), "P": _arr(kf["P"], np.float64, (-1, 3)),
               "pl": _arr(kf["pl"], np.float64, (-1, 2)), "ldesc": _arr(kf["ldesc"], np.uint8, (-1, 32)),
               "sPeP": _arr(kf["sPeP"], np.float64, (-1, 6)), "le": _arr(kf["le"], np.float64, (-1, 3))}
        for k in ("pt_idx", "ls_idx"):
            out[k] = None if kf.get(k) is None else _arr(kf[k], np.int32)
        n_pt, n_ls = out["pdesc"].shape[0], out["ldesc"].shape[0]
        for k, n in (("P", n_pt), ("pl", n_pt), ("pt_idx", n_pt), ("sPeP", n_ls), ("le", n_ls), ("ls_idx", n_ls)):
            if out[k] is not None and out[k].shape[0] != n:
                raise ValueError(f"keyframe array {k} has {out[k].shape[0]} rows, its descriptors {n}")
        return out

    @staticmethod
    def _lc_kf_record(a):
        # a: the arrays of _lc_kf_arrays (host) or of device tensors' addresses; the caller keeps them alive across the call
        return LcKeyframe(_p(a["pdesc"]), _p(a["P"]), _p(a["pl"]), _p(a["pt_idx"]), a["P"].shape[0], a["sPeP"].shape[0],
                          _p(a["ldesc"]), _p(a["sPeP"]), _p(a["le"]), _p(a["ls_idx"]))

    def loop_closure_verify(self, params, kf0, kf1):
        """isLoopClosure(kf0, kf1) -> (result dict, pt_corr[common_pt, 4], pt_inlier, ls_corr[common_ls, 4], ls_inlier).
        kf0 / kf1: dicts with pdesc, P, pl, pt_idx (or None), ldesc, sPeP, le, ls_idx (or None)."""
        a0, a1 = self._lc_kf_arrays(kf0), self._lc_kf_arrays(kf1)
        r0, r1 = self._lc_kf_record(a0), self._lc_kf_record(a1)
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
        F = FastMatching(int(fm["enabled"]), int(fm["grid_cols"]), int(fm["grid_rows"]), int(fm["ws"]),
                         float(fm["inv_width"]), float(fm["inv_height"]), float(fm["nnr_grid"]),
                         float(fm.get("line_sim_th", 0.75)))
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
        F = FastMatching(int(fm["enabled"]), int(fm["grid_cols"]), int(fm["grid_rows"]), int(fm["ws"]),
                         float(fm["inv_width"]), float(fm["inv_height"]), float(fm["nnr_grid"]),
                         float(fm.get("line_sim_th", 0.75)))
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
        F = FastMatching(int(fm["enabled"]), int(fm["grid_cols"]), int(fm["grid_rows"]), int(fm["ws"]),
                         float(fm["inv_width"]), float(fm["inv_height"]), float(fm["nnr_grid"]),
                         float(fm.get("line_sim_th", 0.75)))
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
        F = FastMatching(int(fm["enabled"]), int(fm["grid_cols"]), int(fm["grid_rows"]), int(fm["ws"]),
                         float(fm["inv_width"]), float(fm["inv_height"]), float(fm["nnr_grid"]),
                         float(fm.get("line_sim_th", 0.75)))
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
            raise PlslamError("plslam_pinned_alloc failed")
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


class MatchPipeline:
    """plslam_match_pipeline: a batch shape fixed at creation, `depth` batches in flight (upload / kernels / download on
    three streams).  problems: iterable of (d1_off, n1, d2_off, n2, nnr, mutual, out_off)."""

    def __init__(self, ctx: "Context", arena_bytes: int, problems, out_entries: int, depth: int = 3):
        self._L = ctx._L
        problems = list(problems)
        arr = (ArenaProblem * max(len(problems), 1))()
        for i, (o1, n1, o2, n2, nnr, mutual, oo) in enumerate(problems):
            arr[i] = ArenaProblem(int(o1), int(o2), int(n1), int(n2), float(nnr), int(bool(mutual)), int(oo))
        h = C.c_void_p()
        _check(self._L.plslam_match_pipeline_create(ctx.handle, int(arena_bytes), arr, len(problems), int(out_entries),
                                                    int(depth), C.byref(h)), "plslam_match_pipeline_create")
        self._h, self.nprob, self.arena_bytes, self.out_entries = h, len(problems), int(arena_bytes), int(out_entries)

    def submit(self, arena: np.ndarray, out: np.ndarray, counts: np.ndarray | None = None):
        assert arena.nbytes >= self.arena_bytes and out.dtype == np.int32 and out.size >= self.out_entries
        assert arena.flags.c_contiguous and out.flags.c_contiguous
        _check(self._L.plslam_match_pipeline_submit(self._h, arena.ctypes.data, out.ctypes.data,
                                                    counts.ctypes.data if counts is not None else None),
               "plslam_match_pipeline_submit")

    def wait(self):
        _check(self._L.plslam_match_pipeline_wait(self._h), "plslam_match_pipeline_wait")

    def close(self):
        if getattr(self, "_h", None):
            self._L.plslam_match_pipeline_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class LbaPlan:
    """plslam_lba_plan: observation lists uploaded once, iterate(T_kf_w, Xw, Lw) per LM iteration."""

    def __init__(self, ctx: Context, cam: Cam, homog_th, n_pose_slots, nkf, npt, nls, pt_lm, pt_slot, pt_kf_loc,
                 pt_obs_uv, ls_lm, ls_slot, ls_kf_loc, ls_l_obs):
        self._L = ctx._L
        self._ctx = ctx
        a = [_arr(x, np.int32) for x in (pt_lm, pt_slot, pt_kf_loc)]
        b = [_arr(x, np.int32) for x in (ls_lm, ls_slot, ls_kf_loc)]
        uv, lo = _arr(pt_obs_uv, np.float64, (-1, 2)), _arr(ls_l_obs, np.float64, (-1, 3))
        self.dims = (int(nkf), int(npt), int(nls), uv.shape[0], lo.shape[0], int(n_pose_slots))
        h = C.c_void_p()
        _check(self._L.plslam_lba_plan_create(ctx.handle, C.byref(cam), float(homog_th), int(n_pose_slots), int(nkf),
                                              int(npt), int(nls), _p(a[0]), _p(a[1]), _p(a[2]), _p(uv), uv.shape[0],
                                              _p(b[0]), _p(b[1]), _p(b[2]), _p(lo), lo.shape[0], C.byref(h)),
               "plslam_lba_plan_create")
        self._h = h

    COMPAT_ITER_PASS, COMPAT_GBA = 1, 2
    DIST_TILE = 1024        # plslam_amd/csrc/distribute_dev.hpp: the items one workgroup of the device-side list builder takes

    @classmethod
    def from_device(cls, ctx: Context, cam: Cam, homog_th, n_pose_slots, nkf, npt, nls, pt_lm, pt_slot, pt_kf_loc, pt_obs_uv,
                    n_pt_obs, ls_lm, ls_slot, ls_kf_loc, ls_l_obs, n_ls_obs, d_Xw=0, d_Lw=0, first_estimate_slot=-1):
        """plslam_lba_plan_create_dev: the eight observation columns and d_Xw / d_Lw are DEVICE pointers (ints, 0 = NULL), e.g.
        the entries of LocalMap.device_buffers(); the lists are built on the device.  first_estimate_slot >= 0 rewrites the slot
        of every point observation of an optimised keyframe to first_estimate_slot + kf_loc."""
        self = cls.__new__(cls)
        self._L, self._ctx = ctx._L, ctx
        self.dims = (int(nkf), int(npt), int(nls), int(n_pt_obs), int(n_ls_obs), int(n_pose_slots))
        h = C.c_void_p()
        q = lambda a: C.c_void_p(int(a)) if a else None                          # noqa: E731
        _check(self._L.plslam_lba_plan_create_dev(ctx.handle, C.byref(cam), float(homog_th), int(n_pose_slots), int(nkf), int(npt),
                                                  int(nls), q(pt_lm), q(pt_slot), q(pt_kf_loc), q(pt_obs_uv), int(n_pt_obs),
                                                  q(ls_lm), q(ls_slot), q(ls_kf_loc), q(ls_l_obs), int(n_ls_obs), q(d_Xw), q(d_Lw),
                                                  int(first_estimate_slot), C.byref(h)), "plslam_lba_plan_create_dev")
        self._h = h
        return self

    def lists(self, prepare_schur=False) -> dict:
        """The plan's lists as host arrays (plslam_lba_plan_lists): pt_ptr / pt_ids, ls_ptr / ls_ids, kf_ptr / kf_ids, the
        observation columns as the plan stores them, max_chunks; once the Schur lists exist (prepare_schur=True builds them):
        blk_ptr, pairs (n, 4) and schur_chunks."""
        class _Sizes(C.Structure):
            _fields_ = [(k, C.c_int32) for k in ("nkf", "npt", "nls", "n_pt_obs", "n_ls_obs", "n_kf_ids", "max_chunks", "schur_ready",
                                                 "nblk", "n_pairs", "schur_chunks")]
        names = ("pt_ptr", "pt_ids", "ls_ptr", "ls_ids", "kf_ptr", "kf_ids", "pt_lm_loc", "pt_pose_slot", "pt_kf_loc", "pt_obs_uv",
                 "ls_lm_loc", "ls_pose_slot", "ls_kf_loc", "ls_l_obs", "blk_ptr", "pairs")

        class _Lists(C.Structure):
            _fields_ = [(k, C.c_void_p) for k in names]
        z = _Sizes()
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
        class _S(C.Structure):
            _fields_ = [("T_kf_w", C.c_void_p), ("Xw", C.c_void_p), ("Lw", C.c_void_p), ("g", C.c_void_p),
                        ("n_pose_slots", C.c_int32), ("npt", C.c_int32), ("nls", C.c_int32), ("n", C.c_int64)]
        st = _S()
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
        class _S(C.Structure):
            _fields_ = [("T_kf_w", C.c_void_p), ("Xw", C.c_void_p), ("Lw", C.c_void_p), ("n_pose_slots", C.c_int32),
                        ("npt", C.c_int32), ("nls", C.c_int32), ("stream", C.c_void_p)]
        st = _S()
        _check(self._L.plslam_lba_plan_device_state(self._h, C.byref(st)), "plslam_lba_plan_device_state")
        return {k: getattr(st, k) for k, _ in _S._fields_}

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

    def close(self):
        if getattr(self, "_h", None):
            self._L.plslam_lba_plan_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class MatchPlan:
    """plslam_match_plan over device pointers (ints, e.g. torch.Tensor.data_ptr()).

    problems: iterable of (d1_ptr, n1, d2_ptr, n2, nnr, mutual, matches12_ptr, n_matches_ptr|0)
    """

    def __init__(self, ctx: Context, problems):
        self._ctx = ctx
        self._L = ctx._L
        problems = list(problems)
        arr = (MatchProblem * max(len(problems), 1))()
        for i, (d1, n1, d2, n2, nnr, mutual, m12, nm) in enumerate(problems):
            arr[i] = MatchProblem(d1 or None, d2 or None, int(n1), int(n2), float(nnr), int(bool(mutual)),
                                  m12 or None, nm or None)
        h = C.c_void_p()
        _check(self._L.plslam_match_plan_create(ctx.handle, arr, len(problems), C.byref(h)),
               "plslam_match_plan_create")
        self._h = h

    def run(self, stream: int = 0) -> None:
        _check(self._L.plslam_match_plan_run(self._h, stream or None), "plslam_match_plan_run")

    def run_split(self, scan_stream: int, post_stream: int) -> None:
        """The scan on one HIP stream, the stages behind it on another (they overlap the next run's scan)."""
        _check(self._L.plslam_match_plan_run_split(self._h, scan_stream or None, post_stream or None),
               "plslam_match_plan_run_split")

    def make_gather_step(self, comm: int, nranks: int, rank: int, root: int, wire_bytes: int, send: int, n_entries: int, recv: int,
                         wide: int, scan_stream: int, post_stream: int, comm_stream: int = 0):
        """The argument block of step_gather(), built ONCE per (plan, buffer): the step itself is then one foreign call."""
        return GatherStep(comm or None, int(nranks), int(rank), int(root), int(wire_bytes), send or None, int(n_entries), recv or None,
                          wide or None, scan_stream or None, post_stream or None, comm_stream or None)

    def step_gather(self, step) -> None:
        """plslam_match_plan_step_gather: plan run + gather of the finished table to the root (+ widening), all enqueued."""
        rc = self._L.plslam_match_plan_step_gather(self._h, C.byref(step))
        if rc:
            _check(rc, "plslam_match_plan_step_gather")

    def gather_sync(self) -> None:
        _check(self._L.plslam_match_plan_gather_sync(self._h), "plslam_match_plan_gather_sync")

    def add_stereo_gates(self, gates) -> None:
        """The gate stage (StereoFrame::matchStereoPoints / matchStereoLines over the batch).  gates: iterable of dicts
        with the fields of plslam_stereo_gate_problem (device pointers as ints)."""
        gates = list(gates)
        arr = (StereoGateProblem * max(len(gates), 1))()
        for i, g in enumerate(gates):
            arr[i] = StereoGateProblem(g["matches_12"] or None, g["f_l"] or None, g["f_r"] or None, int(g["n_l"]),
                                       int(g["n_r"]), int(bool(g["lines"])), 0, float(g.get("max_dist_epip", 0.0)),
                                       float(g.get("min_disp", 0.0)), float(g.get("line_horiz_th", 0.0)),
                                       float(g.get("stereo_overlap_th", 0.0)), float(g.get("ls_min_disp_ratio", 0.0)),
                                       g["stereo_12"] or None, g["disp"] or None, g.get("n_stereo") or None)
        _check(self._L.plslam_match_plan_add_stereo_gates(self._h, arr, len(gates)), "plslam_match_plan_add_stereo_gates")

    def set_wire16(self, table32: int, table16: int, n_entries: int) -> None:
        """An int16 mirror of the plan's match tables inside [table32, table32 + n_entries) (device pointers as ints), written by
        the finalize kernel beside the int32 entries: the wire format of the N > 1 gather.  table16 = 0 removes it."""
        _check(self._L.plslam_match_plan_set_wire16(self._h, table32 or None, table16 or None, int(n_entries)),
               "plslam_match_plan_set_wire16")

    def set_profiling(self, on: bool) -> None:
        _check(self._L.plslam_match_plan_set_profiling(self._h, int(bool(on))),
               "plslam_match_plan_set_profiling")

    def elapsed(self):
        a, b, n = C.c_double(), C.c_double(), C.c_int64()
        _check(self._L.plslam_match_plan_elapsed(self._h, C.byref(a), C.byref(b), C.byref(n)),
               "plslam_match_plan_elapsed")
        return a.value, b.value, n.value

    def info(self) -> dict:
        i = PlanInfo()
        _check(self._L.plslam_match_plan_info(self._h, C.byref(i)), "plslam_match_plan_info")
        return {k: getattr(i, k) for k, _ in PlanInfo._fields_}

    def key_state(self) -> int:
        """What dump()'s key table holds: a mask of KEYS_ROW_SECOND_INDEX_INEXACT (1), KEYS_COLUMN_SECOND_LAZY (2),
        KEYS_COLUMNS_NOT_IN_MEMORY (4); 0 = every word an exact key."""
        f = C.c_int32()
        _check(self._L.plslam_match_plan_key_state(self._h, C.byref(f)), "plslam_match_plan_key_state")
        return f.value

    def dump(self):
        """Diagnostics: (keys, column_partials) as uint32 arrays, after a device synchronise."""
        kb, pb = C.c_size_t(), C.c_size_t()
        _check(self._L.plslam_match_plan_dump(self._h, None, 0, None, 0, C.byref(kb), C.byref(pb)),
               "plslam_match_plan_dump")
        k = np.empty(kb.value // 4, np.uint32)
        p = np.empty(pb.value // 4, np.uint32)
        _check(self._L.plslam_match_plan_dump(self._h, k.ctypes.data, k.nbytes, p.ctypes.data, p.nbytes,
                                              C.byref(kb), C.byref(pb)), "plslam_match_plan_dump")
        return k, p

    def close(self):
        if getattr(self, "_h", None):
            self._L.plslam_match_plan_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class GridPlan:
    """plslam_grid_plan over device pointers: a batch of StVO::matchGrid problems, one kernel launch.

    problems: iterable of dicts with the fields of plslam_grid_problem (pointers as ints; window a 4-sequence).
    """

    def __init__(self, ctx: Context, problems):
        self._ctx = ctx
        self._L = ctx._L
        problems = list(problems)
        arr = (GridProblem * max(len(problems), 1))()
        for i, q in enumerate(problems):
            g = GridProblem()
            for k in ("d1", "d2", "centres1", "cell_start", "cell_items", "dir1", "dir2", "matches_12", "n_matches"):
                setattr(g, k, q.get(k) or None)
            for k in ("n1", "n2", "n_centres", "grid_cols", "grid_rows", "n_items", "pair_capacity"):
                setattr(g, k, int(q[k]))
            g.window = (C.c_int32 * 4)(*[int(v) for v in q["window"]])
            g.sim_th, g.nnr, g.mutual = float(q.get("sim_th", 0.0)), float(q["nnr"]), int(bool(q.get("mutual", True)))
            arr[i] = g
        h = C.c_void_p()
        _check(self._L.plslam_grid_plan_create(ctx.handle, arr, len(problems), C.byref(h)), "plslam_grid_plan_create")
        self._h = h

    def run(self, stream: int = 0) -> None:
        _check(self._L.plslam_grid_plan_run(self._h, stream or None), "plslam_grid_plan_run")

    def overflows(self, stream: int = 0) -> int:
        n = C.c_int32()
        _check(self._L.plslam_grid_plan_overflows(self._h, stream or None, C.byref(n)), "plslam_grid_plan_overflows")
        return n.value

    def close(self):
        if getattr(self, "_h", None):
            self._L.plslam_grid_plan_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _bow_stats(stats):
    if stats is None:
        return None
    if isinstance(stats, BowPlStats):
        return stats
    n_pt, n_ls, std_pt, std_ls = stats
    return BowPlStats(int(n_pt), int(n_ls), float(std_pt), float(std_ls))


class BowVocabulary:
    """plslam_bow_vocab: a DBoW2 vocabulary on the device (TemplatedVocabulary::load, TemplatedVocabulary.h:1437-1485).

    voc: anything with the fields k, L, scoring_type, weighting_type, nodes (BOW_NODE_DTYPE records in file order) and words
    (BOW_WORD_DTYPE records) -- plslam_amd.bow.Vocabulary."""

    def __init__(self, ctx: Context, voc):
        self._ctx = ctx
        self._L = ctx._L
        nodes = np.ascontiguousarray(voc.nodes, dtype=BOW_NODE_DTYPE)
        words = np.ascontiguousarray(voc.words, dtype=BOW_WORD_DTYPE)
        desc = BowVocabDesc(int(voc.k), int(voc.L), int(voc.scoring_type), int(voc.weighting_type), nodes.shape[0],
                            words.shape[0], _p(nodes), _p(words))
        h = C.c_void_p()
        _check(self._L.plslam_bow_vocab_create(ctx.handle, C.byref(desc), C.byref(h)), "plslam_bow_vocab_create")
        self._h = h

    @property
    def handle(self):
        return self._h

    def transform(self, desc, offsets):
        """TemplatedVocabulary::transform over ragged sets -> (word_id[total], word_weight[total], bow_word[total],
        bow_weight[total], bow_len[nsets]); set s's BowVector is bow_word / bow_weight[offsets[s] : offsets[s] + bow_len[s]]."""
        d = _arr(desc, np.uint8, (-1, 32))
        off = _arr(offsets, np.int32)
        nsets = off.shape[0] - 1
        total = d.shape[0]
        word, weight = np.empty(total, np.int32), np.empty(total, np.float64)
        bword, bweight = np.empty(total, np.int32), np.empty(total, np.float64)
        blen = np.empty(max(nsets, 0), np.int32)
        _check(self._L.plslam_bow_transform(self._h, _p(d), _p(off), nsets, _p(word), _p(weight), _p(bword), _p(bweight),
                                            _p(blen)), "plslam_bow_transform")
        return word, weight, bword, bweight, blen

    def transform_dev(self, d_desc, d_offsets, nsets, total, max_set, d_word, d_weight, d_bow_word, d_bow_weight, d_bow_len,
                      stream=None):
        """Device-pointer form (addresses as ints); enqueues on `stream` (None = the context's stream), no sync."""
        _check(self._L.plslam_bow_transform_dev(self._h, int(d_desc), int(d_offsets), int(nsets), int(total), int(max_set),
                                                int(d_word), d_weight or None, int(d_bow_word), int(d_bow_weight),
                                                int(d_bow_len), stream or None), "plslam_bow_transform_dev")

    def close(self):
        if getattr(self, "_h", None):
            self._L.plslam_bow_vocab_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class BowDatabase:
    """plslam_bow_db: the keyframes' BowVectors on the device and MapHandler::insertKFBowVector{P,L,PL}
    (src/mapHandler.cpp:3007-3128).  vocab_p / vocab_l: BowVocabulary or None (the mode follows :196-201).  Close it before
    its vocabularies."""

    def __init__(self, ctx: Context, vocab_p, vocab_l, capacity_hint: int = 0):
        self._ctx = ctx
        self._L = ctx._L
        self._voc = (vocab_p, vocab_l)          # kept alive as long as the database
        h = C.c_void_p()
        _check(self._L.plslam_bow_db_create(ctx.handle, vocab_p.handle if vocab_p else None,
                                            vocab_l.handle if vocab_l else None, int(capacity_hint), C.byref(h)),
               "plslam_bow_db_create")
        self._h = h

    @property
    def size(self) -> int:
        n = C.c_int32()
        _check(self._L.plslam_bow_db_size(self._h, C.byref(n)), "plslam_bow_db_size")
        return n.value

    def insert(self, kf_idx, pdesc=None, ldesc=None, stats=None, alive=None, conf_row=None):
        """One keyframe: conf_row (float64, >= kf_idx + 1 entries, updated in place; None = a fresh NaN row) gets
        score(new, i) for every alive i < kf_idx and the self score at kf_idx.  stats: (n_pt, n_ls, std_pt, std_ls), PL mode.
        alive: kf_idx uint8 flags (None = all alive)."""
        kf_idx = int(kf_idx)
        pd = _arr(pdesc if pdesc is not None else np.zeros((0, 32), np.uint8), np.uint8, (-1, 32))
        ld = _arr(ldesc if ldesc is not None else np.zeros((0, 32), np.uint8), np.uint8, (-1, 32))
        al = _arr(np.ones(kf_idx, np.uint8) if alive is None else alive, np.uint8)
        assert al.shape[0] >= kf_idx
        row = np.full(kf_idx + 1, np.nan) if conf_row is None else conf_row
        assert row.dtype == np.float64 and row.flags.c_contiguous and row.shape[0] >= kf_idx + 1
        st = _bow_stats(stats)
        _check(self._L.plslam_bow_db_insert(self._h, kf_idx, _p(pd), pd.shape[0], _p(ld), ld.shape[0],
                                            C.byref(st) if st is not None else None, _p(al), _p(row)), "plslam_bow_db_insert")
        return row

    def insert_dev(self, kf_idx, d_pdesc, n_pdesc, d_ldesc, n_ldesc, stats, d_alive, d_conf_row):
        """Device-pointer form (addresses as ints), enqueued on the context's stream, no sync."""
        st = _bow_stats(stats)
        _check(self._L.plslam_bow_db_insert_dev(self._h, int(kf_idx), d_pdesc or None, int(n_pdesc), d_ldesc or None,
                                                int(n_ldesc), C.byref(st) if st is not None else None, d_alive or None,
                                                int(d_conf_row)), "plslam_bow_db_insert_dev")

    def score(self, queries):
        """plslam_bow_db_score -> (nq, size) float64; NaN where a keyframe was never inserted."""
        q = _arr(queries, np.int32)
        out = np.empty((q.shape[0], self.size), np.float64)
        _check(self._L.plslam_bow_db_score(self._h, _p(q), q.shape[0], _p(out)), "plslam_bow_db_score")
        return out

    def close(self):
        if getattr(self, "_h", None):
            self._L.plslam_bow_db_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _hip_memcpy_dtod(dst: int, src: int, nbytes: int) -> int:
    """Device-to-device copy through the HIP runtime (tests: an in-place update of a plan's device state)."""
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    hip.hipMemcpy.restype = C.c_int
    return hip.hipMemcpy(C.c_void_p(dst), C.c_void_p(src), C.c_size_t(nbytes), 3)      # hipMemcpyDeviceToDevice


class GbaPlan:
    """plslam_gba_plan: the global bundle adjustment of the reference (levMarquardtOptimizationGBA) over one map.

    pt_obs / ls_obs: the reference's Vector6i rows (n, 6) -- landmark map index, landmark local index, observation index,
    keyframe map index, keyframe local index (-1: keyframe 0), inlier flag; pt_uv (n, 2) / ls_l (n, 3) the observations;
    kf_list[k]: the map index of optimised keyframe k."""

    def __init__(self, ctx: Context, cam: Cam, n_map_kf, kf_list, npt, nls, pt_obs, pt_uv, ls_obs, ls_l, homog_th=1e-7):
        self._L = ctx._L
        self._ctx = ctx
        kl = _arr(kf_list, np.int32, (-1,))
        po, lo = _arr(pt_obs, np.int32, (-1, 6)), _arr(ls_obs, np.int32, (-1, 6))
        uv, ll = _arr(pt_uv, np.float64, (-1, 2)), _arr(ls_l, np.float64, (-1, 3))
        self.dims = (int(n_map_kf), kl.shape[0], int(npt), int(nls))
        self._h = None
        h = C.c_void_p()
        _check(self._L.plslam_gba_plan_create(ctx.handle, C.byref(cam), float(homog_th), int(n_map_kf), kl.shape[0], _p(kl),
                                              int(npt), int(nls), _p(po), _p(uv), po.shape[0], _p(lo), _p(ll), lo.shape[0],
                                              C.byref(h)), "plslam_gba_plan_create")
        self._h = h

    @classmethod
    def from_device(cls, ctx: Context, cam: Cam, n_map_kf, nkf, d_kf_list, npt, nls, d_pt_obs, d_pt_uv, n_pt_obs, d_ls_obs, d_ls_l,
                    n_ls_obs, homog_th=1e-7):
        """plslam_gba_plan_create_dev: the same plan from DEVICE columns (addresses as ints), e.g. what LocalMap.form_all +
        .gather leave in LocalMap.device_buffers(): kf_list, pt_obs, pt_obs_uv, ls_obs, ls_l_obs."""
        self = cls.__new__(cls)
        self._L, self._ctx, self._h = ctx._L, ctx, None
        self.dims = (int(n_map_kf), int(nkf), int(npt), int(nls))
        h = C.c_void_p()
        _check(self._L.plslam_gba_plan_create_dev(ctx.handle, C.byref(cam), float(homog_th), int(n_map_kf), int(nkf),
                                                  d_kf_list or None, int(npt), int(nls), d_pt_obs or None, d_pt_uv or None,
                                                  int(n_pt_obs), d_ls_obs or None, d_ls_l or None, int(n_ls_obs), C.byref(h)),
               "plslam_gba_plan_create_dev")
        self._h = h
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

    def close(self) -> None:
        # a plan is destroyed before its context: once the context is closed the handle is only dropped
        if self._h is not None and self._h.value and self._ctx.handle:
            self._L.plslam_gba_plan_destroy(self._h)
        self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


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


class LcBatch:
    """plslam_lc_batch: isLoopClosure for up to max_pairs candidate pairs per call (K54), with `params` fixed."""

    def __init__(self, ctx: Context, params: LcParams, max_pairs: int):
        self._L = ctx._L
        self._ctx = ctx
        self.params = params
        self.max_pairs = int(max_pairs)
        self._h = None
        h = C.c_void_p()
        _check(self._L.plslam_lc_batch_create(ctx.handle, C.byref(params), self.max_pairs, C.byref(h)), "plslam_lc_batch_create")
        self._h = h

    def verify(self, pairs):
        """pairs: a sequence of (kf0, kf1) keyframe dicts (Context.loop_closure_verify's).  A dict that appears several
        times is packed and uploaded once.  -> one (result dict, pt_corr, pt_inlier, ls_corr, ls_inlier) per pair."""
        B = len(pairs)
        packed = {}

        def rec(kf):
            if id(kf) not in packed:
                a = Context._lc_kf_arrays(kf)
                packed[id(kf)] = (Context._lc_kf_record(a), a)
            return packed[id(kf)][0]

        r0 = (LcKeyframe * max(B, 1))(*(rec(p[0]) for p in pairs))
        r1 = (LcKeyframe * max(B, 1))(*(rec(p[1]) for p in pairs))
        rp = np.concatenate([[0], np.cumsum([r0[b].n_pt for b in range(B)])]).astype(np.int64)
        rl = np.concatenate([[0], np.cumsum([r0[b].n_ls for b in range(B)])]).astype(np.int64)
        pc, pi = np.zeros((int(rp[-1]), 4), np.int32), np.zeros(int(rp[-1]), np.uint8)
        lc, li = np.zeros((int(rl[-1]), 4), np.int32), np.zeros(int(rl[-1]), np.uint8)
        res = (LcResult * max(B, 1))()
        _check(self._L.plslam_lc_batch_verify(self._h, r0, r1, B, res, _p(pc), _p(pi), _p(lc), _p(li)), "plslam_lc_batch_verify")
        out = []
        for b in range(B):
            d = res[b].as_dict()
            n, m = d["common_pt"], d["common_ls"]
            out.append((d, pc[rp[b]:rp[b] + n], pi[rp[b]:rp[b] + n].astype(bool), lc[rl[b]:rl[b] + m],
                        li[rl[b]:rl[b] + m].astype(bool)))
        return out

    def verify_dev(self, kf0_dev, kf1_dev, results_ptr, pt_corr_ptr, pt_inlier_ptr, ls_corr_ptr, ls_inlier_ptr, stream=None):
        """Device-pointer form.  kf0_dev / kf1_dev: B dicts of device addresses each (Context.loop_closure_verify_dev's);
        results_ptr: B x sizeof(LcResult) bytes; pair b's rows start at row sum(n_pt of kf0_dev[:b]) (n_ls for lines).
        Enqueued behind `stream` (None = the context's stream), no synchronisation."""
        B = len(kf0_dev)
        if len(kf1_dev) != B:
            raise ValueError("kf0_dev and kf1_dev differ in length")

        def recs(ks):
            return (LcKeyframe * max(B, 1))(*(
                LcKeyframe(*(C.c_void_p(k.get(n) or 0) for n in ("pdesc", "P", "pl", "pt_idx")), int(k["n_pt"]), int(k["n_ls"]),
                           *(C.c_void_p(k.get(n) or 0) for n in ("ldesc", "sPeP", "le", "ls_idx"))) for k in ks))

        _check(self._L.plslam_lc_batch_verify_dev(self._h, recs(kf0_dev), recs(kf1_dev), B, C.c_void_p(results_ptr or 0),
                                                  C.c_void_p(pt_corr_ptr or 0), C.c_void_p(pt_inlier_ptr or 0),
                                                  C.c_void_p(ls_corr_ptr or 0), C.c_void_p(ls_inlier_ptr or 0),
                                                  C.c_void_p(stream or 0)), "plslam_lc_batch_verify_dev")

    def close(self) -> None:
        if self._h is not None and self._h.value and self._ctx.handle:
            self._L.plslam_lc_batch_destroy(self._h)
        self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class PgoPlan:
    """plslam_pgo_plan: the loop-closure pose graph of the reference (loopClosureOptimizationCovGraphG2O) over one map.

    kf_valid (n,): 0 for a NULL keyframe slot; full_graph (n, n) int32; lc_idx (n_lc, 3)."""

    def __init__(self, ctx: Context, kf_valid, full_graph, lc_idx, min_lm_ess_graph=75, min_lm_cov_graph=75, max_iters_pgo=100,
                 lambda_init=1e-10, max_trials=10):
        self._L = ctx._L
        self._ctx = ctx
        v = _arr(kf_valid, np.uint8, (-1,))
        n = v.shape[0]
        fg = _arr(full_graph, np.int32, (n, n))
        lc = _arr(lc_idx, np.int32, (-1, 3))
        self.n_map, self.n_lc = n, lc.shape[0]
        self.params = PgoParams(int(min_lm_ess_graph), int(min_lm_cov_graph), int(max_iters_pgo), int(max_trials),
                                float(lambda_init))
        self._h = None
        h = C.c_void_p()
        _check(self._L.plslam_pgo_plan_create(ctx.handle, C.byref(self.params), n, _p(v), _p(fg), self.n_lc, _p(lc), C.byref(h)),
               "plslam_pgo_plan_create")
        self._h = h

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

    def close(self) -> None:
        if self._h is not None and self._h.value and self._ctx.handle:
            self._L.plslam_pgo_plan_destroy(self._h)
        self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


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
