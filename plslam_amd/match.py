"""The matchers over device pointers (include/plslam_hip.h): plslam_match_plan (a batch of StVO::match problems, the stereo
gates behind it, the gather of the finished tables), plslam_grid_plan (a batch of StVO::matchGrid problems) and
plslam_match_pipeline (host to host, batches in flight)."""
from __future__ import annotations

import ctypes as C

import numpy as np

from ._lib import Handle, _arr, _check, _p, load, proto

MAX_TRAIN_ROWS = 1 << 23


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


class PlanInfo(C.Structure):
    """plslam_plan_info"""
    _fields_ = [("distance_evals", C.c_int64), ("directed_evals", C.c_int64),
                ("algorithmic_bytes", C.c_int64), ("n_scans", C.c_int32),
                ("scan_blocks", C.c_int32), ("scan_variant", C.c_int32),
                ("scan_block_threads", C.c_int32)]


_vp, _i32, _f64 = C.c_void_p, C.c_int32, C.c_double
proto("plslam_grid_pair_capacity", [_vp, _i32, _i32, _vp, _i32, _i32, _vp, C.c_int], C.c_int64)
proto("plslam_grid_pair_capacity_bound", [_i32, _i32, _vp, _i32, _i32, _vp, C.c_int], C.c_int64)


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


proto("plslam_match_pipeline_create", [_vp, C.c_size_t, C.POINTER(ArenaProblem), _i32, C.c_size_t, _i32, C.POINTER(_vp)])
proto("plslam_match_pipeline_submit", [_vp, _vp, _vp, _vp])
proto("plslam_match_pipeline_wait", [_vp])
proto("plslam_match_pipeline_destroy", [_vp], None)


class MatchPipeline(Handle):
    """plslam_match_pipeline: a batch shape fixed at creation, `depth` batches in flight (upload / kernels / download on
    three streams).  problems: iterable of (d1_off, n1, d2_off, n2, nnr, mutual, out_off)."""

    def __init__(self, ctx: "Context", arena_bytes: int, problems, out_entries: int, depth: int = 3):
        problems = list(problems)
        arr = (ArenaProblem * max(len(problems), 1))()
        for i, (o1, n1, o2, n2, nnr, mutual, oo) in enumerate(problems):
            arr[i] = ArenaProblem(int(o1), int(o2), int(n1), int(n2), float(nnr), int(bool(mutual)), int(oo))
        h = C.c_void_p()
        _check(ctx._L.plslam_match_pipeline_create(ctx.handle, int(arena_bytes), arr, len(problems), int(out_entries),
                                                   int(depth), C.byref(h)), "plslam_match_pipeline_create")
        self._open(ctx, "plslam_match_pipeline_destroy", h)
        self.nprob, self.arena_bytes, self.out_entries = len(problems), int(arena_bytes), int(out_entries)

    def submit(self, arena: np.ndarray, out: np.ndarray, counts: np.ndarray | None = None):
        assert arena.nbytes >= self.arena_bytes and out.dtype == np.int32 and out.size >= self.out_entries
        assert arena.flags.c_contiguous and out.flags.c_contiguous
        _check(self._L.plslam_match_pipeline_submit(self._h, arena.ctypes.data, out.ctypes.data,
                                                    counts.ctypes.data if counts is not None else None),
               "plslam_match_pipeline_submit")

    def wait(self):
        _check(self._L.plslam_match_pipeline_wait(self._h), "plslam_match_pipeline_wait")


proto("plslam_match_plan_create", [_vp, C.POINTER(MatchProblem), _i32, C.POINTER(_vp)])
proto("plslam_match_plan_run", [_vp, _vp])
proto("plslam_match_plan_run_split", [_vp, _vp, _vp])
proto("plslam_match_plan_step_gather", [_vp, C.POINTER(GatherStep)])
proto("plslam_match_plan_gather_sync", [_vp])
proto("plslam_match_plan_add_stereo_gates", [_vp, C.POINTER(StereoGateProblem), _i32])
proto("plslam_match_plan_set_wire16", [_vp, _vp, _vp, C.c_size_t])
proto("plslam_match_plan_set_profiling", [_vp, C.c_int])
proto("plslam_match_plan_elapsed", [_vp, C.POINTER(_f64), C.POINTER(_f64), C.POINTER(C.c_int64)])
proto("plslam_match_plan_info", [_vp, C.POINTER(PlanInfo)])
proto("plslam_match_plan_key_state", [_vp, C.POINTER(C.c_int32)])
proto("plslam_match_plan_dump", [_vp, _vp, C.c_size_t, _vp, C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)])
proto("plslam_match_plan_destroy", [_vp], None)
# the gather of the match tables over ranks (plslam_amd/frontend.py calls these through load())
proto("plslam_gather_match_tables", [_vp, _vp, C.c_int, C.c_int, C.c_int, _vp, C.c_int64, _vp, _vp])
proto("plslam_rccl_use", [C.c_char_p])
proto("plslam_rccl_available", [])


class MatchPlan(Handle):
    """plslam_match_plan over device pointers (ints, e.g. torch.Tensor.data_ptr()).

    problems: iterable of (d1_ptr, n1, d2_ptr, n2, nnr, mutual, matches12_ptr, n_matches_ptr|0)
    """

    def __init__(self, ctx: Context, problems):
        problems = list(problems)
        arr = (MatchProblem * max(len(problems), 1))()
        for i, (d1, n1, d2, n2, nnr, mutual, m12, nm) in enumerate(problems):
            arr[i] = MatchProblem(d1 or None, d2 or None, int(n1), int(n2), float(nnr), int(bool(mutual)),
                                  m12 or None, nm or None)
        h = C.c_void_p()
        _check(ctx._L.plslam_match_plan_create(ctx.handle, arr, len(problems), C.byref(h)),
               "plslam_match_plan_create")
        self._open(ctx, "plslam_match_plan_destroy", h)

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


proto("plslam_grid_plan_create", [_vp, C.POINTER(GridProblem), _i32, C.POINTER(_vp)])
proto("plslam_grid_plan_run", [_vp, _vp])
proto("plslam_grid_plan_overflows", [_vp, _vp, C.POINTER(_i32)])
proto("plslam_grid_plan_destroy", [_vp], None)


class GridPlan(Handle):
    """plslam_grid_plan over device pointers: a batch of StVO::matchGrid problems, one kernel launch.

    problems: iterable of dicts with the fields of plslam_grid_problem (pointers as ints; window a 4-sequence).
    """

    def __init__(self, ctx: Context, problems):
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
        _check(ctx._L.plslam_grid_plan_create(ctx.handle, arr, len(problems), C.byref(h)), "plslam_grid_plan_create")
        self._open(ctx, "plslam_grid_plan_destroy", h)

    def run(self, stream: int = 0) -> None:
        _check(self._L.plslam_grid_plan_run(self._h, stream or None), "plslam_grid_plan_run")

    def overflows(self, stream: int = 0) -> int:
        n = C.c_int32()
        _check(self._L.plslam_grid_plan_overflows(self._h, stream or None, C.byref(n)), "plslam_grid_plan_overflows")
        return n.value
