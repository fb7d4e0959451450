"""A C++ client (tests/cpp/test_pgo_shim.cpp) runs a drifted 400-keyframe map with two loops, NULL slots and anchored points
through plslam_amd/host/pgo.hpp, i.e. the C ABI as loopClosureOptimizationCovGraphG2O would call it; the result must be the
Python binding's, bit for bit."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import plslam_amd
from plslam_amd import capi, pgo

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cpp_client_runs_a_drifted_map(ctx, tmp_path):
    lib = os.path.dirname(plslam_amd.LIB_PATH)
    exe = str(tmp_path / "test_pgo_shim")
    subprocess.run([shutil.which("g++") or "g++", "-O2", "-std=c++17", os.path.join(ROOT, "tests", "cpp", "test_pgo_shim.cpp"),
                    "-I" + os.path.join(ROOT, "include"), "-L" + lib, "-lplslam_hip", "-Wl,-rpath," + lib,
                    "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib", "-lamdhip64", "-o", exe], check=True)
    m = pgo.pose_graph(n_kf=400, n_loops=2, null_slots=(50, 396), seed=19)
    lm = pgo.anchored_landmarks(400, 20000, seed=20, kf_valid=m["kf_valid"], n_double=30)
    (tmp_path / "meta.txt").write_text(f"{m['n_map_kf']} {lm['valid'].shape[0]}\n")
    for name, a, dt in (("T", m["T_kf_w"], np.float64), ("x", m["x_kf_w"], np.float64), ("lc_pose", m["lc_pose"], np.float64),
                        ("valid", m["kf_valid"], np.uint8), ("fg", m["full_graph"], np.int32), ("lc_idx", m["lc_idx"], np.int32),
                        ("aptr", lm["anchor_ptr"], np.int32), ("aidx", lm["anchor_idx"], np.int32),
                        ("dptr", lm["dir_ptr"], np.int32), ("pvalid", lm["valid"], np.uint8), ("X", lm["X"], np.float64),
                        ("med", lm["med_dir"], np.float64), ("dirs", lm["dirs"], np.float64)):
        np.ascontiguousarray(a, dtype=dt).tofile(str(tmp_path / f"{name}.bin"))
    r = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    plan = plslam_amd.PgoPlan(ctx, m["kf_valid"], m["full_graph"], m["lc_idx"])
    try:
        got = plan.optimize(m["T_kf_w"], m["x_kf_w"], m["lc_pose"])
    finally:
        plan.close()
    T_want = np.where(got["corrected"][:, None, None], got["T"], m["T_kf_w"])
    assert np.array_equal(np.fromfile(str(tmp_path / "T_out.bin")).reshape(-1, 4, 4), T_want)
    x_want = np.where(got["corrected"][:, None], got["x"], m["x_kf_w"])
    assert np.array_equal(np.fromfile(str(tmp_path / "x_out.bin")).reshape(-1, 6), x_want)
    gp, _ = capi.correct_map(ctx, got["T_corr"].reshape(-1, 16), got["corrected"], lm)
    assert np.array_equal(np.fromfile(str(tmp_path / "X_out.bin")).reshape(-1, 3), gp["X"])
    assert np.array_equal(np.fromfile(str(tmp_path / "med_out.bin")).reshape(-1, 3), gp["med_dir"])
    assert np.array_equal(np.fromfile(str(tmp_path / "dirs_out.bin")).reshape(-1, 3), gp["dirs"])
    assert np.array_equal(np.fromfile(str(tmp_path / "trace.bin")), np.array([t["chi_new"] for t in got["trace"]]))
