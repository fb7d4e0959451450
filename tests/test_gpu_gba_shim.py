"""A C++ client (tests/cpp/test_gba_shim.cpp) runs a G1-sized map (400 keyframes, 40 k points, 6 k lines, one loop) through
plslam_amd/host/gba.hpp, i.e. the lists globalBundleAdjustment builds and the C ABI; the result must be the Python binding's."""
import os
import shutil
import subprocess

import numpy as np

import plslam_amd
from plslam_amd import gba, synth

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cpp_client_runs_a_g1_map(ctx, tmp_path):
    lib = os.path.dirname(plslam_amd.LIB_PATH)
    exe = str(tmp_path / "test_gba_shim")
    subprocess.run([shutil.which("g++") or "g++", "-O2", "-std=c++17", os.path.join(ROOT, "tests", "cpp", "test_gba_shim.cpp"),
                    "-I" + os.path.join(ROOT, "include"), "-L" + lib, "-lplslam_hip", "-Wl,-rpath," + lib,
                    "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib", "-lamdhip64", "-o", exe], check=True)
    m = gba.trajectory_map(400, 40000, 6000, obs_per_lm=4, loop=True, seed=11)
    c = synth.EUROC
    (tmp_path / "meta.txt").write_text(f"{m['n_map_kf']} {m['npt']} {m['nls']} {c['fx']!r} {c['fy']!r} {c['cx']!r} {c['cy']!r}\n")
    for k, name, dt in (("T_kf_w", "T", np.float64), ("x_kf", "x", np.float64), ("Xw", "Xw", np.float64), ("Lw", "Lw", np.float64),
                        ("pt_obs", "pt_obs", np.int32), ("ls_obs", "ls_obs", np.int32), ("pt_uv", "pt_uv", np.float64),
                        ("ls_l", "ls_l", np.float64)):
        np.ascontiguousarray(m[k], dtype=dt).tofile(str(tmp_path / f"{name}.bin"))
    r = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    cam = plslam_amd.make_cam(c["fx"], c["fy"], c["cx"], c["cy"])
    plan = plslam_amd.GbaPlan(ctx, cam, m["n_map_kf"], m["kf_list"], m["npt"], m["nls"], m["pt_obs"], m["pt_uv"], m["ls_obs"],
                              m["ls_l"])
    try:
        got = plan.optimize(m["T_kf_w"], m["x_kf"], m["Xw"], m["Lw"])
    finally:
        plan.close()
    assert got["n_solves"] == 15
    assert np.array_equal(np.fromfile(str(tmp_path / "T_out.bin")).reshape(-1, 4, 4), got["T"])
    assert np.array_equal(np.fromfile(str(tmp_path / "Xw_out.bin")).reshape(-1, 3), got["Xw"])
    assert np.array_equal(np.fromfile(str(tmp_path / "Lw_out.bin")).reshape(-1, 6), got["Lw"])
    tr = np.fromfile(str(tmp_path / "trace.bin")).reshape(-1, 3)
    assert np.array_equal(tr, np.array([[t["lam"], t["err_raw"], t["dx_norm"]] for t in got["trace"]]))
