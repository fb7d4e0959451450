"""A C++ client (tests/cpp/test_local_map_shim.cpp) rebuilds reference-shaped containers from a generated map and runs
formLocalMap(kf) -> the gather of localBundleAdjustment -> removeBadMapLandmarks through plslam_amd/host/local_map.hpp, i.e. the
C ABI as MapHandler::addKeyFrame would call it; every container it gets back must be the sequential restatement's."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import local_map_cases as CS
import plslam_amd

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cpp_client_runs_a_keyframe(ctx, tmp_path):
    lib = os.path.dirname(plslam_amd.LIB_PATH)
    exe = str(tmp_path / "test_local_map_shim")
    subprocess.run([shutil.which("g++") or "g++", "-O2", "-std=c++17", "-D__HIP_PLATFORM_AMD__",
                    os.path.join(ROOT, "tests", "cpp", "test_local_map_shim.cpp"), "-I" + os.path.join(ROOT, "include"),
                    "-I/opt/rocm/include", "-L" + lib, "-lplslam_hip", "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib",
                    "-L/opt/rocm/lib", "-lamdhip64", "-o", exe], check=True)
    m, p = CS.mixed(1500, null_kf=(7, 26))
    p = dict(p, anchor=21, max_kf_idx=36)
    np.array([p[k] for k in ("anchor", "min_cov", "window", "kf2", "max_kf_idx", "min_lm_obs")], np.int32).tofile(str(tmp_path / "params.bin"))
    for name in ("kf_valid", "x_kf_w", "row"):
        np.ascontiguousarray(m[name]).tofile(str(tmp_path / f"{name}.bin"))
    for kind, tag in (("points", "pt"), ("lines", "ls")):
        for f in ("valid", "inlier", "X", "obs_ptr", "obs_kf", "obs_val", "feat_ptr", "feat_idx"):
            np.ascontiguousarray(m[kind][f]).tofile(str(tmp_path / f"{tag}_{f}.bin"))
    r = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    ref, after = CS.run_ref(m, p)

    def got(name, dt, shape=(-1,)):
        return np.fromfile(str(tmp_path / f"out_{name}.bin"), dt).reshape(shape)
    for k in ("kf_local", "pt_local", "ls_local"):
        assert np.array_equal(got(k, np.uint8), ref[k]), k
    for k in ("kf_list", "pt_list", "ls_list"):
        assert np.array_equal(got(k, np.int32), ref[k]), k
    assert np.array_equal(got("pt_obs", np.int32, (-1, 6)), ref["pt_obs"]) and np.array_equal(got("ls_obs", np.int32, (-1, 6)), ref["ls_obs"])
    assert len(ref["pt_obs"]) > 300 and len(ref["ls_obs"]) > 50 and got("rc", np.int32)[0] == 0
    for k, w in (("X_aux", 1), ("pt_obs_uv", 2), ("ls_l_obs", 3)):
        assert np.array_equal(got(k, np.float64).view(np.uint64), ref[k].ravel().view(np.uint64)), k
    assert got("removed", np.int32)[0] == ref["pt_removed"].sum() + ref["ls_removed"].sum() > 10
    for kind, tag in (("points", "pt"), ("lines", "ls")):
        assert np.array_equal(got(tag + "_valid", np.uint8), after[kind]["valid"]), kind
        assert np.array_equal(got(tag + "_feat_idx", np.int32), after[kind]["feat_idx"]), kind
