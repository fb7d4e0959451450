"""A C++ client (tests/cpp/test_lc_correct_image_shim.cpp) runs the loop-closure correction of one packed map twice through
plslam_amd/host/pgo.hpp: pgo::run on containers with the map_*_kf_idx lists, and pgo::runResident on the device-resident image and
its dir lists, which takes no list.  Keyframes, landmarks and dir lists of the two must be identical, bit for bit."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import plslam_amd
from plslam_amd import local_map as LM
from plslam_amd import map_lists as ML
from plslam_amd import pgo

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_run_resident_equals_run_on_the_same_map(ctx, tmp_path):
    lib = os.path.dirname(plslam_amd.LIB_PATH)
    exe = str(tmp_path / "test_lc_correct_image_shim")
    subprocess.run([shutil.which("g++") or "g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-D__HIP_PLATFORM_AMD__",
                    os.path.join(ROOT, "tests", "cpp", "test_lc_correct_image_shim.cpp"), "-I" + os.path.join(ROOT, "include"),
                    "-I/opt/rocm/include", "-L" + lib, "-lplslam_hip", "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib",
                    "-L/opt/rocm/lib", "-lamdhip64", "-o", exe], check=True)
    g = pgo.pose_graph(n_kf=60, seed=23, null_slots=(7, 58))
    m = LM.synthetic_map(n_kf=60, n_pt=700, n_ls=180, seed=24, null_kf=(7, 58))
    lists = ML.synthetic_lists(m, seed=25, with_med=False)
    (tmp_path / "meta.txt").write_text(f"{g['n_map_kf']}\n")
    put = lambda name, a, dt: np.ascontiguousarray(a, dtype=dt).tofile(str(tmp_path / f"{name}.bin"))  # noqa: E731
    for name, a, dt in (("T", g["T_kf_w"], np.float64), ("x", g["x_kf_w"], np.float64), ("lc_pose", g["lc_pose"], np.float64),
                        ("valid", g["kf_valid"], np.uint8), ("fg", g["full_graph"], np.int32), ("lc_idx", g["lc_idx"], np.int32)):
        put(name, a, dt)
    for kind, tag in (("points", "pt"), ("lines", "ls")):
        K = m[kind]
        aptr, aidx = LM.anchor_lists(m, kind)
        for name, a, dt in (("valid", K["valid"], np.uint8), ("X", K["X"], np.float64), ("obs_val", K["obs_val"], np.float64),
                            ("dir", lists[kind]["dir"], np.float64), ("obs_ptr", K["obs_ptr"], np.int32), ("obs_kf", K["obs_kf"], np.int32),
                            ("aptr", aptr, np.int32), ("aidx", aidx, np.int32)):
            put(f"{tag}_{name}", a, dt)
    r = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout, r.stderr)
    rd = lambda name: np.fromfile(str(tmp_path / f"{name}.bin"))  # noqa: E731
    bits = lambda a: a.view(np.uint64)  # noqa: E731
    assert np.array_equal(bits(rd("run_T")), bits(rd("res_T"))) and np.array_equal(bits(rd("run_x")), bits(rd("res_x")))
    assert not np.array_equal(rd("run_T"), g["T_kf_w"].reshape(-1))
    assert np.array_equal(bits(rd("res_image_x")), bits(rd("res_x")))       # the image's x_kf_w follows the Keyframes'
    for kind, tag in (("points", "pt"), ("lines", "ls")):
        for f, before in (("X", m[kind]["X"]), ("dir", lists[kind]["dir"])):
            a, b = rd(f"run_{tag}_{f}"), rd(f"res_{tag}_{f}")
            assert a.shape == b.shape == (before.size,) and np.array_equal(bits(a), bits(b)), (kind, f)
            assert (a != before.reshape(-1)).mean() > 0.5, (kind, f)      # (most of the map was re-anchored)
    counts = np.fromfile(str(tmp_path / "counts.bin"), np.int32)
    assert counts[0] > 400 and counts[1] > 100 and counts[2] > counts[0] and counts[3] > counts[1]
