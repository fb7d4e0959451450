"""A C++ client (tests/cpp/test_map_insert_shim.cpp) uploads a generated map once and runs the KF <-> KF insertion and then the
map <-> KF insertion through plslam_amd/host/map_insert.hpp, i.e. the C ABI as MapHandler::addKeyFrame would call it, the image
staying on the device; the image, the events, row_delta and the counts it gets back must be the sequential restatement's."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import map_insert_cases as CS
import plslam_amd

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cpp_client_inserts_a_keyframe(ctx, tmp_path):
    lib = os.path.dirname(plslam_amd.LIB_PATH)
    exe = str(tmp_path / "test_map_insert_shim")
    subprocess.run([shutil.which("g++") or "g++", "-O2", "-std=c++17", "-D__HIP_PLATFORM_AMD__",
                    os.path.join(ROOT, "tests", "cpp", "test_map_insert_shim.cpp"), "-I" + os.path.join(ROOT, "include"),
                    "-I/opt/rocm/include", "-L" + lib, "-lplslam_hip", "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib",
                    "-L/opt/rocm/lib", "-lamdhip64", "-o", exe], check=True)
    m, kf, (_, out_a), kf_b, (m_b, out_b), _ = CS.run_ref("mixed")

    def put(name, a, dt):
        np.ascontiguousarray(a, dt).tofile(str(tmp_path / f"{name}.bin"))
    put("params", [kf["kf1"], kf["kf2"]], np.int32)
    put("T", np.concatenate([kf["T1"].ravel(), kf["T2"].ravel()]), np.float64)
    put("kf_valid", m["kf_valid"], np.uint8)
    put("x_kf_w", m["x_kf_w"], np.float64)
    for kind, tag in (("points", "pt"), ("lines", "ls")):
        for f in ("valid", "inlier", "X", "obs_ptr", "obs_kf", "obs_val", "feat_ptr", "feat_idx"):
            put(f"{tag}_{f}", m[kind][f], m[kind][f].dtype)
        put(f"{tag}_matches_12", kf[kind]["table"], np.int32)
        put(f"{tag}_map_to_kf", kf_b[kind]["table"], np.int32)
        for f in ("P1", "obs1", "P2", "obs2"):
            put(f"{tag}_{f}", kf[kind][f], np.float64)
    r = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr

    def got(name, dt):
        return np.fromfile(str(tmp_path / f"out_{name}.bin"), dt)
    for tag, out in (("a", out_a), ("b", out_b)):
        assert np.array_equal(got(f"{tag}_row_delta", np.int32), out["row_delta"]), tag
        for kind, k in (("points", "pt"), ("lines", "ls")):
            assert np.array_equal(got(f"{tag}_{k}_ev", np.int32), out[kind]["ev"].ravel()), (tag, kind)
            assert np.array_equal(got(f"{tag}_{k}_dir", np.uint64), out[kind]["dir"].ravel().view(np.uint64)), (tag, kind)
    ca, cb = ({k: o[k]["counts"] for k in ("points", "lines")} for o in (out_a, out_b))
    assert got("counts", np.int32).tolist() == [ca["points"]["n_events"], ca["points"]["n_new"], ca["points"]["n_skipped"],
                                                ca["lines"]["n_events"], ca["lines"]["n_new"], ca["lines"]["n_skipped"],
                                                cb["points"]["n_events"], cb["points"]["n_skipped"], cb["lines"]["n_events"],
                                                cb["lines"]["n_skipped"]]
    assert ca["points"]["n_new"] > 10 and ca["points"]["n_skipped"] > 10 and cb["points"]["n_events"] > 5
    assert np.array_equal(got("kf_valid", np.uint8), m_b["kf_valid"])
    assert np.array_equal(got("x_kf_w", np.uint64), m_b["x_kf_w"].ravel().view(np.uint64))
    for kind, tag in (("points", "pt"), ("lines", "ls")):
        for f in ("valid", "inlier", "X", "obs_ptr", "obs_kf", "obs_val", "feat_ptr", "feat_idx"):
            w = np.ascontiguousarray(m_b[kind][f]).ravel()
            g = got(f"{tag}_{f}", w.dtype)
            assert g.shape == w.shape, (kind, f, g.shape, w.shape)
            assert np.array_equal(g.view(np.uint64) if w.dtype == np.float64 else g, w.view(np.uint64) if w.dtype == np.float64 else w), (kind, f)
