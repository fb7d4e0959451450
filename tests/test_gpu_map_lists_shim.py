"""A C++ client (tests/cpp/test_map_lists_shim.cpp) keeps a generated map AND its side lists on the device through
plslam_amd/host/map_lists.hpp, i.e. the C ABI as MapHandler would call it: the two insertions of a keyframe with a carry behind
each, and a loop-closure fusion with its carry.  The lists it brings back must be, to the bit, what the Python route
(plslam_amd.map_lists on the same inputs) leaves on the device -- which tests/test_gpu_map_lists.py pins to the replay."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import map_lists_ref as R
import plslam_amd
from plslam_amd import map_lists as ML
from test_gpu_map_lists import _fuse_pass, _insert_passes

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TAGS = (("points", "pt"), ("lines", "ls"))


@pytest.fixture(scope="module")
def client(tmp_path_factory):
    lib = os.path.dirname(plslam_amd.LIB_PATH)
    exe = str(tmp_path_factory.mktemp("map_lists_shim") / "test_map_lists_shim")
    subprocess.run([shutil.which("g++") or "g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-D__HIP_PLATFORM_AMD__",
                    os.path.join(ROOT, "tests", "cpp", "test_map_lists_shim.cpp"), "-I" + os.path.join(ROOT, "include"),
                    "-I/opt/rocm/include", "-L" + lib, "-lplslam_hip", "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib",
                    "-L/opt/rocm/lib", "-lamdhip64", "-o", exe], check=True)
    return exe


def _put(d, name, a, dt):
    np.ascontiguousarray(a, dt).tofile(str(d / f"{name}.bin"))


def _put_map(d, m, lists):
    _put(d, "kf_valid", m["kf_valid"], np.uint8)
    _put(d, "x_kf_w", m["x_kf_w"], np.float64)
    for kind, tag in TAGS:
        for f in ("valid", "inlier", "X", "obs_ptr", "obs_kf", "obs_val", "feat_ptr", "feat_idx"):
            _put(d, f"{tag}_{f}", m[kind][f], m[kind][f].dtype)
        for f in ("desc", "dir") + (("pts",) if kind == "lines" else ()):
            _put(d, f"{tag}_{f}", lists[kind][f], lists[kind][f].dtype)


def _same_as_the_python_route(d, dl, m_after):
    counts = np.fromfile(str(d / "out_counts.bin"), np.int32).tolist()
    assert counts == [m_after["points"]["n"], m_after["points"]["obs_kf"].size, m_after["lines"]["n"], m_after["lines"]["obs_kf"].size]
    for kind, tag in TAGS:
        for f in ML._fields_of(kind):
            want = dl.host(f"{kind}.{f}")
            got = np.fromfile(str(d / f"out_{tag}_{f}.bin"), want.dtype).reshape(want.shape)
            assert np.array_equal(got.view(np.uint64) if want.dtype == np.float64 else got,
                                  np.ascontiguousarray(want).view(np.uint64) if want.dtype == np.float64 else want), (kind, f)
        assert dl.host(f"{kind}.refreshed").sum() >= 3


def test_cpp_client_carries_the_lists_through_a_keyframe(ctx, client, tmp_path):
    r = R.run_insert("mixed")
    _, dl2 = _insert_passes(ctx, r)
    m, kf, kf_b = r["m"], r["kf"], r["kf_b"]
    _put_map(tmp_path, m, r["lists0"])
    _put(tmp_path, "params", [kf["kf1"], kf["kf2"]], np.int32)
    _put(tmp_path, "T", np.concatenate([kf["T1"].ravel(), kf["T2"].ravel()]), np.float64)
    for kind, tag in TAGS:
        _put(tmp_path, f"{tag}_matches_12", kf[kind]["table"], np.int32)
        _put(tmp_path, f"{tag}_map_to_kf", kf_b[kind]["table"], np.int32)
        for f in ("P1", "obs1", "P2", "obs2"):
            _put(tmp_path, f"{tag}_{f}", kf[kind][f], np.float64)
        for f, a in r["rows_a"][kind].items():
            _put(tmp_path, f"{tag}_{f}", a, a.dtype)
    p = subprocess.run([client, str(tmp_path), "insert"], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr
    _same_as_the_python_route(tmp_path, dl2, r["m_b"])


def test_cpp_client_carries_the_lists_through_a_fusion(ctx, client, tmp_path):
    r = R.run_fuse("three_entries")
    dl = _fuse_pass(ctx, r)
    m, lc = r["m"], r["lc"]
    _put_map(tmp_path, m, r["lists0"])
    _put(tmp_path, "lc_idx", lc["lc_idx"], np.int32)
    _put(tmp_path, "T_kf_w", lc["T_kf_w"], np.float64)
    for kind, tag in TAGS:
        for f, dt in (("tuples", np.int32), ("entry_ptr", np.int32), ("P0", np.float64), ("obs0", np.float64), ("P1", np.float64), ("obs1", np.float64)):
            _put(tmp_path, f"{tag}_{f}", lc[kind][f], dt)
        for f, a in r["rows"][kind].items():
            _put(tmp_path, f"{tag}_{f}", a, a.dtype)
    p = subprocess.run([client, str(tmp_path), "fuse"], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr
    _same_as_the_python_route(tmp_path, dl, r["m_a"])
