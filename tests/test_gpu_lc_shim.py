"""A C++ client (tests/cpp/test_lc_shim.cpp) replays a seeded keyframe pair through plslam_amd/host/loop_closure.hpp and
prints what MapHandler::isLoopClosure leaves behind; checked against tests/lc_ref.py."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import plslam_amd
from plslam_amd import loop_closure as LC, synth
from oracle import oracle as O

import lc_ref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("over", [{}, dict(lc_rot=0.5)])
def test_cpp_client_replays_a_pair(tmp_path, over):
    lib = os.path.dirname(plslam_amd.LIB_PATH)
    exe = str(tmp_path / "test_lc_shim")
    subprocess.run([shutil.which("g++") or "g++", "-O2", "-std=c++17", os.path.join(ROOT, "tests", "cpp", "test_lc_shim.cpp"),
                    "-I" + os.path.join(ROOT, "include"), "-L" + lib, "-lplslam_hip", "-Wl,-rpath," + lib,
                    "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib", "-lamdhip64", "-o", exe], check=True)
    kf0, kf1, _ = LC.keyframe_pair(101, 1500, 200)
    for q, kf in enumerate((kf0, kf1)):
        for k, dt in (("pdesc", np.uint8), ("P", np.float64), ("pl", np.float64), ("pt_idx", np.int32), ("ldesc", np.uint8),
                      ("sPeP", np.float64), ("le", np.float64), ("ls_idx", np.int32)):
            np.ascontiguousarray(kf[k], dtype=dt).tofile(str(tmp_path / f"k{q}_{k}.bin"))
    (tmp_path / "meta.txt").write_text(f"{len(kf0['P'])} {len(kf0['sPeP'])} {len(kf1['P'])} {len(kf1['sPeP'])}\n")
    prm = dict(LC.DEFAULTS)
    prm.update(over)
    c = synth.EUROC
    vals = [c["fx"], c["fy"], c["cx"], c["cy"]] + [prm[k] for k in ("homog_th", "min_ratio_12_p", "min_ratio_12_l", "mutual",
                                                                     "has_points", "has_lines", "max_iters", "max_iters_ref",
                                                                     "lc_inlier_ratio", "lc_res", "lc_unc", "lc_inl", "lc_trs",
                                                                     "lc_rot")]
    (tmp_path / "params.txt").write_text(" ".join(repr(v) for v in vals) + "\n")
    r = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.split("\n")
    ref = lc_ref.is_loop_closure(prm, O.make_cam(**c), kf0, kf1)
    assert int(lines[0].split()[1]) == ref["is_lc"]
    pose = np.array([float(v) for v in lines[1].split()[1:]])
    npt = int(lines[2].split()[1])
    pt = np.array([[int(v) for v in ln.split()] for ln in lines[3:3 + npt]], np.int32).reshape(-1, 4)
    nls = int(lines[3 + npt].split()[1])
    ls = np.array([[int(v) for v in ln.split()] for ln in lines[4 + npt:4 + npt + nls]], np.int32).reshape(-1, 4)
    exp_pt, exp_ls = lc_ref.reference_outputs(ref)
    assert np.array_equal(pt, exp_pt) and np.array_equal(ls, exp_ls)
    if ref["is_lc"]:
        assert np.max(np.abs(pose - ref["pose_inc"])) <= 1e-9 * np.max(np.abs(ref["pose_inc"]))
