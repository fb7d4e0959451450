"""A C++ client (tests/cpp/test_lc_batch_shim.cpp) replays three keyframe pairs through the batch form of
plslam_amd/host/loop_closure.hpp in one call, then through its single form one by one: both must leave the same outputs, and
those are checked against tests/lc_ref.py."""
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
KEYS = (("pdesc", np.uint8), ("P", np.float64), ("pl", np.float64), ("pt_idx", np.int32), ("ldesc", np.uint8),
        ("sPeP", np.float64), ("le", np.float64), ("ls_idx", np.int32))


def _parse(lines, at):
    tag, b, _, is_lc = lines[at].split()
    pose = np.array([float(v) for v in lines[at + 1].split()[1:]])
    npt = int(lines[at + 2].split()[1])
    pt = np.array([[int(v) for v in ln.split()] for ln in lines[at + 3:at + 3 + npt]], np.int32).reshape(-1, 4)
    nls = int(lines[at + 3 + npt].split()[1])
    ls = np.array([[int(v) for v in ln.split()] for ln in lines[at + 4 + npt:at + 4 + npt + nls]], np.int32).reshape(-1, 4)
    return (tag, int(b), int(is_lc), pose, pt, ls), at + 4 + npt + nls


def test_cpp_client_replays_three_pairs_batched_and_single(tmp_path):
    lib = os.path.dirname(plslam_amd.LIB_PATH)
    exe = str(tmp_path / "test_lc_batch_shim")
    subprocess.run([shutil.which("g++") or "g++", "-O2", "-std=c++17", os.path.join(ROOT, "tests", "cpp", "test_lc_batch_shim.cpp"),
                    "-I" + os.path.join(ROOT, "include"), "-L" + lib, "-lplslam_hip", "-Wl,-rpath," + lib,
                    "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib", "-lamdhip64", "-o", exe], check=True)
    # an accepted pair, a pair the translation test rejects (every match is left), and a second candidate against pair 0's
    # kf1 (the top-K shape) that stops at the gate
    a0, a1, _ = LC.keyframe_pair(201, 1500, 200)
    b0, b1, _ = LC.keyframe_pair(202, 800, 100, pose=(1.3, -0.9, 0.8, 0.01, -0.02, 0.015))
    c0, _, _ = LC.keyframe_pair(203, 1500, 200)
    pairs = [(a0, a1, 0), (b0, b1, 0), (c0, a1, 1)]
    meta = [str(len(pairs))]
    for b, (k0, k1, shared) in enumerate(pairs):
        for q, kf in enumerate((k0, k1)):
            for k, dt in KEYS:
                np.ascontiguousarray(kf[k], dtype=dt).tofile(str(tmp_path / f"p{b}_k{q}_{k}.bin"))
        meta.append(f"{len(k0['P'])} {len(k0['sPeP'])} {len(k1['P'])} {len(k1['sPeP'])} {shared}")
    (tmp_path / "meta.txt").write_text("\n".join(meta) + "\n")
    prm = dict(LC.DEFAULTS)
    c = synth.EUROC
    vals = [c["fx"], c["fy"], c["cx"], c["cy"]] + [prm[k] for k in ("homog_th", "min_ratio_12_p", "min_ratio_12_l", "mutual",
                                                                     "has_points", "has_lines", "max_iters", "max_iters_ref",
                                                                     "lc_inlier_ratio", "lc_res", "lc_unc", "lc_inl", "lc_trs",
                                                                     "lc_rot")]
    (tmp_path / "params.txt").write_text(" ".join(repr(v) for v in vals) + "\n")
    r = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True, timeout=180)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.split("\n")
    recs, at = [], 0
    for _ in range(2 * len(pairs)):
        rec, at = _parse(lines, at)
        recs.append(rec)
    batch, single = recs[:3], recs[3:]
    refs = []
    for b, (k0, k1, _) in enumerate(pairs):
        assert batch[b][0] == "batch" and single[b][0] == "single" and batch[b][1] == single[b][1] == b
        assert batch[b][2] == single[b][2]
        assert np.array_equal(batch[b][3], single[b][3])                   # %.17g: every bit of pose_inc
        assert np.array_equal(batch[b][4], single[b][4]) and np.array_equal(batch[b][5], single[b][5])
        ref = lc_ref.is_loop_closure(prm, O.make_cam(**c), k0, k1)
        refs.append(ref)
        assert batch[b][2] == ref["is_lc"]
        exp_pt, exp_ls = lc_ref.reference_outputs(ref)
        assert np.array_equal(batch[b][4], exp_pt) and np.array_equal(batch[b][5], exp_ls)
        if ref["is_lc"]:
            assert np.max(np.abs(batch[b][3] - ref["pose_inc"])) <= 1e-9 * np.max(np.abs(ref["pose_inc"]))
    assert refs[0]["is_lc"] == 1 and refs[1]["gn_ran"] == 1 and refs[1]["ok_trs"] == 0 and refs[2]["gn_ran"] == 0
