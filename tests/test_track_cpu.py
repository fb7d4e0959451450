"""The tracker without a GPU: the two restatements of its rows (tests/track_ref.py) against each other, the back-projection
against the scene it inverts, the restated rows through tests/lc_ref.py against the scene's true motion, and
include/plslam_track.h held to what tests/test_abi.py asks of include/plslam_hip.h."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import plslam_amd
from plslam_amd import _lib, loop_closure as LC, synth, track as TR

import track_cases as TC
import track_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -53                          # the unit round-off of fp64
SEEDS = (1, 2, 3)
# The worst errors of the recovered motion over SEEDS x 4 pairs (300 + 60 features, half a pixel of noise, a tenth of the true
# rows outliers), as test_restated_rows_recover_the_true_motion prints them: 3.550e-3 m and 2.086e-2 degrees.  The estimate is
# limited by the noise, not by the arithmetic: ten times the worst seen, so that other seeds pass too.
MAX_T_ERR, MAX_R_ERR_DEG = 3.55e-2, 2.086e-1


def _bits(a):
    return np.ascontiguousarray(a, np.float64).reshape(-1).view(np.uint64)


scene_tables = TC.scene_tables


def test_the_two_restatements_agree_bit_for_bit_on_the_edge_tables():
    names, pairs = TC.edge_pairs()
    kept = nan = inf = 0
    for name, p in zip(names, pairs):
        a, b = track_ref.rows_seq(TC.CAM, p), track_ref.rows_vec(TC.CAM, p)
        for k in a:
            assert a[k].shape == b[k].shape and a[k].dtype == b[k].dtype, (name, k)
            if a[k].dtype == np.int32:
                assert np.array_equal(a[k], b[k]), (name, k)
            else:
                assert np.array_equal(_bits(a[k]), _bits(b[k])), (name, k)
        kept += a["pt_rows"].shape[0] + a["ls_rows"].shape[0]
        nan += int(np.isnan(a["le_obs"]).any())
        inf += int(np.isinf(a["P"]).any()) + int(np.isinf(a["sPeP"]).any())
        if "none" in name:
            assert a["pt_rows"].shape[0] == a["ls_rows"].shape[0] == 0
        if "all" in name:
            assert a["pt_rows"].shape[0] == len(p["m_pt"]) and a["ls_rows"].shape[0] == len(p["m_ls"])
        assert (np.diff(a["pt_rows"][:, 0]) > 0).all() and (np.diff(a["ls_rows"][:, 0]) > 0).all()      # ascending i1
    assert kept > 2000 and nan >= 5 and inf >= 10        # the zero-length segments and the zero disparities are among the kept rows


def test_batch_offsets_are_the_running_counts():
    pairs = TC.small_pairs(9)
    r = track_ref.batch(TC.CAM, pairs)
    assert r["pt_off"][0] == r["ls_off"][0] == 0 and r["pt_off"][-1] == r["P"].shape[0] and r["ls_off"][-1] == r["sPeP"].shape[0]
    for b, per in enumerate(r["per_pair"]):
        assert np.array_equal(r["pt_rows"][r["pt_off"][b]:r["pt_off"][b + 1]], per["pt_rows"])
        assert np.array_equal(r["ls_rows"][r["ls_off"][b]:r["ls_off"][b + 1]], per["ls_rows"])
    assert r["pt_off"][1] == 0 and r["pt_off"][5] == r["pt_off"][4] and r["pt_off"][9] == r["pt_off"][8]       # the empty pairs


def test_back_projection_of_exact_projections_recovers_the_points():
    """u = cx + fx x / z, v = cy + fx y / z, d = fx b / z in fp64 (fy = fx: a rectified pair), each operation rounded once
    (relative error <= U = 2^-53).  Then, to first order in U:
      d = fl(fl(fx b) / z): relative 2 U;  bd = fl(b / d): 3 U;  Z' = fl(bd fx): 4 U            -> |Z' - z| <= 4 U z
      t = fl(fl(fx x) / z): |dt| <= 2 U |t|;  u = fl(cx + t): |du| <= U |u| + 2 U |t|;
      fl(u - cx): U |t| more                                                                  -> U (|u| + 3 |t|) on (u - cx)
      X' = fl(bd (u - cx)): bd's 3 U and the product's U relative, the difference's error times bd = z / fx
                                                                    -> |X' - x| <= U (z / fx) (|u| + 3 |u - cx|) + 4 U |x|
    and the same for Y'.  The second-order terms are below 1e-15 of these; the bounds are asserted with a factor 1 + 1e-9."""
    cam = synth.KITTI00
    rng = np.random.Generator(np.random.PCG64(11))
    n = 20000
    z = rng.uniform(0.5, 80.0, n)
    x, y = rng.uniform(-1.5, 1.5, n) * z, rng.uniform(-0.5, 0.5, n) * z
    fx, cx, cy, b = (np.float64(cam[k]) for k in ("fx", "cx", "cy", "b"))
    u, v, d = cx + fx * x / z, cy + fx * y / z, fx * b / z
    X, Y, Z = track_ref.back_projection(cam, u, v, d)
    s = 1.0 + 1e-9
    ex, ey, ez = np.abs(X - x), np.abs(Y - y), np.abs(Z - z)
    bx = U * (z / fx) * (np.abs(u) + 3 * np.abs(u - cx)) + 4 * U * np.abs(x)
    by = U * (z / fx) * (np.abs(v) + 3 * np.abs(v - cy)) + 4 * U * np.abs(y)
    print("worst error / bound: x %.3f  y %.3f  z %.3f" % ((ex / bx).max(), (ey / by).max(), (ez / (4 * U * z)).max()))
    assert (ex <= s * bx).all() and (ey <= s * by).all() and (ez <= s * 4 * U * z).all()
    assert ex.max() > 0 and ez.max() > 0                  # (and the bound is not met by an exact identity)


def motion_error(T_est, T_true):
    dR = T_est[:3, :3] @ T_true[:3, :3].T
    ang = np.degrees(np.arccos(np.clip((np.trace(dR) - 1.0) / 2.0, -1.0, 1.0)))
    return float(np.linalg.norm(T_est[:3, 3] - T_true[:3, 3])), float(ang)


def test_restated_rows_recover_the_true_motion():
    import lc_ref
    from oracle import oracle as O
    cam = TR.SCENE_CAM
    ocam = O.make_cam(**cam)
    prm = LC.params_dict(LC.params(cam=cam))
    worst_t = worst_r = 0.0
    for seed in SEEDS:
        for b, p in enumerate(TR.track_scene(seed, 4, 300, 60)):
            r = track_ref.rows_seq(cam, scene_tables(p))
            assert r["pt_rows"].shape[0] > 100 and r["ls_rows"].shape[0] > 15
            # a row is a true prev -> curr pair that is stereo in both frames
            assert np.array_equal(p["m_pt"][r["pt_rows"][:, 0]], r["pt_rows"][:, 1])
            ref = lc_ref.relpose_robust_gn(prm, ocam, r["P"], r["pl_obs"], r["sPeP"], r["le_obs"])
            et, er = motion_error(np.asarray(ref["T_inc"]), p["T"])
            print(f"seed {seed} pair {b}: {r['pt_rows'].shape[0]} + {r['ls_rows'].shape[0]} rows, |dt| = {et:.3e} m, angle = {er:.3e} deg, "
                  f"inliers {ref['n_pt_inliers']} + {ref['n_ls_inliers']}")
            # the outlier pass finds the moved rows
            assert not ref["pt_inlier"][p["pt_out"][r["pt_rows"][:, 1]]].any()
            worst_t, worst_r = max(worst_t, et), max(worst_r, er)
    print(f"worst: {worst_t:.3e} m, {worst_r:.3e} deg")
    assert worst_t <= MAX_T_ERR and worst_r <= MAX_R_ERR_DEG


@pytest.mark.parametrize("which", ["pose", "chain"])
def test_the_references_of_the_device_tests_are_off_every_threshold(which):
    """What tests/test_gpu_track.py compares masks and decisions against: every pair's restated solve is clear of the outlier
    threshold and of the decision thresholds, runs on enough rows, and the chain's tables keep most of the true rows"""
    refs = TC.gn_references(which)
    sizes = TC.POSE_SIZES if which == "pose" else TC.CHAIN_SIZES
    assert len(refs) == len(sizes)
    for b, (rows, ref, prm) in enumerate(refs):
        TC.margins(ref, prm)
        n_pt, n_ls = sizes[b]
        assert (rows["pt_rows"].shape[0] > n_pt // 4) == (n_pt > 0) and (rows["ls_rows"].shape[0] > n_ls // 6) == (n_ls > 0), (b, rows["pt_rows"].shape, rows["ls_rows"].shape)
        assert np.isfinite(ref["T_inc"]).all() and ref["n_pt_inliers"] + ref["n_ls_inliers"] > 10
    if which == "chain":
        pairs, _ = TC.chain_pairs()
        for p, truth in zip(pairs, TC.chain_scene()):
            agree = (p["m_pt"] == truth["m_pt"])[truth["m_pt"] >= 0].mean()
            assert agree > 0.9, agree                                  # the matcher finds the true prev <-> curr rows


def test_scene_is_seeded_and_pair_b_does_not_depend_on_B():
    a, b = TR.track_scene(4, 3, 40, 10), TR.track_scene(4, 2, 40, 10)
    for k in ("kp_pl", "kp_cr", "seg_cl", "pdesc_cl", "ldesc_pr", "m_pt", "st_ls_curr"):
        assert np.array_equal(a[1][k], b[1][k])
    p = a[0]
    assert p["kp_pl"].dtype == np.float32 and p["seg_cr"].shape == (10, 4)
    fresh, non_stereo = (p["m_pt"] < 0).mean(), (p["st_pt_prev"] < 0).mean()
    assert 0.05 < fresh < 0.6 and 0.05 < non_stereo < 0.5 and p["pt_out"].any()
    s = TR.track_scene(4, 3, sizes=[(30, 0), (0, 12), (30, 12)])
    assert s[0]["seg_pl"].shape == (0, 4) and s[1]["kp_pl"].shape == (0, 2) and len(s[1]["m_ls"]) == 12
    # kp_r = kp_l - (fx b / z, 0) on the true stereo rows
    i = np.flatnonzero(p["st_pt_prev"] >= 0)
    dp, _ = TR.true_disparities(p, "p")
    assert np.allclose(dp[i], p["cam"]["fx"] * p["cam"]["b"] / p["X"][i, 2], rtol=0, atol=2e-4)
    assert np.array_equal(p["kp_pl"][i, 1], p["kp_pr"][p["st_pt_prev"][i], 1])


# ---- include/plslam_track.h to the standard of include/plslam_hip.h ---------------------------------------------------------
def _header_symbols():
    src = open(os.path.join(ROOT, "include", "plslam_track.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(plslam_[a-z0-9_]+)\s*\(", src)))


def test_track_header_symbols_all_exported_and_declared_exactly():
    syms = _header_symbols()
    assert len(syms) == 6 and "plslam_track_batch_run" in syms and "plslam_stereo_backproject_dev" in syms
    lib = ctypes.CDLL(plslam_amd.LIB_PATH)
    assert not [s for s in syms if not hasattr(lib, s)]
    assert sorted(_lib.HEADER_PROTOTYPES) == syms                       # nothing missing, nothing extra
    assert all(v[0] == "plslam_track.h" for v in _lib.HEADER_PROTOTYPES.values())
    assert not set(_lib.HEADER_PROTOTYPES) & set(_lib.PROTOTYPES)
    L = plslam_amd.load()
    for name, (_, argtypes, restype) in _lib.HEADER_PROTOTYPES.items():
        f = getattr(L, name)
        assert f.argtypes is not None and list(f.argtypes) == list(argtypes) and f.restype is restype, name


def test_track_header_is_plain_c(tmp_path):
    src = tmp_path / "abi.c"
    src.write_text('#include "plslam_track.h"\nint main(void) { return (int)sizeof(plslam_track_pair) - 112; }\n')
    for cmd in (["gcc", "-std=c99"], ["g++", "-std=c++11", "-x", "c++"]):
        r = subprocess.run(cmd + ["-Wall", "-Wextra", "-pedantic", "-Werror", "-I" + os.path.join(ROOT, "include"), "-fsyntax-only",
                                  str(src)], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]


def test_track_structs_have_the_header_layout(tmp_path):
    """sizeof and every offsetof of the two records, from a C program, against the ctypes structures"""
    fields = {"plslam_track_pair": TR.TrackPair, "plslam_track_buffers": TR.TrackBuffers}
    body = "".join(f'printf("{s} %zu\\n", sizeof({s}));\n' + "".join(f'printf("{s}.{n} %zu\\n", offsetof({s}, {n}));\n' for n, _ in c._fields_)
                   for s, c in fields.items())
    src = tmp_path / "lay.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "plslam_track.h"\nint main(void) {\n' + body + "return 0; }\n")
    exe = str(tmp_path / "lay")
    subprocess.run(["gcc", "-std=c99", "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe], check=True)
    got = dict(ln.split() for ln in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.splitlines())
    for s, c in fields.items():
        assert int(got[s]) == ctypes.sizeof(c)
        for n, _ in c._fields_:
            assert int(got[f"{s}.{n}"]) == getattr(c, n).offset, (s, n)


def test_the_track_source_is_built_and_the_surface_of_the_first_header_is_untouched():
    from plslam_amd import build as B
    assert "track.hip" in B.SOURCES and any(h.endswith("track_plan.hpp") for h in B.HEADERS)
    assert len(plslam_amd.ABI_SYMBOLS) == 153 and not [s for s in plslam_amd.ABI_SYMBOLS if "track" in s or "backproject" in s]
    assert "TrackBatch" not in plslam_amd.__all__ and len(plslam_amd.__all__) == 25


def test_track_pair_refuses_unknown_fields():
    with pytest.raises(KeyError):
        TR.track_pair(m_pts=1)
    p = TR.track_pair(m_pt=256, n_pt_prev=3)
    assert p.m_pt == 256 and p.n_pt_prev == 3 and p.m_ls is None and p.n_ls_curr == 0
