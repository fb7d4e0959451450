"""CPU side of the global bundle adjustment (K26-K39): tests/gba_ref.py against the reference's own first-pass loops and its
text, the restatement's Schur + L D L^T solve against a dense solve, the trajectory-shaped map generator, and the C++ shim."""
import functools
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from plslam_amd import gba, synth
from oracle import oracle as O

import gba_cases
from gba_cases import DAMPED_ITERS, DAMPED_LAMBDA, STOP_DX_CASE, STOP_DX_ITERS
import gba_dense
import gba_ref

OCAM = O.make_cam(**synth.EUROC)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = np.finfo(np.float64).eps
REF_SRC = "/root/reference/src/mapHandler.cpp"


def _gba_text():
    if not os.path.exists(REF_SRC):
        pytest.skip("the reference source is not on this machine")
    src = open(REF_SRC).read()
    a = src.index("void MapHandler::levMarquardtOptimizationGBA")
    b = src.index("\n}\n", a)
    body = src[a:b]
    it = body.index("// LM iterations")
    return body[:it], body[it:]


def test_first_pass_equals_the_references_own_loops():
    m = gba.trajectory_map(6, 50, 16, obs_per_lm=3, loop=False, seed=5)
    P = gba_ref.Problem(OCAM, m)
    B = P.blocks(True, m["x_kf"], m["Xw"], m["Lw"])
    H, g = P.full_H(B)
    T_map = m["T_kf_w"]
    pt, ls = m["pt_obs"], m["ls_obs"]
    ref = O.ref_lba_accumulate("gba", OCAM, 1e-7, P.nkf, T_map, T_map[1:], m["Xw"], m["Lw"], pt[:, 1], pt[:, 3], pt[:, 4],
                               m["pt_uv"], ls[:, 1], ls[:, 3], ls[:, 4], m["ls_l"])
    if ref is None:
        pytest.skip("oracle/_ref not built with the LBA harness (needs the reference at build time)")
    Hr, gr, er = ref
    np.testing.assert_allclose(H, Hr, rtol=1e-11, atol=1e-11 * np.abs(Hr).max())
    np.testing.assert_allclose(g, gr, rtol=1e-11, atol=1e-11 * np.abs(gr).max())
    assert np.isclose(B["err"], er, rtol=1e-11)


def test_the_text_the_findings_rest_on():
    first, loop = _gba_text()
    # 1: the observation counts are declared and never incremented; err is divided by them in both passes
    for t in (first, loop):
        assert "err /= (Npt_obs+Nls_obs);" in t
    body = first + loop
    assert "int Npt = 0, Npt_obs = 0;" in body and "int Nls = 0, Nls_obs = 0;" in body
    assert not re.search(r"N(pt|ls)_obs\s*(\+\+|\+=|=[^=])", body.replace("int Npt = 0, Npt_obs = 0", "")
                         .replace("int Nls = 0, Nls_obs = 0", ""))
    assert "if( err > err_prev ){" in loop and "lambda *= lambda_k;" in loop
    # 2: Hmax is an int
    assert "int Hmax = 0.0;" in first and "lambda *= Hmax;" in first
    # 3: the epsilon stops
    assert "if( abs(err-err_prev) < numeric_limits<double>::epsilon() || err < numeric_limits<double>::epsilon() )" in loop
    assert "if( DX.norm() < numeric_limits<double>::epsilon() )" in loop
    # 4: the pose x line cross blocks per pass
    assert "H.coeffRef(idx+i,jdx+j) += Hij(i,j);\n                        H.coeffRef(jdx+j,idx+i) += Hij(i,j);" in first
    assert "H.coeffRef(idx+i,jdx+j) += Hij(i,j);\n                            H.coeffRef(jdx+j,idx+i) += Hij(j,i);" in loop
    assert "SimplicialLDLT< SparseMatrix<double> > solver1(H);" in first and "SimplicialLDLT< SparseMatrix<double> > solver1(H);" in loop
    # 5: the first pass reads the stored poses; the iteration pass's points read the estimate, its lines the stored pose and
    # both end points from one stride-3 block
    assert first.count("Matrix4d Tiw   = map_keyframes[kf_idx_map]->T_kf_w;") == 2
    assert "Tiw = expmap_se3( X.block( 6*kf_idx_loc,0,6,1 ) );" in loop
    assert "Vector3d Pwj = X.block(6*Nkf+3*Npt+3*lm_idx_loc,0,3,1);" in loop
    assert "Vector3d Qwj = X.block(6*Nkf+3*Npt+3*lm_idx_loc,0,3,1);" in loop
    assert "Matrix4d Tiw   = map_keyframes[kf_idx_map]->T_kf_w;" in loop
    assert "SlamConfig::homogTh()" in loop and "0.0000001" not in loop
    # 6: keyframe 0 is not optimised
    src = open(REF_SRC).read()
    g = src[src.index("void MapHandler::globalBundleAdjustment"):src.index("void MapHandler::levMarquardtOptimizationGBA")]
    assert "if( (*kf_it)->kf_idx != 0 )" in g and "obs_aux(4) = -1;" in g


@pytest.mark.parametrize("first", [True, False])
@pytest.mark.parametrize("shape", [(5, 40, 0), (5, 0, 12), (7, 60, 20)])
def test_schur_ldlt_equals_a_dense_solve_of_the_lower_triangle(first, shape):
    n_kf, npt, nls = shape
    m = gba.trajectory_map(n_kf, npt, nls, obs_per_lm=3, loop=False, seed=17 + n_kf)
    P = gba_ref.Problem(OCAM, m)
    x = m["x_kf"] + 0.001
    B = P.blocks(first, x, m["Xw"], m["Lw"])
    if not first:
        B = dict(B, Wls=B["Wls"])
    H, g = P.full_H(B)       # lower blocks mirrored: the symmetric matrix SimplicialLDLT factors
    lam = 1e-3
    Hd = H + lam * np.diag(np.diag(H))
    ref = np.linalg.solve(Hd, g)
    s = gba_ref.schur_solve(P, B, lam)
    got = np.concatenate([s["dp"], s["dx_pt"].reshape(-1), s["dx_ls"].reshape(-1)])
    cond = np.linalg.cond(Hd)
    np.testing.assert_allclose(got, ref, rtol=0, atol=cond * 1e-15 * np.abs(ref).max())
    assert s["n_singular"] == 0 and s["n_bad"] == 0


def test_ldlt_restatement_on_indefinite_input():
    rng = np.random.Generator(np.random.PCG64(3))
    for n in (6, 65, 130):
        A = rng.standard_normal((n, n))
        A = A + A.T
        b = rng.standard_normal(n)
        x, bad = gba_ref.ldlt_solve(np.tril(A) + np.triu(rng.standard_normal((n, n)), 1), b)   # the upper triangle is ignored
        np.testing.assert_allclose(A @ x, b, atol=1e-8 * np.linalg.cond(A))
        assert bad == 0


def test_generator_is_banded_with_the_loop_block_and_deterministic():
    m = gba.trajectory_map(120, 3000, 500, obs_per_lm=4, loop=True, seed=9)
    blocks = gba.covisible_blocks(m)
    nkf = len(m["kf_list"])
    band = {(k1, k2) for k1, k2 in blocks if k1 - k2 <= 3}
    far = blocks - band
    assert far and all(k1 - k2 >= nkf - 4 for k1, k2 in far)          # only the loop links the two ends
    assert len(blocks) < 5 * nkf                                      # banded, not dense (nkf (nkf + 1) / 2 = 7140)
    assert all((k, k) in blocks for k in range(nkf))
    m2 = gba.trajectory_map(120, 3000, 500, obs_per_lm=4, loop=True, seed=9)
    for k, v in m.items():
        assert np.array_equal(np.asarray(v), np.asarray(m2[k])), k
    m3 = gba.trajectory_map(120, 3000, 500, obs_per_lm=4, loop=False, seed=9)
    assert all(k1 - k2 <= 3 for k1, k2 in gba.covisible_blocks(m3))
    # keyframe 0's observations carry local index -1 and every landmark is seen in front of its keyframes
    assert (m["pt_obs"][:, 4] == m["pt_obs"][:, 3] - 1).all() and (m["pt_obs"][m["pt_obs"][:, 3] == 0, 4] == -1).all()


def test_restatement_loop_follows_the_reference_schedule():
    m = gba.trajectory_map(8, 200, 40, obs_per_lm=3, loop=False, seed=23)
    r = gba_ref.gba_lm(gba_ref.Problem(OCAM, m), m["x_kf"], m["Xw"], m["Lw"], max_iters=15)
    assert r["iters"] == 15 and r["stop_reason"] == 0 and len(r["trace"]) == 15
    lam0 = 1e-5 * np.trunc(r["hmax"])
    # the first solve leaves lambda alone (:2366-2380); every later one is accepted and multiplies it by lambda_k afterwards
    lam = lam0
    for i, t in enumerate(r["trace"]):
        assert t["accepted"] and t["lam"] == lam and np.isinf(t["err"])
        if i > 0:
            lam *= 10.0


def test_cpp_shim_compiles_against_the_header(tmp_path):
    exe = str(tmp_path / "test_gba_shim")
    cxx = shutil.which("g++") or "g++"
    subprocess.run([cxx, "-O1", "-std=c++17", "-fsyntax-only", os.path.join(ROOT, "tests", "cpp", "test_gba_shim.cpp"),
                    "-I" + os.path.join(ROOT, "include")], check=True)
    assert not os.path.exists(exe)


# ---- beyond the banded arc: the inputs of tests/gba_cases.py, from the input and the restatement alone -------------------------
ARC = {"arc_both": dict(n_kf=12, n_pt=300, n_ls=80), "arc_loop": dict(n_kf=120, n_pt=2400, n_ls=300, loop=True)}


@functools.lru_cache(maxsize=None)
def _run(name, max_iters=15, lambda_lm=0.00001):
    """(map, Problem, gba_lm's result) of a named input"""
    if name in ARC:
        m = gba.trajectory_map(**dict(dict(obs_per_lm=3, loop=False, seed=41), **ARC[name]))
    else:
        m = (gba_cases.INPUTS.get(name) or gba_cases.DEGENERATE[name])()
    P = gba_ref.Problem(OCAM, m)
    with np.errstate(all="ignore"):
        return m, P, gba_ref.gba_lm(P, m["x_kf"], m["Xw"], m["Lw"], max_iters=max_iters, lambda_lm=lambda_lm)


def plan_layout(m):
    """The covisible blocks of the GBA plan (plslam_amd/csrc/gba_lists.hpp), restated from its comment -- tests/test_gba_lists_cpu.py
    holds the lists the planner really builds against this: every ordered pair (o1, o2) of a landmark's
    observations by optimised keyframes with kf(o1) >= kf(o2) falls in lower block (kf(o1), kf(o2)); a block's point pairs
    come before its line pairs; a chunk holds at most 64 pairs of one kind; every diagonal block exists.
    -> {(k1, k2): (point pairs, line pairs, [chunk sizes])}"""
    nkf = len(m["kf_list"])
    cnt = {(k, k): [0, 0] for k in range(nkf)}
    for kind, obs in enumerate((m["pt_obs"], m["ls_obs"])):
        seen = {}
        for v in obs:
            if v[4] >= 0:
                seen.setdefault(int(v[1]), []).append(int(v[4]))
        for ks in seen.values():
            for k1 in ks:
                for k2 in ks:
                    if k1 >= k2:
                        cnt.setdefault((k1, k2), [0, 0])[kind] += 1
    return {b: (p, l, [min(64, n - i) for n in (p, l) for i in range(0, n, 64)]) for b, (p, l) in sorted(cnt.items())}


def test_chunks_blocks_hold_the_pair_counts_they_are_built_for():
    lay = plan_layout(gba_cases.chunks())
    assert {b: v[:2] for b, v in lay.items()} == gba_cases.CHUNK_BLOCKS
    assert lay[(1, 0)][2] == [63] and lay[(2, 1)][2] == [64, 1] and lay[(3, 0)][2] == [64, 64] and lay[(3, 1)][2] == [64, 64, 1]
    assert lay[(2, 0)][2] == [64, 64, 1]            # the point run ends on the chunk boundary, then 65 line pairs
    assert lay[(3, 2)][2] == [1]                    # an off-diagonal block of a single pair
    assert lay[(0, 0)][:2] == (255, 65) and lay[(0, 0)][2] == [64, 64, 64, 63, 64, 1]
    assert lay[(3, 3)][:2] == (258, 0) and lay[(3, 3)][2] == [64, 64, 64, 64, 2]


def test_ragged_tracks_and_scattered_blocks():
    m = gba_cases.ragged()
    nkf = len(m["kf_list"])
    lay = plan_layout(m)
    assert set(lay) == gba.covisible_blocks(m) | {(k, k) for k in range(nkf)}
    far = [b for b in lay if b[0] - b[1] > 10 and b != (nkf - 1, 0)]
    assert len(far) > 500 and len(lay) > 0.8 * nkf * (nkf + 1) / 2            # scattered over the whole triangle, not a band
    for kind, obs, n in (("pt", m["pt_obs"], m["npt"]), ("ls", m["ls_obs"], m["nls"])):
        lens = np.bincount(obs[:, 1], minlength=n)
        assert set(lens) == set(gba_cases.RAGGED_LENGTHS)
        for j in gba_cases.RAGGED_KF0_ONLY[kind]:
            assert obs[obs[:, 1] == j, 4].tolist() == [-1]                    # an empty range of K37's lm_ptr
        for j in gba_cases.RAGGED_KF0_PLUS_ONE[kind]:
            assert sorted(obs[obs[:, 1] == j, 3] == 0) == [False, True]
        rows = obs[obs[:, 1] == int(np.argmax(lens))]
        assert (np.diff(rows[:, 3]) < 0).any() and (np.diff(np.sort(rows[:, 3])) > 1).any()      # unsorted, non-consecutive


def test_gaps_index_maps():
    m = gba_cases.gaps()
    assert m["n_map_kf"] == 24 and m["kf_list"].tolist() == list(gba_cases.GAPS_KF_LIST)
    for obs in (m["pt_obs"], m["ls_obs"]):
        opt = obs[:, 4] >= 0
        assert (m["kf_list"][obs[opt, 4]] == obs[opt, 3]).all() and (obs[opt, 4] != obs[opt, 3] - 1).any()
        for k in gba_cases.GAPS_FIXED[1:]:                                     # fixed keyframes other than 0 observe
            assert (obs[obs[:, 3] == k, 4] == -1).all() and (obs[:, 3] == k).any()
    used = set(gba_cases.GAPS_KF_LIST + gba_cases.GAPS_FIXED)
    T = m["T_kf_w"].reshape(24, 16)
    assert all(np.isnan(T[k]).all() != (k in used) for k in range(24))         # a wrong slot read shows
    r = gba_cases.renumbered(m)
    opt = r["pt_obs"][:, 4] >= 0
    assert r["n_map_kf"] == 13 and (r["kf_list"][r["pt_obs"][opt, 4]] == r["pt_obs"][opt, 3]).all()
    assert np.isfinite(r["T_kf_w"]).all() and np.array_equal(r["pt_obs"][:, [0, 1, 2, 4, 5]], m["pt_obs"][:, [0, 1, 2, 4, 5]])


def test_unpadded_sizes():
    for name, nkf in (("nkf16", 16), ("nkf32", 32), ("no_obs_keyframe", 16), ("nan_landmark", 16)):
        assert len(_run(name)[0]["kf_list"]) == nkf and (6 * nkf) % 32 == 0


def reach(m, ref):
    """How often the LM loop takes each branch of expmap_se3 / logmap_se3 in K38's x <- logmap(expmap(x) inverse(expmap(dp))),
    and the largest pose angle: pose_small / pose_full (theta(x) < 1e-6 or not), dp_small / dp_full, log_small / log_full."""
    c = dict(pose_small=0, pose_full=0, dp_small=0, dp_full=0, log_small=0, log_full=0, max_angle=0.0)
    x = np.asarray(m["x_kf"], np.float64)
    for t in ref["trace"]:
        if t["accepted"]:
            for xk, dk in zip(x, t["dp"]):
                th, thd = np.sqrt(xk[3] ** 2 + xk[4] ** 2 + xk[5] ** 2), np.sqrt(dk[3] ** 2 + dk[4] ** 2 + dk[5] ** 2)
                c["pose_small" if th < 0.000001 else "pose_full"] += 1
                c["dp_small" if thd < 0.000001 else "dp_full"] += 1
                R = (gba_ref.expmap_se3(xk) @ gba_ref.inverse_se3(gba_ref.expmap_se3(dk)))[:3, :3]
                thl = np.arccos(min(1.0, max(-1.0, (R[0, 0] + R[1, 1] + R[2, 2] - 1.0) / 2.0)))
                c["log_full" if thl > 0.000001 else "log_small"] += 1
                c["max_angle"] = max(c["max_angle"], th)
            x = t["x_kf"]
    return c


def test_reach_counts_of_the_se3_branches():
    for name in ARC:
        c = reach(*_run(name)[::2])
        assert c["pose_small"] == 0 and c["log_small"] == 0, (name, c)                  # what the arc never sees
        assert c["max_angle"] < 1.3 or name == "arc_loop"          # (the closed loop turns about y through the whole circle)
        assert c["pose_full"] > 0 and c["dp_full"] > 0 and c["dp_small"] > 0
    c = reach(*_run("tumbling")[::2])
    assert c["pose_small"] == 2 and c["pose_full"] > 0 and c["dp_small"] > 0 and c["dp_full"] > 0, c   # w = 0 and |w| = 5e-7
    assert math.pi / 2 < c["max_angle"] < 2.8
    w = np.linalg.norm(_run("tumbling")[0]["x_kf"][:3, 3:], axis=1)
    assert w[0] == 0.0 and abs(w[1] - 5e-7) < 1e-20 and abs(w[2] - 2e-6) < 1e-20
    # under a damping of 1e3 Hmax no step turns a keyframe by 1e-6: the two small keyframes stay in logmap_se3's small branch
    c = reach(*_run("tumbling", DAMPED_ITERS, DAMPED_LAMBDA)[::2])
    assert c["log_small"] == 2 * DAMPED_ITERS == c["pose_small"] and c["log_full"] > 0 and c["dp_full"] == 0, c
    for name in ("rotated_about_x", "rotated_about_z", "rotated_generic"):
        x = _run(name)[0]["x_kf"][:, 3:]
        assert (np.abs(x) > 0.05).all(axis=1).any() and np.linalg.norm(x, axis=1).max() < 2.8          # a general axis


def test_singular_landmarks_and_bad_pivots_per_case():
    for name in gba_cases.INPUTS:
        assert all(t["n_singular"] == 0 and t["n_bad_pivots"] == 0 for t in _run(name)[2]["trace"]), name
    tr = _run("no_obs_keyframe")[2]["trace"]
    assert (tr[0]["n_singular"], tr[0]["n_bad_pivots"]) == (0, 6)                  # the zero 6 x 6 block of S, the last pivots
    assert all((t["n_singular"], t["n_bad_pivots"]) == (397, 96) for t in tr[1:])  # then every block but three points is NaN
    assert all((t["n_singular"], t["n_bad_pivots"]) == (30, 0) for t in _run("no_point_obs")[2]["trace"])
    m, _, ref = _run("nan_landmark")
    assert ref["trace"][0]["n_singular"] == 2 and ref["trace"][0]["n_bad_pivots"] > 0 and math.isfinite(ref["hmax"])


def test_the_device_bound_cannot_go_vacuous():
    """_check_against bounds the device's error by 100 cond(S) eps times the step: a condition on the inputs, not a measurement"""
    for name in gba_cases.INPUTS:
        m, P, ref = _run(name)
        frac = ref["hmax"] - math.floor(ref["hmax"])
        assert 1e-6 < frac < 1 - 1e-6, name
        for i, t in enumerate(ref["trace"]):
            S = t["S"]
            cond = np.linalg.cond(np.tril(S) + np.tril(S, -1).T)
            assert 100.0 * cond * EPS <= 1e-3, (name, i, cond)
        assert ref["stop_reason"] == 0 and len(ref["trace"]) == 15


def test_the_loop_stops_on_the_step_norm():
    """lambda grows tenfold per accepted solve, so ||DX|| falls by ten: with 40 iterations it passes eps.  The device's ||DX||
    agrees with the restatement's to 1e-5 (_check_against), so it crosses at the same solve if no solve's norm lies within a
    factor of 2 of eps."""
    _, _, ref = _run(STOP_DX_CASE, STOP_DX_ITERS)
    assert ref["stop_reason"] == 2 and ref["iters"] < STOP_DX_ITERS
    dx = np.array([t["dx_norm"] for t in ref["trace"]])
    assert dx[-1] < EPS / 2 and (dx[:-1] > 2 * EPS).all() and len(dx) == ref["iters"] + 1, dx[-3:]


@pytest.mark.parametrize("first", [True, False])
@pytest.mark.parametrize("name", list(gba_cases.SMALL))
def test_schur_solve_equals_a_long_double_elimination_of_the_whole_system(name, first):
    m = gba_cases.SMALL[name]()
    P = gba_ref.Problem(OCAM, m)
    assert 6 * P.nkf + 3 * P.npt + 6 * P.nls <= 1500
    B = P.blocks(first, m["x_kf"] + (0.0 if first else 0.001), m["Xw"], m["Lw"])
    lam = 1e-5 * np.trunc(np.abs(np.diag(P.full_H(B)[0])).max())
    Hd, g = gba_dense.damped_system(P, B, lam)
    ref = gba_dense.solve_long_double(Hd, g).astype(np.float64)
    s = gba_ref.schur_solve(P, B, lam)
    got = np.concatenate([s["dp"], s["dx_pt"].reshape(-1), s["dx_ls"].reshape(-1)])
    cond = np.linalg.cond(Hd)
    # the bound of test_schur_ldlt_equals_a_dense_solve_of_the_lower_triangle
    np.testing.assert_allclose(got, ref, rtol=0, atol=cond * 1e-15 * np.abs(ref).max())
    assert s["n_singular"] == 0 and s["n_bad"] == 0


def _axes():
    rng = np.random.Generator(np.random.PCG64(77))
    a = rng.standard_normal((4, 3))
    return a / np.linalg.norm(a, axis=1, keepdims=True)


@pytest.mark.parametrize("theta", [5e-7, 9.99e-7, 1.01e-6, 2e-6, 0.3, 2.8])
def test_se3_maps_against_the_full_formulas_in_long_double(theta):
    """expmap_se3: below 1e-6 it returns R = I, t = x[:3], dropping Rodrigues' first-order terms: |R - I| <= theta + theta^2 / 2
    per entry and |t - x[:3]| <= (theta / 2 + theta^2 / 6) |x[:3]|_1.  At and above 1e-6 the formula is complete and only
    rounds: sin, cos and the products to a few eps each (16 eps for R), and V's (1 - cos theta) / theta carries the eps of
    1 - cos divided by theta (16 eps (1 + 1 / theta) |x[:3]|_1 for t).
    logmap_se3 of that pose: theta = acos(c) and sine = sqrt(1 - c^2) come from the same rounded c = (tr R - 1) / 2, whose
    error is 2 eps: acos moves by 2 eps / sin theta, and w = theta (R - R^T)v / (2 sine) by that relative to theta plus the
    same relative to sine -- 2 eps (1 / (theta sin theta) + cos theta / sin^2 theta) |w|, within 8 eps |w| / sin^2 theta for
    every angle here, plus 16 eps of rounding.  Its translation V^-1 t inherits w's error through V (at most |t|_1 times it,
    times |V^-1| <= 4 below theta = 2.8) and the 1 / theta of V's first coefficient.  Below 1e-6 logmap_se3 returns w = 0 and
    t as it is: |w| <= theta and the V^-1 term (theta / 2 + theta^2) |t|_1 are dropped."""
    for axis in _axes():
        x = np.concatenate([[0.7, -1.3, 2.1], theta * axis])
        t1 = np.abs(x[:3]).sum()
        T, Tl = gba_ref.expmap_se3(x), gba_dense.expmap_ld(x)
        th = float(np.sqrt(np.sum(np.array(x[3:], np.longdouble) ** 2)))
        small = np.sqrt(x[3] * x[3] + x[4] * x[4] + x[5] * x[5]) < 0.000001
        assert small == (theta < 1e-6)
        bR = th + th * th / 2 if small else 16 * EPS
        bt = (th / 2 + th * th / 6) * t1 if small else 16 * EPS * (1 + 1 / th) * t1
        assert np.abs(T[:3, :3] - Tl[:3, :3]).max() <= bR and np.abs(T[:3, 3] - Tl[:3, 3]).max() <= bt
        if small:
            assert np.array_equal(T[:3, :3], np.eye(3)) and np.array_equal(T[:3, 3], x[:3])
        # logmap_se3 of the double pose against the long-double log of the same matrix
        y, yl = gba_ref.logmap_se3(T), gba_dense.logmap_ld(T)
        cosine = min(1.0, max(-1.0, (T[0, 0] + T[1, 1] + T[2, 2] - 1.0) / 2.0))
        if np.arccos(cosine) > 0.000001:
            bw = (8 * EPS / math.sin(th) ** 2 + 16 * EPS) * th
            assert np.abs(y[3:] - yl[3:]).max() <= bw, (theta, np.abs(y[3:] - yl[3:]).max(), bw)
            assert np.abs(y[:3] - yl[:3]).max() <= (bw + 16 * EPS * (1 + 1 / th)) * 4 * t1
        else:
            assert small and np.array_equal(y[3:], np.zeros(3)) and np.array_equal(y[:3], T[:3, 3])
            assert np.abs(yl[3:]).max() <= th and np.abs(y[:3] - yl[:3]).max() <= (th / 2 + th * th) * t1


def test_logmap_of_a_nan_pose_returns_a_zero_rotation_and_is_unchanged_on_finite_input():
    """logmap_se3 clamps cosine and sine by comparisons, as se3_dev.hpp and the C oracle do: a NaN passes both, theta is NaN,
    `theta > 1e-6` fails and w stays 0 with V = I, so a NaN pose comes back as (NaN, NaN, NaN, 0, 0, 0) -- what K38 leaves in
    x_kf behind a NaN step, and what the degenerate device tests compare the finite set with.  min / max, the earlier
    form, return their first argument for a NaN and gave theta = pi and w = NaN.  For finite input both forms are the same
    to the bit."""
    T = np.eye(4)
    T[:3, :] = np.nan
    with np.errstate(all="ignore"):
        x = gba_ref.logmap_se3(T)
    assert np.isnan(x[:3]).all() and np.array_equal(x[3:], np.zeros(3))
    T = gba_ref.expmap_se3(np.array([0.3, -0.2, 0.5, 0.4, -0.1, 0.2]))
    T[0, 0] = np.nan                                                   # one NaN on the diagonal is enough
    with np.errstate(all="ignore"):
        assert np.array_equal(gba_ref.logmap_se3(T)[3:], np.zeros(3))
    rng = np.random.Generator(np.random.PCG64(5))
    for x in np.concatenate([rng.standard_normal((20, 6)), [[1.0, 2.0, 3.0, 0.0, 0.0, 0.0], [0.1, 0.2, 0.3, 4e-7, 0.0, 3e-7]]]):
        T = gba_ref.expmap_se3(x)
        R = T[:3, :3]
        cosine = min(1.0, max(-1.0, (R[0, 0] + R[1, 1] + R[2, 2] - 1.0) / 2.0))
        sine = min(1.0, max(-1.0, np.sqrt(1.0 - cosine * cosine)))
        y = gba_ref.logmap_se3(T)
        th = np.arccos(cosine)
        if th > 0.000001:
            w = th * np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]]) / (2.0 * sine)
            assert np.array_equal(y[3:], w)
        else:
            assert np.array_equal(y[3:], np.zeros(3))


def _first_solve(m):
    """The restatement's state after the first solve of m, and _check_against's bound for it"""
    P = gba_ref.Problem(OCAM, m)
    B = P.blocks(True, m["x_kf"], m["Xw"], m["Lw"])
    hmax = np.abs(np.diag(P.full_H(B)[0])).max()
    assert 1e-3 < hmax - math.floor(hmax) < 1 - 1e-3                     # both frames truncate it to the same lambda_0
    x, X, L, S = gba_ref.one_step(P, True, m["x_kf"], m["Xw"], m["Lw"], 1e-5 * math.trunc(hmax))
    b = np.concatenate([x.reshape(-1), X.reshape(-1), L.reshape(-1)])
    start = np.concatenate([m["x_kf"].reshape(-1), m["Xw"].reshape(-1), m["Lw"].reshape(-1)])
    cond = np.linalg.cond(np.tril(S) + np.tril(S, -1).T)
    return (x, X, L), b, 1e-9 * np.abs(b).max() + 100.0 * cond * EPS * np.abs(b - start).max(), np.abs(b - start).max()


def test_where_the_first_solve_turns_with_the_world_frame():
    """What the device's frame-invariance test rests on, from the restatement alone.  A world transform G leaves every camera's
    view alone; J_X turns with R, so H_X' = R H_X R^T.  Marquardt's damping adds lambda diag(H): diag(R H R^T) is a
    permutation of diag(H) only for a signed permutation R, so the points-only ragged map under QUARTER_TURN gives the same
    first solve seen from the other frame (to _check_against's bound, once per run) -- and under a general rotation it does
    not: the steps differ by metres.  With lines the first pass is not covariant under any rotation: the reference writes
    the pose x line cross blocks transposed (J_L[a] J_T[x], mapHandler.cpp:2349-2350), which puts the rotated J_L on the pose
    index; the iteration pass, which writes the correct block into the lower triangle, is covariant again.  So the device
    test runs ragged's points."""
    full = gba_cases.ragged()
    m = gba_cases.points_only(full)
    G = gba_cases.QUARTER_TURN
    assert np.array_equal(np.abs(G[:3, :3]).sum(0), np.ones(3)) and np.array_equal(np.abs(G[:3, :3]).sum(1), np.ones(3))
    assert np.linalg.det(G[:3, :3]) == 1.0 and np.abs(G[:3, 3]).min() > 0.5
    mt = gba_cases.world_transform(m, G)
    assert np.linalg.norm(mt["x_kf"][:, 3:], axis=1).max() < 2.8            # away from logmap_se3's quirk at pi
    (s0, b0, bound, step), (s1, _, _, _) = _first_solve(m), _first_solve(mt)
    back = np.concatenate([v.reshape(-1) for v in gba_cases.moved(gba_ref.inverse_se3(G), *s1)])
    assert np.abs(back - b0).max() <= 2 * bound and step > 1e6 * bound
    # a general rotation: not the same solve
    Gg = gba_ref.expmap_se3(np.concatenate([G[:3, 3], gba_cases.FRAMES["generic"]]))
    s2 = _first_solve(gba_cases.world_transform(m, Gg))[0]
    back = np.concatenate([v.reshape(-1) for v in gba_cases.moved(gba_ref.inverse_se3(Gg), *s2)])
    assert np.abs(back - b0).max() > 1.0
    # with lines: the first pass differs, an iteration pass from the same state does not
    P, Pt, ft = gba_ref.Problem(OCAM, full), gba_ref.Problem(OCAM, gba_cases.world_transform(full, G)), gba_cases.world_transform(full, G)
    for first, same in ((True, False), (False, True)):
        a = gba_ref.one_step(P, first, full["x_kf"], full["Xw"], full["Lw"], 50.0)[:3]
        b = gba_cases.moved(gba_ref.inverse_se3(G), *gba_ref.one_step(Pt, first, ft["x_kf"], ft["Xw"], ft["Lw"], 50.0)[:3])
        d = max(np.abs(u - v).max() for u, v in zip(a, b))
        assert (d < 1e-9) if same else (d > 1e-3), (first, d)
