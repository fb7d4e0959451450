"""CPU side of the loop-closure check (K25): tests/lc_ref.py against the reference's own loop text and against itself,
the keyframe-pair generator, and the reference quirks the kernel keeps.

Second half: what the cases of tests/lc_cases.py cover is a condition on their inputs -- the restatement alone must take each
branch they exist for and must be rounding-stable on them, or the device tests (tests/test_gpu_loop_closure.py,
tests/test_gpu_lc_batch.py) prove nothing there."""
import math

import numpy as np
import pytest

from plslam_amd import loop_closure as LC, synth
from oracle import oracle as O

import lc_cases as CASES
import lc_ref
from test_gpu_loop_closure import REL, _margins, _rel

OCAM = O.make_cam(**synth.EUROC)


def _prm(**over):
    d = dict(LC.DEFAULTS)
    d.update(over)
    return d


def test_every_iterate_equals_the_reference_loop_text():
    if O.ref_pose_gn_accumulate(True, OCAM, 1e-7, np.eye(4), np.zeros((0, 3)), np.zeros((0, 2)), np.zeros(0, np.uint8),
                                np.zeros((0, 6)), np.zeros((0, 3)), np.zeros(0, np.uint8)) is None:
        pytest.skip("oracle/_ref was not built from the reference")
    kf0, kf1, _ = LC.keyframe_pair(3, 1500, 200)
    r = lc_ref.is_loop_closure(_prm(), OCAM, kf0, kf1)
    P, pl, S, le = r["corr_inputs"]
    assert len(r["trace"]) == 15
    for it in r["trace"]:
        pi = np.ones(len(P), np.uint8) if it["stage"] == 0 else r["pt_inlier"].astype(np.uint8)
        li = np.ones(len(S), np.uint8) if it["stage"] == 0 else r["ls_inlier"].astype(np.uint8)
        H, g, e, n = O.ref_pose_gn_accumulate(True, OCAM, 1e-7, it["T"], P, pl, pi, S, le, li)
        assert np.array_equal(H, it["H"]) and np.array_equal(g, it["g"]) and n == it["n"]
        assert e / (n[0] + n[1]) == it["e"]


def test_qr_restatement_solves_full_rank_systems_and_zero():
    rng = np.random.Generator(np.random.PCG64(1))
    for _ in range(50):
        A = rng.normal(size=(6, 6))
        H = A @ A.T + 1e-3 * np.eye(6)
        g = rng.normal(size=6)
        x, nz = lc_ref.colpiv_qr_solve(H, g)
        xe = np.linalg.solve(H, g)
        assert nz == 6 and np.max(np.abs(x - xe)) <= 1e-12 * np.max(np.abs(xe)) * np.linalg.cond(H) / 1e3 + 1e-12 * np.max(np.abs(xe))
    x, nz = lc_ref.colpiv_qr_solve(np.zeros((6, 6)), np.zeros(6))
    assert np.array_equal(x, np.zeros(6))
    x, nz = lc_ref.colpiv_qr_solve(np.diag([1.0, 2, 3, 0, 0, 0]), np.array([1.0, 2, 3, 0, 0, 0]))   # rank cut at 3
    assert nz == 3 and np.allclose(x, [1, 1, 1, 0, 0, 0], rtol=0, atol=1e-15)


def test_noise_free_pairs_recover_the_pose():
    pose = (0.08, -0.05, 0.12, 0.02, -0.015, 0.03)
    kf0, kf1, truth = LC.keyframe_pair(9, 600, 80, pose=pose, noise_px=0.0, outlier_frac=0.0, keep_frac=1.0, flip_p=0.02)
    r = lc_ref.is_loop_closure(_prm(max_iters=20, max_iters_ref=20), OCAM, kf0, kf1)
    assert r["is_lc"]
    # T_inc maps kf0's points into kf1's frame: the generating transform.  The source's step (J / max(th, |r|), g = J w) is
    # an IRLS step whose fixed point is approached slowly as the residuals vanish: both stages end on the
    # |e - err_prev| < eps test (:3682) -- e stopped changing -- with residuals of ~1e-4 px left, long before e < eps.
    # That bounds how close it gets: 1e-6, not 1e-8.
    res = np.concatenate([lc_ref.point_residuals(OCAM, r["T_inc"], *r["corr_inputs"][:2]),
                          lc_ref.line_residuals(OCAM, r["T_inc"], *r["corr_inputs"][2:])])
    print("stops", r["stops"], "e", r["e"], "residual px: max", res.max(), "median", np.median(res))
    assert r["stops"] == ["err_change", "err_change"] and r["e"] >= np.finfo(np.float64).eps
    assert 1e-6 < res.max() < 1e-2
    assert np.max(np.abs(r["T_inc"] - truth["T"])) <= 1e-6
    assert np.max(np.abs(r["pose_inc"] - O.logmap_se3(O.inverse_se3(truth["T"])))) <= 1e-6


def test_std_max_nan_asymmetry_and_the_gate():
    nan = float("nan")
    assert math.isnan(lc_ref.std_max(nan, 5.0)) and lc_ref.std_max(5.0, nan) == 5.0
    assert math.isnan(lc_ref.ratio(0, 0)) and lc_ref.ratio(3, 0) == math.inf
    # kf0 without points: max(NaN, 0) is NaN -> the points+lines gate fails; kf1 without points: max(0, NaN) = 0
    kf0, kf1, _ = LC.keyframe_pair(41, 300, 60)
    empty = dict(kf0, pdesc=kf0["pdesc"][:0], P=kf0["P"][:0], pl=kf0["pl"][:0], pt_idx=kf0["pt_idx"][:0])
    r = lc_ref.is_loop_closure(_prm(), OCAM, empty, kf1)
    assert math.isnan(r["inl_ratio_pt"]) and r["gn_ran"] == 0
    r = lc_ref.is_loop_closure(_prm(), OCAM, kf0, dict(kf1, pdesc=kf1["pdesc"][:0], P=kf1["P"][:0], pl=kf1["pl"][:0],
                                                       pt_idx=kf1["pt_idx"][:0]))
    assert r["inl_ratio_pt"] == 0.0 and r["gn_ran"] == 0
    assert lc_ref.is_loop_closure(_prm(has_points=0), OCAM, empty, kf1)["gn_ran"] == 1


def test_err_prev_is_carried_into_stage_two():
    kf0, kf1, _ = LC.keyframe_pair(3, 800, 100)
    r = lc_ref.is_loop_closure(_prm(), OCAM, kf0, kf1)
    s2 = [t for t in r["trace"] if t["stage"] == 1]
    s1 = [t for t in r["trace"] if t["stage"] == 0]
    assert s2[0]["err_prev"] == s1[-1]["e"] != 999999999.9


def test_lc_inl_is_ignored_and_e_h_are_the_last_assembled():
    kf0, kf1, _ = LC.keyframe_pair(31, 1500, 200)
    r = lc_ref.is_loop_closure(_prm(lc_inl=0.995), OCAM, kf0, kf1)
    assert r["ok_inl"] == 0 and r["is_lc"] == 1
    last = r["trace"][-1]
    assert np.array_equal(r["H"], last["H"]) and r["e"] == last["e"]
    # the last system was assembled at the T_inc BEFORE the final update
    assert not np.array_equal(last["T"], r["T_inc"])


def test_every_correspondence_rejected_gives_nan():
    kf0, kf1, _ = LC.keyframe_pair(51, 400, 50, outlier_frac=1.0, outlier_px=(60.0, 90.0), keep_frac=1.0)
    r = lc_ref.is_loop_closure(_prm(max_iters=0), OCAM, kf0, kf1)
    assert r["n_pt_inliers"] == 0 and r["n_ls_inliers"] == 0
    assert math.isnan(r["e"]) and math.isnan(r["cov_eig"]) and r["stops"][1] == "x_small" and r["is_lc"] == 0
    assert np.array_equal(r["T_inc"], np.eye(4))


def test_params_record_defaults():
    p = LC.params()
    assert (p.max_iters, p.max_iters_ref, p.lc_res, p.lc_unc, p.lc_inl, p.lc_trs, p.lc_rot, p.lc_inlier_ratio) == \
        (5, 10, 1.5, 0.01, 0.3, 1.5, 35.0, 30.0)
    assert abs(p.min_ratio_12_p - 0.75) < 1e-7 and p.cam.fx == synth.EUROC["fx"]
    with pytest.raises(KeyError):
        LC.params(lc_bogus=1)


def test_lc_shim_compiles_against_the_abi(tmp_path):
    """plslam_amd/host/loop_closure.hpp and its C++ client compile and link against the C-ABI library (no device needed)."""
    import os
    import shutil
    import subprocess
    import plslam_amd
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    lib = os.path.dirname(plslam_amd.LIB_PATH)
    subprocess.run([shutil.which("g++") or "g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror",
                    os.path.join(root, "tests", "cpp", "test_lc_shim.cpp"), "-I" + os.path.join(root, "include"),
                    "-L" + lib, "-lplslam_hip", "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib",
                    "-lamdhip64", "-o", str(tmp_path / "test_lc_shim")], check=True)


# ---- the cases of tests/lc_cases.py ---------------------------------------------------------------------------------------
TRANSLATION = (0, 1, 2)
VALUES = ("e", "t", "r", "cov_eig")
EXACT = ("is_lc", "gn_ran", "iters_1", "iters_2", "ok_res", "ok_unc", "ok_inl", "ok_trs", "ok_rot", "n_pt_inliers",
         "n_ls_inliers", "stops")


def _pivots(name):
    return {q["tr"] for q in CASES.reference(name)[2]["qr"]}


def _lu(name):
    (lu,) = CASES.reference(name)[2]["lu"]
    return lu


def _sides(name):
    """per call site of std::max(homog_th, .): rows that took (homog_th, the value), summed over the case's first-stage
    iterations (where every row is an inlier)"""
    ref, prm, _ = CASES.reference(name)
    P, pl, S, le = ref["corr_inputs"]
    cam = CASES.ocam(CASES.case(name)[1])
    tot = {}
    for it in (t for t in ref["trace"] if t["stage"] == 0):
        for k, (a, b) in lc_ref.dmax_sides(cam, prm["homog_th"], it["T"], P, pl, S, le).items():
            tot[k] = (tot.get(k, (0, 0))[0] + a, tot.get(k, (0, 0))[1] + b)
    return tot


def test_instrumentation_changes_no_result():
    rng = np.random.Generator(np.random.PCG64(3))
    A = rng.standard_normal((9, 6))
    H, g = A.T @ A, rng.standard_normal(6)
    qr, lu = [], []
    x0, n0 = lc_ref.colpiv_qr_solve(H, g)
    x1, n1 = lc_ref.colpiv_qr_solve(H, g, qr)
    assert np.array_equal(x0, x1) and n0 == n1 == qr[0]["rank"] == 6 and len(qr[0]["tr"]) == 6
    assert all(k <= b < 6 for k, b in enumerate(qr[0]["tr"]))
    assert np.array_equal(lc_ref.lu_inverse(H), lc_ref.lu_inverse(H, lu)) and not lu[0]["zero_pivot"]
    assert np.allclose(lc_ref.lu_inverse(H) @ H, np.eye(6), atol=1e-9) and np.allclose(H @ x0, g, atol=1e-9)
    lu = []
    lc_ref.lu_inverse(np.zeros((6, 6)), lu)
    assert lu[0] == dict(swaps=[0] * 6, zero_pivot=True)
    name = "n255"
    over, cam, kf0, kf1 = CASES.case(name)
    ref, prm, log = CASES.reference(name)
    plain = lc_ref.is_loop_closure(prm, CASES.ocam(cam), kf0, kf1)
    for k in VALUES + ("T_inc", "pose_inc", "H", "g", "pt_inlier", "ls_inlier"):
        assert np.array_equal(np.asarray(plain[k]), np.asarray(ref[k]), equal_nan=True), k
    assert len(log["qr"]) == ref["iters_1"] + ref["iters_2"] and len(log["lu"]) == 1


def test_each_case_reaches_what_it_is_for():
    P = {n: _pivots(n) for n in CASES.NAMES}
    R = {n: CASES.reference(n)[0] for n in CASES.NAMES}
    assert all(R[n]["gn_ran"] == 1 for n in CASES.NAMES)
    # the pivot lists: the forward-facing scene takes a rotation column in each of its first three steps
    for n in ("far50", "far1000", "no_idx0", "no_idx") + tuple(CASES.COUNT_NAMES):
        assert P[n] <= {(4, 3, 5, 3, 4, 5), (4, 3, 5, 4, 4, 5), (3, 4, 5, 3, 4, 5), (3, 4, 5, 4, 4, 5), (4, 3, 5, 4, 5, 5)}, n
    assert P["near"] == {(0, 1, 2, 3, 4, 5), (0, 1, 2, 4, 4, 5), (1, 1, 2, 4, 4, 5)}
    assert P["tele"] == {(3, 4, 3, 4, 5, 5), (3, 4, 4, 3, 5, 5), (4, 3, 3, 4, 5, 5), (4, 3, 4, 3, 5, 5)}
    assert P["tele_near"] == {(0, 1, 3, 4, 4, 5), (0, 1, 4, 3, 4, 5), (1, 1, 3, 4, 4, 5)}
    assert P["lines_near"] == {(1, 1, 2, 3, 5, 5), (1, 1, 2, 5, 5, 5)}
    assert len(P["th1"]) >= 4 and all(tr[0] in (3, 4) for tr in P["th1"])
    assert P["nan_landmark"] == {(0, 1, 2, 3, 4, 5)}          # every comparison with a NaN norm is false: no exchange
    assert P["still_p"] == P["still_pl"] == set()             # err_small stops in front of the solve
    # across the cases
    every = set().union(*P.values())
    assert len(every) >= 10, sorted(every)
    assert any(tr[0] in TRANSLATION for n in CASES.VALUE_COMPARED for tr in P[n])
    assert all(tr[0] in TRANSLATION for tr in P["lines_near"])            # a lines-only system takes translation first
    assert all(q["rank"] == 6 for n in CASES.NAMES for q in CASES.reference(n)[2]["qr"])
    # the norm downdate recomputes only far away
    rec = {n: sum(q["recomputes"] for q in CASES.reference(n)[2]["qr"]) for n in CASES.NAMES}
    assert rec["far1000"] > 0 and rec["points_far"] > 0
    assert all(v == 0 for n, v in rec.items() if n not in ("far1000", "points_far")), rec
    # the LU's row exchanges
    want = {"near": [0] * 6, "lines_near": [0] * 6, "far50": [4, 2, 3, 0, 1, 0], "far1000": [4, 2, 3, 0, 1, 0],
            "points_far": [4, 2, 3, 2, 0, 0], "tele": [4, 2, 2, 0, 0, 0], "tele_near": [0, 0, 2, 0, 0, 0], "th1": [4, 2, 0, 0, 0, 0]}
    for n, swaps in want.items():
        assert _lu(n)["swaps"] == swaps and not _lu(n)["zero_pivot"], (n, _lu(n))
    assert _lu("still_p") == dict(swaps=[0] * 6, zero_pivot=True)
    assert len({tuple(_lu(n)["swaps"]) for n in CASES.VALUE_COMPARED}) >= 6
    # the stops: err_small only where nothing moves, after one iteration per stage
    for n in CASES.NAMES:
        still = n in ("still_p", "still_pl")
        assert R[n]["stops"] == (["err_small"] * 2 if still else [None, None]), (n, R[n]["stops"])
        assert (R[n]["iters_1"], R[n]["iters_2"]) == ((1, 1) if still else (5, 10)), n
    # std::max(homog_th, .): the value wins everywhere at 1e-7, both arguments at every call site of th1
    for n in ("near", "tele", "n257"):
        assert all(a == 0 and b > 0 for a, b in _sides(n).values()), (n, _sides(n))
    s = _sides("th1")
    assert set(s) == {"pt_z2", "ls_z2", "pt_r", "ls_r"} and all(a >= 8 and b >= 8 for a, b in s.values()), s


def test_counts_and_ratios():
    for n, (n_pt, n_ls) in CASES.COUNT_NAMES.items():
        ref = CASES.reference(n)[0]
        assert (ref["common_pt"], ref["common_ls"]) == (n_pt, n_ls)                 # every row matches
        assert ref["inl_ratio_pt"] == ref["inl_ratio_ls"] == 100.0
    for n, kf in (("cut_kf1", 0), ("cut_kf0", 1)):
        over, cam, kf0, kf1 = CASES.case(n)
        ref = CASES.reference(n)[0]
        assert {len(kf0["P"]), len(kf1["P"])} == {255, 513} and len((kf0, kf1)[kf]["P"]) == 513
        assert (ref["common_pt"], ref["common_ls"]) == (255, 63) and ref["is_lc"] == 1
        # the two ratios under std::max differ, and the larger is the second one exactly where kf1 is the cut keyframe
        r0, r1 = lc_ref.ratio(255, len(kf0["P"])), lc_ref.ratio(255, len(kf1["P"]))
        assert r0 != r1 and ref["inl_ratio_pt"] == max(r0, r1) == 100.0 and (r1 > r0) == (n == "cut_kf1")
        assert ref["inl_ratio_ls"] == 100.0 and lc_ref.ratio(63, 129) < 100.0
    for n, cols in (("no_idx0", (0,)), ("no_idx", (0, 2))):
        ref = CASES.reference(n)[0]
        for rows in (ref["pt_corr"], ref["ls_corr"]):
            assert rows.shape[0] > 0 and all((rows[:, c] == -1).all() == (c in cols) for c in (0, 2))


def test_the_degenerate_cases_as_the_issue_states_them():
    r = CASES.reference("still_p")[0]
    assert r["e"] == 0.0 and not r["H"].any() and math.isnan(r["cov_eig"]) and r["is_lc"] == 0 and r["ok_unc"] == 0
    assert np.array_equal(r["T_inc"], np.eye(4)) and r["pt_inlier"].all() and r["n_pt_inliers"] == 257 and r["common_ls"] == 0
    r = CASES.reference("still_pl")[0]
    assert 0.0 < r["e"] < 1e-20 and r["is_lc"] == 0 and r["ok_unc"] == 0          # e is rounding noise, and so is all of H
    assert np.array_equal(r["T_inc"], np.eye(4)) and r["pt_inlier"].all() and r["ls_inlier"].all()
    r = CASES.reference("nan_landmark")[0]
    over, cam, kf0, kf1 = CASES.case("nan_landmark")
    bad = np.flatnonzero(np.isnan(kf0["P"]).any(axis=1))
    assert bad.size == 1 and bad[0] in r["pt_corr"][:, 1]                            # a matched row
    assert r["gn_ran"] == 1 and r["pt_inlier"].all() and r["ls_inlier"].all()        # NaN > chi is false: nothing is rejected
    assert math.isnan(r["e"]) and math.isnan(r["cov_eig"]) and r["is_lc"] == 0 and (r["iters_1"], r["iters_2"]) == (5, 10)


def _permuted(name, k):
    """the case's GN with its correspondence rows in another order; masks come back in the case's order"""
    ref, prm, _ = CASES.reference(name)
    P, pl, S, le = ref["corr_inputs"]
    rng = np.random.Generator(np.random.PCG64(1000 + k))
    pp, pq = rng.permutation(len(P)), rng.permutation(len(S))
    out = lc_ref.relpose_robust_gn(prm, CASES.ocam(CASES.case(name)[1]), P[pp], pl[pp], S[pq], le[pq])
    pi, li = np.empty(len(P), bool), np.empty(len(S), bool)
    pi[pp], li[pq] = out["pt_inlier"], out["ls_inlier"]
    return dict(out, pt_inlier=pi, ls_inlier=li)


def _move(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    if a.ndim == 0:
        if math.isnan(float(b)):
            return 0.0 if math.isnan(float(a)) else math.inf
        return abs(float(a) - float(b)) / abs(float(b)) if float(b) != 0.0 else (0.0 if float(a) == 0.0 else math.inf)
    return _rel(a, b)


def test_admissibility_is_a_condition_on_the_input(capsys):
    """A case's values are compared at REL = 1e-9 only if the restatement itself does not move by a tenth of that when its
    correspondences come in another order (its sums then round differently, as the device's tree does), and if no flag, mask
    or iteration count depends on the order.  A case that fails is re-seeded or re-scaled, never given a looser tolerance."""
    rows = []
    for n in CASES.IDENTITY:
        CASES.identity_problem(n)
    for n in CASES.VALUE_COMPARED + tuple(CASES.IDENTITY):
        ref, prm, _ = CASES.reference(n)
        _margins(ref, prm)                                       # 0.05 px, and 1 % around each threshold
        rp, rl = ref["res_at_outlier_pass"]
        res = np.concatenate([rp, rl])
        spread = 0.0
        for k in range(8):
            alt = _permuted(n, k)
            for f in EXACT:
                assert alt[f] == ref[f], (n, k, f)
            assert np.array_equal(alt["pt_inlier"], ref["pt_inlier"]) and np.array_equal(alt["ls_inlier"], ref["ls_inlier"]), (n, k)
            spread = max([spread] + [_move(alt[f], ref[f]) for f in VALUES + ("T_inc", "pose_inc")])
        assert 10.0 * spread <= REL, (n, spread)
        rows.append((n, spread, float(np.min(np.abs(res - lc_ref.CHI)))))
    with capsys.disabled():
        print("\ncase          spread under 8 row orders   nearest residual to sqrt(7.815) [px]")
        for n, s, m in rows:
            print(f"{n:<12}  {s:9.1e}                   {m:6.3f}")


def test_first_system_in_long_double_against_the_oracle(capsys):
    """lc_ref.first_system_ld shares no code with the oracle's C rows.  The oracle's distance from it is fp64 rounding on that
    input (a few eps per term, relative to the sum of the terms' magnitudes); ten times it is what the device test allows the
    device, whose tree sums the same terms in another order."""
    rows = []
    for n in CASES.VALUE_COMPARED:
        (H, g, e, _), dist = CASES.first_system(n)
        ref = CASES.reference(n)[0]
        assert ref["common_pt"] + ref["common_ls"] > 0
        if n == "still_p":
            # at rest every fp64 residual is exactly 0 and the long-double ones are the fp64 rounding of pl_obs: H and g are
            # rounding alone in both, the distance is 1 by construction and says nothing
            assert dist <= 1.0 and 0.0 <= float(e) < 1e-20 and ref["e"] == 0.0
        else:
            # n terms summed in sequence: at most ~n eps, and in practice a few eps sqrt(n); 1e-12 fails on any wrong term
            assert 0.0 < dist < 1e-12, (n, dist)
            assert _rel(ref["trace"][0]["H"], np.asarray(H, np.float64)) < 1e-11
            assert _rel(ref["trace"][0]["g"], np.asarray(g, np.float64)) < 1e-11
        rows.append((n, ref["common_pt"], ref["common_ls"], dist))
    with capsys.disabled():
        print("\ncase          points lines   oracle's distance from long double")
        for n, a, b, d in rows:
            print(f"{n:<12}  {a:6d} {b:5d}   {d:9.2e}")


def test_first_system_ld_sees_a_wrong_term():
    """the long-double system is a check, not an echo: one row's weight off by 1e-9 moves the oracle 1e4 distances away"""
    over, cam, _, _ = CASES.case("near")
    ref, prm, _ = CASES.reference("near")
    P, pl, S, le = ref["corr_inputs"]
    ld, dist = CASES.first_system("near")
    one = np.ones(len(P), np.uint8)
    H, g, e, (n_p, n_l) = O.pose_gn_accumulate(CASES.ocam(cam), prm["homog_th"], np.eye(4), P, pl, one, S, le, np.ones(len(S), np.uint8))
    assert lc_ref.system_distance(H, g, e / (n_p + n_l), ld) == dist
    assert lc_ref.system_distance(H * (1 + 1e-11), g, e / (n_p + n_l), ld) > 100 * dist
    one[7] = 0
    H, g, e, (n_p, n_l) = O.pose_gn_accumulate(CASES.ocam(cam), prm["homog_th"], np.eye(4), P, pl, one, S, le, np.ones(len(S), np.uint8))
    assert lc_ref.system_distance(H, g, e / (n_p + n_l + 1), ld) > 1e6 * dist
