"""The loop-closure correction on the device (plslam_pgo_*, plslam_lc_correct_map[_dev], K40-K53) against the numpy
restatement of loopClosureOptimizationCovGraphG2O (tests/pgo_ref.py), and the envelope L D L^T alone
(plslam_envelope_ldlt_solve) against numpy and the dense device L D L^T."""
import numpy as np
import pytest

import plslam_amd
from plslam_amd import capi, pgo

import pgo_ref

pytestmark = pytest.mark.gpu


# ---- the envelope L D L^T alone ----------------------------------------------------------------------------------------------
def _banded_spd(n, bw, seed, ragged=True):
    rng = np.random.Generator(np.random.PCG64(seed))
    A = np.zeros((n, n))
    for r in range(n):
        w = int(rng.integers(0, bw + 1)) if ragged else bw
        c0 = max(0, r - w)
        A[r, c0:r] = rng.standard_normal(r - c0)
    A = A + A.T
    A[np.diag_indices(n)] = np.abs(A).sum(1) + 1.0 + rng.random(n)
    return A, rng.standard_normal(n)


@pytest.mark.parametrize("n,bw", [(6, 5), (60, 11), (600, 40), (1000, 107), (500, 112), (300, 113), (400, 250)])
def test_envelope_solve_agrees_with_numpy_and_the_dense_solve(ctx, n, bw):
    A, b = _banded_spd(n, bw, seed=n + bw)
    x, nb, width = capi.envelope_ldlt_solve(ctx, A, b)
    assert nb == 0 and width <= bw
    xr = np.linalg.solve(A, b)
    xd, nbd = capi.dense_ldlt_solve(ctx, A, b)
    assert nbd == 0
    for ref in (xr, xd):
        assert np.linalg.norm(x - ref) <= 1e-12 * np.linalg.norm(ref)
    assert np.linalg.norm(A @ x - b) <= 1e-12 * np.linalg.norm(b)


def test_envelope_solve_reports_a_zero_pivot(ctx):
    A, b = _banded_spd(40, 6, seed=3)
    A[10, :] = 0.0
    A[:, 10] = 0.0
    _, nb, _ = capi.envelope_ldlt_solve(ctx, A, b)
    assert nb >= 1


# ---- the pose graph ------------------------------------------------------------------------------------------------------------
CASES = {
    "kf12": dict(n_kf=12, period=9, n_after=1),
    "P1": dict(n_kf=120),
    "kf400_2loops": dict(n_kf=400, n_loops=2, seed=4),
    "null_slots": dict(n_kf=60, null_slots=(9, 20, 33, 58), seed=6),
    "dup_lc_edge": dict(n_kf=50, extra_lc=((30, 31),), seed=7),
    "several_lc_one_optimized": dict(n_kf=80, n_loops=3, extra_lc=((5, 70),), optimized=(0,), seed=8),
    "rejections": dict(n_kf=60, lc_noise=1.0, seed=9),
}


def _run(ctx, m, max_iters=100):
    plan = plslam_amd.PgoPlan(ctx, m["kf_valid"], m["full_graph"], m["lc_idx"], max_iters_pgo=max_iters)
    try:
        return plan.optimize(m["T_kf_w"], m["x_kf_w"], m["lc_pose"])
    finally:
        plan.close()


def _ref(m, max_iters=100):
    P = pgo_ref.Pgo(m["kf_valid"], m["full_graph"], m["lc_idx"])
    r = P.optimize(m["T_kf_w"], m["x_kf_w"], m["lc_pose"], max_iters=max_iters)
    return P, r, pgo_ref.write_back(P, r, m["T_kf_w"], m["x_kf_w"])


def _decisive(trace):
    """The trials whose chi' differs from chi by more than rounding: their accept / reject does not depend on the order of a
    sum.  Once the state has converged, chi' - chi is rounding noise and so is the sign of rho."""
    n = 0
    for t in trace:
        if t["ok"] and abs(t["chi"] - t["chi_new"]) <= 1e-9 * abs(t["chi"]):
            break
        n += 1
    return n


def _compare(got, ref, wb, x_tol=1e-9):
    tg, tr = got["trace"], ref["trace"]
    n = _decisive(tr)
    assert len(tg) >= n
    for a, b in zip(tg[:n], tr[:n]):
        assert (a["it"], a["trial"], a["ok"], a["accepted"]) == (b["it"], b["trial"], b["ok"], b["accepted"]), (a, b)
        assert a["chi"] == pytest.approx(b["chi"], rel=1e-9, abs=1e-300)
        assert a["chi_new"] == pytest.approx(b["chi_new"], rel=1e-9, abs=1e-300)
        assert a["lam"] == pytest.approx(b["lam"], rel=1e-9)
    if n < len(tr):        # the prefix runs up to convergence: what follows only moves chi by rounding
        assert tr[n]["chi"] == pytest.approx(ref["chi_final"], rel=1e-9)
    if n == len(tr):
        assert len(tg) == len(tr)
        assert got["iterations"] == ref["iterations"] and got["stop_reason"] == ref["stop"]
    T_out, x_out, T_corr, corrected = wb
    assert np.array_equal(got["corrected"], corrected)
    assert np.abs(got["x"] - x_out).max() <= x_tol
    assert np.abs(got["T"] - T_out).max() <= x_tol
    assert got["chi_initial"] == pytest.approx(ref["chi_initial"], rel=1e-9, abs=1e-300)
    return n


@pytest.mark.parametrize("name", list(CASES))
def test_optimize_matches_the_restatement(ctx, name):
    m = pgo.pose_graph(**CASES[name])
    got = _run(ctx, m)
    P, ref, wb = _ref(m)
    assert got["n_active"] == len(P.active) and got["n_edges"] == len(P.g["edges"])
    assert got["n_lc_edges"] == m["lc_idx"].shape[0]
    # a large residual (the rejections case) makes Gauss-Newton converge linearly: after the last decisive trial the state still
    # moves by ~1e-8 over trials whose acceptance is rounding, so where either run stops is too
    n = _compare(got, ref, wb, x_tol=1e-6 if name == "rejections" else 1e-9)
    assert n >= 2
    assert got["chi_final"] < 0.1 * got["chi_initial"]
    if name == "rejections":
        assert any(not t["accepted"] for t in ref["trace"][:n])


@pytest.mark.parametrize("max_iters", [0, 1, 100])
def test_iteration_limits(ctx, max_iters):
    m = pgo.pose_graph(n_kf=40, seed=12)
    got = _run(ctx, m, max_iters)
    _, ref, wb = _ref(m, max_iters)
    _compare(got, ref, wb)
    if max_iters < 100:
        assert got["iterations"] == max_iters and got["stop_reason"] == capi.PGO_STOP_MAX_ITERS
        assert len(got["trace"]) == len(ref["trace"])


def test_two_calls_give_the_same_bits(ctx):
    m = pgo.pose_graph(n_kf=120, seed=13)
    plan = plslam_amd.PgoPlan(ctx, m["kf_valid"], m["full_graph"], m["lc_idx"])
    try:
        a = plan.optimize(m["T_kf_w"], m["x_kf_w"], m["lc_pose"])
        b = plan.optimize(m["T_kf_w"], m["x_kf_w"], m["lc_pose"])
    finally:
        plan.close()
    for k in ("T", "x", "T_corr"):
        assert np.array_equal(a[k], b[k])
    assert a["trace"] == b["trace"]


def test_dense_comparison_path_agrees(ctx):
    m = pgo.pose_graph(n_kf=120, seed=14)
    env = _run(ctx, m)
    ctx.set_option("pgo_solver", 1)
    try:
        den = _run(ctx, m)
    finally:
        ctx.set_option("pgo_solver", 0)
    n = _decisive(env["trace"])
    for a, b in zip(env["trace"][:n], den["trace"][:n]):
        assert a["accepted"] == b["accepted"] and a["chi_new"] == pytest.approx(b["chi_new"], rel=1e-9)
    assert np.abs(env["x"] - den["x"]).max() <= 1e-9


def test_refusals(ctx):
    m = pgo.pose_graph(n_kf=30, seed=15)
    v, fg, lc = m["kf_valid"], m["full_graph"], m["lc_idx"]

    def refused(code, **kw):
        a = dict(kf_valid=v, full_graph=fg, lc_idx=lc)
        a.update(kw)
        with pytest.raises(plslam_amd.PlslamError) as e:
            plslam_amd.PgoPlan(ctx, a["kf_valid"], a["full_graph"], a["lc_idx"])
        assert e.value.code == code

    EINVAL, ERANGE = -1, -5
    bad = v.copy()
    bad[lc[0, 0]] = 0
    refused(EINVAL, kf_valid=bad)                                        # LC entry names a NULL keyframe
    refused(EINVAL, lc_idx=np.array([[0, 30, 1]], np.int32))             # out of range
    z = v.copy()
    z[0] = 0
    refused(EINVAL, kf_valid=z)                                          # keyframe 0 NULL
    refused(EINVAL, lc_idx=np.zeros((0, 3), np.int32))                   # no LC entry
    iso = pgo.pose_graph(n_kf=30, seed=15, null_slots=(10, 11, 12, 13, 14))
    lc_far = np.array([[16, 25, 1]], np.int32)                            # 15 .. 25 have no path to vertex 0
    refused(EINVAL, kf_valid=iso["kf_valid"], full_graph=iso["full_graph"], lc_idx=lc_far)
    big = pgo.pose_graph(n_kf=4200, n_loops=1, seed=1)
    refused(ERANGE, kf_valid=big["kf_valid"], full_graph=big["full_graph"], lc_idx=big["lc_idx"])


# ---- the map correction -----------------------------------------------------------------------------------------------------
def _corrected_map(ctx):
    m = pgo.pose_graph(n_kf=60, null_slots=(13, 57), n_after=4, seed=16)
    got = _run(ctx, m)
    assert got["corrected"][59] and not got["corrected"][57] and got["corrected"][58]   # later keyframes, a NULL one skipped
    pts = pgo.anchored_landmarks(60, 3000, seed=17, kf_valid=m["kf_valid"], n_double=20)
    lns = pgo.anchored_landmarks(60, 700, seed=18, line=True, kf_valid=m["kf_valid"], n_double=10)
    return m, got, pts, lns


def _ref_map(got, lm, line):
    return pgo_ref.correct_landmarks(got["T_corr"], got["corrected"], lm["anchor_ptr"], lm["anchor_idx"], lm["valid"], lm["X"],
                                     lm["med_dir"], lm["dir_ptr"], lm["dirs"], line=line)


def test_correct_map_is_bit_identical_to_the_restatement(ctx):
    m, got, pts, lns = _corrected_map(ctx)
    assert (np.bincount(pts["anchor_idx"], minlength=3000) >= 2).sum() >= 10      # doubly anchored landmarks
    assert (pts["valid"] == 0).any()                                               # NULL landmark slots
    gp, gl = capi.correct_map(ctx, got["T_corr"].reshape(-1, 16), got["corrected"], pts, lns)
    for g, lm, line in ((gp, pts, False), (gl, lns, True)):
        X, med, dirs = _ref_map(got, lm, line)
        assert np.array_equal(g["X"], X) and np.array_equal(g["med_dir"], med) and np.array_equal(g["dirs"], dirs)
        assert not np.array_equal(X, lm["X"])


def test_correct_map_dev_is_bit_identical_to_the_restatement(ctx):
    import torch
    m, got, pts, lns = _corrected_map(ctx)
    dev = torch.device("cuda", 0)
    keep = []

    def put(a):
        t = torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        keep.append(t)
        return t

    def kind(lm):
        d = {k: put(lm[k]) for k in ("anchor_ptr", "anchor_idx", "valid", "X", "med_dir", "dir_ptr", "dirs")}
        p = {k: t.data_ptr() for k, t in d.items()}
        p.update(n=lm["valid"].shape[0], n_anchor=lm["anchor_idx"].shape[0], n_dir=lm["dirs"].shape[0])
        return d, p

    Tc = put(got["T_corr"].reshape(-1, 16))
    co = put(got["corrected"].astype(np.uint8))
    dp, pp = kind(pts)
    dl, pl = kind(lns)
    torch.cuda.synchronize()
    capi.correct_map_dev(ctx, 60, Tc.data_ptr(), co.data_ptr(), pp, pl)
    for d, lm, line in ((dp, pts, False), (dl, lns, True)):
        X, med, dirs = _ref_map(got, lm, line)
        assert np.array_equal(d["X"].cpu().numpy(), X)
        assert np.array_equal(d["med_dir"].cpu().numpy(), med)
        assert np.array_equal(d["dirs"].cpu().numpy(), dirs)
