"""The loop-closure correction on the device (plslam_pgo_*, plslam_lc_correct_map[_dev], K40-K53) against the numpy
restatement of loopClosureOptimizationCovGraphG2O (tests/pgo_ref.py), and the envelope L D L^T alone
(plslam_envelope_ldlt_solve) against numpy and the dense device L D L^T."""
import numpy as np
import pytest

import plslam_amd
from plslam_amd import capi, pgo

import pgo_cases
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


def _block_banded_spd(n_blocks, bw, seed):
    """The envelope as the pose-graph plan builds it: all six rows of a block start at the first column of the block's lowest
    neighbour, 0 .. (bw - 5) // 6 blocks back; one block reaches the full distance, so the widest row (the block's last) is
    6 * ((bw - 5) // 6) + 5 wide."""
    rng = np.random.Generator(np.random.PCG64(seed))
    n, wb = 6 * n_blocks, (bw - 5) // 6
    back = rng.integers(0, wb + 1, n_blocks)
    back[n_blocks // 2] = wb
    A = np.zeros((n, n))
    for B in range(n_blocks):
        c0 = 6 * max(0, B - int(back[B]))
        for r in range(6 * B, 6 * B + 6):
            A[r, c0:r] = rng.standard_normal(r - c0)
    A = A + A.T
    A[np.diag_indices(n)] = np.abs(A).sum(1) + 1.0 + rng.random(n)
    return A, rng.standard_normal(n), 6 * wb + 5


# widths 107 (the last that fits the LDS window of 112), 113 (the first that does not), 149; no n is a multiple of 16
@pytest.mark.parametrize("n_blocks,bw", [(51, 108), (67, 114), (85, 150), (43, 114)])
def test_block_envelope_solve_agrees_with_numpy_and_the_dense_solve(ctx, n_blocks, bw):
    A, b, want = _block_banded_spd(n_blocks, bw, seed=n_blocks + bw)
    assert A.shape[0] % 16 != 0
    x, nb, width = capi.envelope_ldlt_solve(ctx, A, b)
    assert nb == 0 and width == want
    xr = np.linalg.solve(A, b)
    xd, nbd = capi.dense_ldlt_solve(ctx, A, b)
    assert nbd == 0
    for ref in (xr, xd):
        assert np.linalg.norm(x - ref) <= 1e-12 * np.linalg.norm(ref)
    assert np.linalg.norm(A @ x - b) <= 1e-12 * np.linalg.norm(b)


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


# ---- the pose graph beyond the planar circle (tests/pgo_cases.py; tests/test_pgo_cpu.py checks which branches each input reaches)
def _compare_steps(got, ref, n):
    """scale and rho of the first n (decisive) trials.  rho = (chi - chi') / scale is a difference: its bound is what 1e-9
    relative on chi, chi' and scale each allow."""
    for a, b in zip(got["trace"][:n], ref["trace"][:n]):
        assert a["scale"] == pytest.approx(b["scale"], rel=1e-9)
        tol = 1e-9 * (abs(b["chi"]) + abs(b["chi_new"])) / abs(b["scale"]) + 1e-9 * abs(b["rho"])
        assert abs(a["rho"] - b["rho"]) <= tol, (a, b)


def _compare_all(got, ref, wb, x_tol=1e-9):
    n = _compare(got, ref, wb, x_tol)
    _compare_steps(got, ref, n)
    assert np.abs(got["T_corr"] - wb[2]).max() <= x_tol
    return n


@pytest.mark.parametrize("name", list(pgo_cases.INPUTS))
def test_optimize_matches_the_restatement_off_the_circle(ctx, name):
    m = pgo_cases.INPUTS[name]()
    got = _run(ctx, m)
    P, ref, wb = _ref(m)
    assert got["n_active"] == len(P.active) and got["n_edges"] == len(P.g["edges"])
    # tumbling_rejections is the rejections case over again (1.5 rad of LC noise): a large residual makes Gauss-Newton converge
    # linearly, so after the last decisive trial the state still moves by ~1e-8 over trials whose acceptance is rounding
    n = _compare_all(got, ref, wb, x_tol=1e-6 if name == "tumbling_rejections" else 1e-9)
    assert n >= 2
    assert got["chi_final"] < 0.1 * got["chi_initial"]
    if name == "tumbling_rejections":
        assert any(not t["accepted"] for t in ref["trace"][:n])


@pytest.mark.parametrize("max_iters", [0, 1])
@pytest.mark.parametrize("name", ["tumbling", "near_5e-7", "near_5e-6", "near_3e-5", "near_2e-3"])
def test_stage_probes(ctx, name, max_iters):
    """max_iters_pgo = 0: the measurements, the initial guess and the write-back with no solve in between (chi_initial, T, x,
    T_corr).  1: one linearisation, its solve and the vertex update (the first trial's chi', scale and rho)."""
    m = pgo_cases.INPUTS[name]()
    got = _run(ctx, m, max_iters)
    _, ref, wb = _ref(m, max_iters)
    assert got["iterations"] == max_iters and len(got["trace"]) == len(ref["trace"])
    n = _compare_all(got, ref, wb)
    if max_iters == 0:
        assert got["trace"] == [] and got["chi_final"] == pytest.approx(ref["chi_initial"], rel=1e-9)
    else:
        assert n >= 1 and got["trace"][0]["accepted"]
        assert got["chi_final"] == pytest.approx(ref["chi_final"], rel=1e-9)


def test_device_chi_does_not_depend_on_the_world_frame(ctx):
    """The device against itself: a map conjugated by a world rotation has the chi of the original (1e-9 relative, the trace
    tolerance), and its corrected poses mapped back are the original's."""
    m0 = pgo.pose_graph(n_kf=60, seed=6)
    g0 = _run(ctx, m0)
    for name in pgo_cases.FRAMES:
        G = pgo_cases.frame(name)
        Gi = np.linalg.inv(G)
        g = _run(ctx, pgo_cases.conjugate(m0, G))
        assert g["chi_initial"] == pytest.approx(g0["chi_initial"], rel=1e-9)
        assert g["chi_final"] == pytest.approx(g0["chi_final"], rel=1e-9)
        assert np.abs(np.stack([Gi @ T @ G for T in g["T"]]) - g0["T"]).max() <= 1e-9
        assert np.array_equal(g["corrected"], g0["corrected"])


def _against_the_dense_path(ctx, m, env):
    ctx.set_option("pgo_solver", 1)
    try:
        den = _run(ctx, m)
    finally:
        ctx.set_option("pgo_solver", 0)
    n = _decisive(env["trace"])
    assert n >= 2
    for a, b in zip(env["trace"][:n], den["trace"][:n]):
        assert a["accepted"] == b["accepted"] and a["chi_new"] == pytest.approx(b["chi_new"], rel=1e-9)
    assert np.abs(env["x"] - den["x"]).max() <= 1e-9


@pytest.mark.parametrize("name", ["wide_band", "many_loops"])
def test_envelope_beyond_the_lds_window_inside_optimize(ctx, name):
    """The global-memory path of the factor and the solve on the 6-row-block envelope with + lambda I that optimize builds."""
    m = pgo_cases.wide_band() if name == "wide_band" else pgo_cases.many_loops()
    got = _run(ctx, m)
    assert got["env_width"] > 112
    _, ref, wb = _ref(m)
    assert _compare_all(got, ref, wb) >= 2
    _against_the_dense_path(ctx, m, got)


def test_envelope_of_the_last_lds_window_size_inside_optimize(ctx):
    m = pgo_cases.wide_band(window=8)
    got = _run(ctx, m)
    assert 100 <= got["env_width"] <= 112
    _, ref, wb = _ref(m)
    assert _compare_all(got, ref, wb) >= 2
    _against_the_dense_path(ctx, m, got)


def test_a_non_finite_pose_fails_every_factorisation(ctx):
    """a failed factorisation takes a zero step and chi' = DBL_MAX.  With a NaN in one stored pose every
    trial fails; rho is NaN, so each iteration makes one trial and nothing is accepted."""
    import warnings
    m = pgo_cases.with_nan_pose(pgo_cases.tumbling(n_kf=60, seed=35), 20)
    got = _run(ctx, m, 3)
    with warnings.catch_warnings(), np.errstate(all="ignore"):
        warnings.simplefilter("ignore")
        _, ref, wb = _ref(m, 3)
    assert len(ref["trace"]) == 3 and not any(t["ok"] or t["accepted"] for t in ref["trace"])
    assert len(got["trace"]) == got["trials"] == len(ref["trace"])
    for a, b in zip(got["trace"], ref["trace"]):
        assert (a["it"], a["trial"]) == (b["it"], b["trial"])
        assert not a["ok"] and not a["accepted"] and a["chi_new"] == pgo_ref.DBL_MAX == b["chi_new"]
        assert a["lam"] == pytest.approx(b["lam"], rel=1e-9)
    assert got["iterations"] == ref["iterations"] and got["stop_reason"] == ref["stop"]
    assert np.array_equal(got["corrected"], wb[3])


def test_correct_map_with_the_corrections_of_a_tumbling_run(ctx):
    m = pgo_cases.tumbling(n_kf=60, seed=36, n_after=4)
    got = _run(ctx, m)
    Rc = got["T_corr"][1:, :3, :3]
    assert (np.abs(Rc[:, [2, 0, 1], [1, 2, 0]] - Rc[:, [1, 2, 0], [2, 0, 1]]) > 1e-6).all(1).sum() >= 50     # turns about all axes
    pts = pgo.anchored_landmarks(60, 2000, seed=37, kf_valid=m["kf_valid"], n_double=20)
    lns = pgo.anchored_landmarks(60, 500, seed=38, line=True, kf_valid=m["kf_valid"], n_double=10)
    gp, gl = capi.correct_map(ctx, got["T_corr"].reshape(-1, 16), got["corrected"], pts, lns)
    for g, lm, line in ((gp, pts, False), (gl, lns, True)):
        X, med, dirs = _ref_map(got, lm, line)
        assert np.array_equal(g["X"], X) and np.array_equal(g["med_dir"], med) and np.array_equal(g["dirs"], dirs)
        assert not np.array_equal(X, lm["X"])
