"""plslam_lba_plan_optimize_dev off the runs of tests/test_gpu_lba_optimize_dev.py, whose helpers, comparisons and tolerances this
module imports unchanged.  tests/golden/lba_lm_dev_edges_golden.npz (make_lba_lm_dev_edges_golden.py) holds eleven more runs of the
reference's own text:
  * the one-workgroup solve K99 either side of 64 kB of dynamic LDS (n84 | n90) and at its last size (n120, n120_dx);
  * the padded route K100 / ldlt_enqueue / K101 running out of iterations (wide_max), leaving by the ||DX|| test (wide_dx), rejecting
    a step (wide_reject) and going on behind rejections (wide_retry);
  * the schedule lambda / k behind a rejection, the SAME err again, the retry applied, lambda * k (retry, wide_retry);
  * max_iters 0 and 2 (iters0, iters2).
Every case: against the reference (section 1), lba_loop_peek 1 against 0 and a device-built plan against a host-built one to the bit
(section 3).  Then the not-positive-definite exit on the padded route and at 6 nkf = 120 (4), the loop's count of singular
landmarks (5), and one plan called many times (6): trace capacity grown and reused, the Schur step's calls behind the loop, three
plans of two routes alive on one context.
Plan creation accepts landmarks that no observation names, so section 5 runs as planned; its comparisons are all bit for bit."""
import numpy as np
import pytest

from plslam_amd import capi
from plslam_amd.capi import LbaPlan

import test_gpu_lba_optimize_dev as B
from test_gpu_lba_optimize_dev import _bits, _problem, _run, _run_cached, _same_run

pytestmark = pytest.mark.gpu

NAMES = ("n84", "n90", "n120", "n120_dx", "wide_max", "wide_dx", "wide_reject", "wide_retry", "retry", "iters0", "iters2")
RETRY = ("retry", "wide_retry")
STATE = ("x_kf", "T", "Xw", "Lw", "slots")


# ---- 1. every case of the fixture against the reference's stored run: the comparison of the first module, as it stands ----------------
@pytest.mark.parametrize("name", NAMES)
def test_the_loop_on_the_device_equals_the_references_own_text(ctx, name):
    B._equals_the_references_own_text(ctx, "edges", name)
    got, p = _run_cached(ctx, "edges", name), _problem("edges", name)
    route = "padded" if 6 * p["nkf"] > capi.LBA_SOLVE_MAX_N6 else "one workgroup"
    print(f"{name}: 6 nkf = {6 * p['nkf']} ({route}), builds {got['n_builds']}, iters {got['iters']}, stop {got['stop_reason']}, "
          f"applied {got['applied'].tolist()}")
    assert (name.startswith("wide")) == (route == "padded")
    if name in ("iters0", "iters2"):                   # the first solve lies outside the text's loop: max_iters = 0 runs it too
        assert (got["n_builds"], got["iters"], got["stop_reason"]) == ((1, 1, 0) if name == "iters0" else (2, 2, 0))
    if name.endswith("_dx"):                           # the ||DX|| test: the last build's solve ran, iters and err_prev stay
        assert got["stop_reason"] == 2 and got["applied"][-1] == 1 and got["iters"] == got["n_builds"] - 1
        assert 0 < got["dx_norm"][-1] < p["prm"]["min_error_change"]


# ---- 2. rejection and retry: lambda / k, the same err, the retry applied, lambda * k ---------------------------------------------------
@pytest.mark.parametrize("name", RETRY)
def test_a_retry_behind_a_rejection_follows_the_schedule(ctx, name):
    p, got = _problem("edges", name), _run_cached(ctx, "edges", name)
    k, applied, lam, err = p["prm"]["lambda_k"], got["applied"], got["lam"], got["err"]
    assert p["prm"]["min_error_change"] == 0.0 and got["stop_reason"] == 0 and (applied >= 0).all()
    rejected = np.flatnonzero(applied == 0)
    rejected = rejected[rejected + 1 < len(applied)]
    assert len(rejected) >= 4
    for r in rejected:
        assert _bits(err[r + 1:r + 2])[0] == _bits(err[r:r + 1])[0], r       # the state it had: the err it had, to the bit
        assert _bits(got["err_raw"][r + 1:r + 2])[0] == _bits(got["err_raw"][r:r + 1])[0], r
        assert applied[r + 1] == 1 and lam[r + 1] == lam[r] / k, r
    for i in range(1, len(applied) - 1):
        if applied[i] == 1:
            assert lam[i + 1] == lam[i] * k, i
    assert got["lam_last"] == (lam[-1] * k if applied[-1] == 1 else lam[-1] / k)


def _cut(ctx, name, max_iters):
    key = ("cut", name, max_iters)
    if key not in B._cache:
        B._cache[key] = _run(ctx, _problem("edges", name), max_iters=max_iters)
    return B._cache[key]


@pytest.mark.parametrize("name", RETRY + ("wide_reject",))
def test_every_rejected_step_leaves_landmarks_and_poses_untouched(ctx, name):
    """tests/test_gpu_lba_optimize_dev.py's rejected-step test at every rejection of the run, on both routes"""
    p, full = _problem("edges", name), _run_cached(ctx, "edges", name)
    solved = full["applied"][full["applied"] >= 0]
    rejected = np.flatnonzero(solved == 0)
    assert len(rejected) >= 1 and rejected[0] >= 2
    for r in (int(v) for v in rejected):
        before, after = _cut(ctx, name, r), _cut(ctx, name, r + 1)     # builds 0 .. r - 1 | ... and build r, whose step is rejected
        assert before["n_builds"] == r and after["n_builds"] == r + 1 and after["applied"].tolist() == solved[:r + 1].tolist()
        assert before["stop_reason"] == after["stop_reason"] == 0
        for key in STATE:
            assert np.array_equal(_bits(before[key]), _bits(after[key])), (r, key)
        assert after["lam_last"] == after["lam"][-1] / p["prm"]["lambda_k"] and after["dx_norm"][-1] > 0
        assert after["err_prev"] == after["err"][-1]
        if r + 2 <= len(solved) and name in RETRY:     # ... and the retry behind it moves them
            moved = _cut(ctx, name, r + 2)
            assert moved["applied"].tolist() == solved[:r + 2].tolist() and moved["applied"][-1] == 1
            assert not np.array_equal(_bits(moved["x_kf"]), _bits(after["x_kf"])) and not np.array_equal(_bits(moved["Xw"]), _bits(after["Xw"]))


# ---- 3. predication: passes (and the padded route's unpredicated factorisations) behind the stop change nothing ------------------------
@pytest.mark.parametrize("name", NAMES)
def test_passes_behind_the_stop_change_nothing(ctx, name):
    p = _problem("edges", name)
    a, b = _run_cached(ctx, "edges", name, 1), _run_cached(ctx, "edges", name, 0)
    _same_run(a, b, "lba_loop_peek 1 against 0")
    assert b["n_enqueued_passes"] == max(p["prm"]["max_iters"], 1)
    assert a["n_builds"] <= a["n_enqueued_passes"] <= b["n_enqueued_passes"]
    if name in ("wide_dx", "wide_reject", "n120_dx"):
        assert b["n_enqueued_passes"] - b["n_builds"] >= 10
    print(f"{name}: builds {a['n_builds']}, enqueued with the peek {a['n_enqueued_passes']}, without {b['n_enqueued_passes']}")


@pytest.mark.parametrize("name", NAMES)
def test_a_device_built_plan_gives_the_host_built_plans_bits(ctx, name):
    p = _problem("edges", name)
    for peek in (1, 0):
        _same_run(_run_cached(ctx, "edges", name, peek), _run(ctx, p, peek, make=B._dev_plan), f"plslam_lba_plan_create_dev, peek {peek}")


# ---- 4. not positive definite: an optimised key frame that no observation names ----------------------------------------------------------
def _with_an_empty_keyframe(which, name):
    """the problem with one more optimised key frame, which no observation names (the construction of the first module's test)"""
    p = _problem(which, name)
    p["nkf"] += 1
    p["T"] = np.concatenate([p["T"], p["T"][:1]])
    p["x_kf"] = np.concatenate([p["x_kf"], np.full((1, 6), 0.01)])
    return p


def _last_keyframe_emptied(which, name):
    """the problem with every observation by its last optimised key frame taken out: the same nkf, one key frame empty"""
    p = _problem(which, name)
    c, last = p["cols"], p["nkf"] - 1
    kp, kl = c["pt_kf_loc"] != last, c["ls_kf_loc"] != last
    assert 0 < (~kp).sum() and 0 < (~kl).sum()
    assert np.bincount(c["pt_lm"][kp], minlength=p["npt"]).min() >= 2 and np.bincount(c["ls_lm"][kl], minlength=p["nls"]).min() >= 2
    p["cols"] = dict({k: np.ascontiguousarray(v[kp]) for k, v in c.items() if k.startswith("pt_")},
                     **{k: np.ascontiguousarray(v[kl]) for k, v in c.items() if k.startswith("ls_")})
    return p


@pytest.mark.parametrize("route", ["padded_132", "one_workgroup_120"])
def test_a_keyframe_without_observations_ends_the_loop_not_positive_definite(ctx, route):
    p = _with_an_empty_keyframe("dev", "wide") if route == "padded_132" else _last_keyframe_emptied("edges", "n120")
    assert 6 * p["nkf"] == (132 if route == "padded_132" else capi.LBA_SOLVE_MAX_N6)
    got = _run(ctx, p)
    assert got["stop_reason"] == capi.LBA_STOP_NOT_PD and got["iters"] == 0 and got["n_builds"] == 1
    assert got["applied"].tolist() == [0] and got["n_bad_pivots"][0] >= 1 and got["lam"][0] > 0 and np.isinf(got["err"][0])
    assert np.array_equal(_bits(got["x_kf"]), _bits(p["x_kf"])) and np.array_equal(_bits(got["Xw"]), _bits(p["Xw"]))
    assert np.array_equal(_bits(got["Lw"]), _bits(p["Lw"]))
    assert np.array_equal(_bits(got["slots"].reshape(-1, 16)), _bits(p["T"]))
    from oracle import oracle as O
    for kf in range(p["nkf"]):
        assert np.allclose(got["T"][kf], O.expmap_se3(p["x_kf"][kf]).reshape(4, 4), rtol=0, atol=1e-12)
    _same_run(got, _run(ctx, p, 0), "not positive definite, lba_loop_peek 0")


# ---- 5. singular landmarks counted in the loop -----------------------------------------------------------------------------------------
SINGULAR = dict(max_iters=4, min_error_change=0.0, min_error=0.0)     # every decision compares two errs: Npt + Nls cancels


def _with_unobserved_landmarks(p, n_pt=3, n_ls=2):
    q = dict(p)
    rng = np.random.Generator(np.random.PCG64(7))
    q["Xw"] = np.concatenate([p["Xw"], 5.0 + rng.standard_normal((n_pt, 3))])
    q["Lw"] = np.concatenate([p["Lw"], 5.0 + rng.standard_normal((n_ls, 6))])
    q["npt"], q["nls"] = p["npt"] + n_pt, p["nls"] + n_ls
    return q


def test_landmarks_without_observations_are_counted_and_change_nothing(ctx):
    p = _problem("lm", "main")
    q = _with_unobserved_landmarks(p)
    a, b = _run(ctx, p, **SINGULAR), _run(ctx, q, **SINGULAR)
    assert a["n_builds"] == b["n_builds"] == 4 and a["stop_reason"] == b["stop_reason"] == 0 and a["applied"].tolist() == [1, 1, 1, 1]
    assert (a["n_singular"] == 0).all() and b["n_singular"].tolist() == [5, 5, 5, 5]
    for k in ("err_raw", "lam", "applied", "x_kf", "T", "n_bad_pivots"):
        assert np.array_equal(_bits(a[k]), _bits(b[k])), k
    assert a["hmax"] == b["hmax"] and a["lam_last"] == b["lam_last"] and a["iters"] == b["iters"] == 4
    npt, nls = p["npt"], p["nls"]
    assert np.array_equal(_bits(b["Xw"][:npt]), _bits(a["Xw"])) and np.array_equal(_bits(b["Lw"][:nls]), _bits(a["Lw"]))
    assert np.array_equal(_bits(b["Xw"][npt:]), _bits(q["Xw"][npt:])) and np.array_equal(_bits(b["Lw"][nls:]), _bits(q["Lw"][nls:]))
    assert not np.array_equal(_bits(a["Xw"]), _bits(p["Xw"]))              # not vacuous: the observed ones moved
    # err is the same sum over another count of landmarks
    assert np.array_equal(b["err"][1:], b["err_raw"][1:] / (npt + nls + 5)) and np.array_equal(a["err"][1:], a["err_raw"][1:] / (npt + nls))
    _same_run(b, _run(ctx, q, 0, **SINGULAR), "unobserved landmarks, lba_loop_peek 0")
    _same_run(b, _run(ctx, q, 1, make=B._dev_plan, **SINGULAR), "unobserved landmarks, a device-built plan")


# ---- 6. one plan, many calls -----------------------------------------------------------------------------------------------------------
def _call(ctx, plan, p, **over):
    out = plan.optimize_dev(p["T"], p["x_kf"], p["n_map"], **dict(p["prm"], **over))
    out["Xw"], out["Lw"] = plan.get_landmarks()
    out["slots"] = B._slots(ctx, plan)
    return out


def _start_again(plan, p):
    plan.iterate_dev(p["T"], p["Xw"], p["Lw"], want_g=False)


def test_repeated_calls_on_one_plan_equal_fresh_plans(ctx):
    """3 records, then 15 (the trace capacity grows, and the image's layout with it), then 3 again on the larger capacity"""
    p = _problem("lm", "main")
    fresh3, fresh15 = _run_cached(ctx, "dev", "main_3"), _run_cached(ctx, "lm", "main")
    assert fresh3["n_builds"] == 3 and fresh15["n_builds"] > 3
    plan = B._host_plan(ctx, p)
    first = _call(ctx, plan, p, max_iters=3)
    _start_again(plan, p)
    second = _call(ctx, plan, p, max_iters=15)
    _start_again(plan, p)
    third = _call(ctx, plan, p, max_iters=3)
    plan.close()
    _same_run(first, fresh3, "the first call of the plan")
    _same_run(second, fresh15, "the second call: more records than the plan had room for")
    _same_run(third, fresh3, "the third call: fewer records than the plan has room for")
    _same_run(third, first, "the third call against the first")
    assert len(first["lam"]) == len(third["lam"]) == 3 and len(second["lam"]) == fresh15["n_builds"]


def _schur_step(plan, lam, dp=None):
    err, S, b, ns = plan.iterate_schur(lam)
    if dp is None:
        dp = np.linalg.solve(S, b)
    ss = plan.apply_step(dp)
    return dict(err=np.array([err]), S=S, b=b, ns=np.array([ns]), ss=np.array([ss]), dp=dp)


@pytest.mark.parametrize("how", ["stopped_with_empty_passes_behind", "ran_out"])
def test_the_schur_steps_calls_behind_the_loop_equal_a_fresh_plans(ctx, how):
    """the loop leaves no parity, counter or flag behind: five landmarks without observations make both counters of singular landmarks
    non-zero during the loop, so one left uncleared shows in the count the next call returns"""
    p = _with_unobserved_landmarks(_problem("lm", "main"))
    over = dict(min_error_change=1.0) if how.startswith("stopped") else dict(max_iters=3)
    ctx.set_option("lba_loop_peek", 0)
    try:
        plan = B._host_plan(ctx, p)
        out = _call(ctx, plan, p, **over)
    finally:
        ctx.set_option("lba_loop_peek", 1)
    if how.startswith("stopped"):
        assert out["stop_reason"] == 2 and out["n_builds"] == 2 and out["n_enqueued_passes"] == 15
    else:
        assert out["stop_reason"] == 0 and out["n_builds"] == out["n_enqueued_passes"] == 3
    assert (out["n_singular"] == 5).all()
    lam = out["lam_last"]
    a = _schur_step(plan, lam)
    a["Xw"], a["Lw"] = plan.get_landmarks()
    a["slots"] = B._slots(ctx, plan)
    plan.close()
    c = p["cols"]
    fresh = LbaPlan(ctx, B._cam(), p["th"], p["n_map"] + p["nkf"], p["nkf"], p["npt"], p["nls"], c["pt_lm"], c["pt_slot"], c["pt_kf_loc"],
                    c["pt_obs_uv"], c["ls_lm"], c["ls_slot"], c["ls_kf_loc"], c["ls_l_obs"])
    fresh.iterate_dev(out["slots"].reshape(-1, 16), out["Xw"], out["Lw"], want_g=False)
    b = _schur_step(fresh, lam, a["dp"])
    b["Xw"], b["Lw"] = fresh.get_landmarks()
    b["slots"] = B._slots(ctx, fresh)
    fresh.close()
    assert a["ns"][0] == 5 and np.isfinite(a["dp"]).all() and a["ss"][0] > 0
    for k in ("err", "S", "b", "ns", "ss", "Xw", "Lw", "slots"):
        assert np.array_equal(_bits(a[k]), _bits(b[k])), k
    assert np.array_equal(_bits(a["slots"]), _bits(out["slots"])) and not np.array_equal(_bits(a["Xw"]), _bits(out["Xw"]))


def test_three_plans_of_two_routes_alive_on_one_context(ctx):
    """wide (padded), n120 (one workgroup, the attribute raised by a plan that is not the first), main: interleaved"""
    cases = {"wide": ("dev", "wide"), "n120": ("edges", "n120"), "main": ("lm", "main")}
    probs = {k: _problem(*v) for k, v in cases.items()}
    fresh = {k: _run_cached(ctx, *v) for k, v in cases.items()}
    plans = {k: B._host_plan(ctx, probs[k]) for k in ("wide", "n120", "main")}
    called = set()
    try:
        for k in ("wide", "n120", "main", "n120", "wide"):
            if k in called:
                _start_again(plans[k], probs[k])
            _same_run(_call(ctx, plans[k], probs[k]), fresh[k], f"{k}, {'again' if k in called else 'first'}")
            called.add(k)
    finally:
        for q in plans.values():
            q.close()
