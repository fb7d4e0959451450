"""The global bundle adjustment on the device (plslam_gba_*, K26-K39) against the numpy restatement of
levMarquardtOptimizationGBA (tests/gba_ref.py), and the device L D L^T alone (plslam_dense_ldlt_solve) against numpy."""
import math

import numpy as np
import pytest

import plslam_amd
from plslam_amd import capi, gba, synth

import gba_ref

pytestmark = pytest.mark.gpu
CAM = plslam_amd.make_cam(**{k: synth.EUROC[k] for k in ("fx", "fy", "cx", "cy", "b", "width", "height")})
EPS = np.finfo(np.float64).eps


def _plan(ctx, m):
    return plslam_amd.GbaPlan(ctx, CAM, m["n_map_kf"], m["kf_list"], m["npt"], m["nls"], m["pt_obs"], m["pt_uv"], m["ls_obs"],
                              m["ls_l"])


def _state(x_kf, Xw, Lw):
    return np.concatenate([np.asarray(x_kf).reshape(-1), np.asarray(Xw).reshape(-1), np.asarray(Lw).reshape(-1)])


def _same_nonfinite(a, b):
    return (math.isnan(a) and math.isnan(b)) or (math.isinf(a) and math.isinf(b) and (a > 0) == (b > 0)) or \
        (math.isfinite(a) and math.isfinite(b))


CASES = {
    "points": dict(n_kf=12, n_pt=300, n_ls=0),
    "lines": dict(n_kf=12, n_pt=0, n_ls=80),
    "both": dict(n_kf=12, n_pt=300, n_ls=80),
    "loop": dict(n_kf=120, n_pt=2400, n_ls=300, loop=True),
    "nkf1": dict(n_kf=2, n_pt=60, n_ls=20, obs_per_lm=2),
    "nkf37": dict(n_kf=38, n_pt=800, n_ls=120),
    "nkf101": dict(n_kf=102, n_pt=2000, n_ls=300),
    "nkf400": dict(n_kf=401, n_pt=6000, n_ls=900, loop=True),
    "singular": dict(n_kf=12, n_pt=300, n_ls=80, n_unobserved=2),
}


@pytest.mark.parametrize("name", list(CASES))
def test_optimize_equals_the_restatement(ctx, name):
    kw = dict(obs_per_lm=3, loop=False, seed=41)
    kw.update(CASES[name])
    m = gba.trajectory_map(**kw)
    assert (m["pt_obs"][:, 4] == -1).any() or (m["ls_obs"][:, 4] == -1).any()       # keyframe 0 observes something
    P = gba_ref.Problem(CAM, m)
    ref = gba_ref.gba_lm(P, m["x_kf"], m["Xw"], m["Lw"], max_iters=15)
    frac = ref["hmax"] - math.floor(ref["hmax"])
    assert 1e-6 < frac < 1 - 1e-6, "lambda_0 truncates max |H(i,i)|: the map must keep it away from an integer"
    with _closing(_plan(ctx, m)) as plan:
        _check_against(name, m, P, ref, plan)


def _check_against(name, m, P, ref, plan):
    got = plan.optimize(m["T_kf_w"], m["x_kf"], m["Xw"], m["Lw"], max_iters=15)
    assert (got["iters"], got["stop_reason"], got["n_solves"]) == (ref["iters"], ref["stop_reason"], len(ref["trace"]))
    assert math.trunc(got["hmax"]) == math.trunc(ref["hmax"])
    for t, r in zip(got["trace"], ref["trace"]):
        assert t["lam"] == r["lam"] and t["accepted"] == r["accepted"]
        assert _same_nonfinite(t["err"], r["err"]) and not math.isfinite(t["err"])
        # err and ||DX|| follow the state, whose bound is below
        assert np.isclose(t["err_raw"], r["err_raw"], rtol=1e-7), (t["err_raw"], r["err_raw"])
        assert t["n_singular"] == r["n_singular"] and t["n_bad_pivots"] == r["n_bad_pivots"] == 0
        assert np.isclose(t["dx_norm"], r["dx_norm"], rtol=1e-5), (t["dx_norm"], r["dx_norm"])
    if name == "singular":
        assert got["trace"][0]["n_singular"] == 4                        # two points and two lines without observations
    # the state after every solve: solve i of the device from the device's own state after solve i - 1 against the same solve
    # of the restatement; the bound is the forward error of a backward-stable solve with S's condition number
    prev = (m["x_kf"], m["Xw"], m["Lw"])
    for it in range(1, len(ref["trace"]) + 1):
        g = got if it == len(ref["trace"]) else plan.optimize(m["T_kf_w"], m["x_kf"], m["Xw"], m["Lw"], max_iters=it)
        x, X, L, S = gba_ref.one_step(P, it == 1, *prev, ref["trace"][it - 1]["lam"])
        cond = np.linalg.cond(np.tril(S) + np.tril(S, -1).T)
        a, b, start = _state(g["x_kf"], g["Xw"], g["Lw"]), _state(x, X, L), _state(*prev)
        bound = 1e-9 * np.abs(b).max() + 100.0 * cond * EPS * np.abs(b - start).max()
        err = np.abs(a - b).max()
        assert err <= bound, f"{name}: solve {it} differs by {err:.3e} > {bound:.3e} (cond(S) = {cond:.3e})"
        prev = (g["x_kf"], g["Xw"], g["Lw"])
    Tr = np.stack([gba_ref.expmap_se3(v) for v in got["x_kf"]])
    np.testing.assert_allclose(got["T"], Tr, rtol=0, atol=1e-12)
    # the whole trajectory against the restatement's own 15 solves: the same iterate up to the growth of rounding differences
    # through 15 relinearisations
    fin = _state(ref["x_kf"], ref["Xw"], ref["Lw"])
    assert np.abs(_state(got["x_kf"], got["Xw"], got["Lw"]) - fin).max() <= 1e-6 * np.abs(fin).max()


class _closing:
    def __init__(self, plan):
        self.plan = plan

    def __enter__(self):
        return self.plan

    def __exit__(self, *a):
        self.plan.close()


def test_two_optimize_calls_are_bit_identical(ctx):
    m = gba.trajectory_map(60, 1500, 200, obs_per_lm=4, loop=True, seed=5)
    with _closing(_plan(ctx, m)) as plan:
        a = plan.optimize(m["T_kf_w"], m["x_kf"], m["Xw"], m["Lw"])
        b = plan.optimize(m["T_kf_w"], m["x_kf"], m["Xw"], m["Lw"])
    for k in ("x_kf", "T", "Xw", "Lw"):
        assert np.array_equal(a[k], b[k]), k
    assert [tuple(t.values()) for t in a["trace"]] == [tuple(t.values()) for t in b["trace"]] or \
        all(np.array_equal(np.array(list(t.values()), float), np.array(list(u.values()), float), equal_nan=True)
            for t, u in zip(a["trace"], b["trace"]))


def test_plan_refusals(ctx):
    m = gba.trajectory_map(5, 40, 10, obs_per_lm=2, loop=False, seed=1)
    with pytest.raises(plslam_amd.PlslamError) as e:
        plslam_amd.GbaPlan(ctx, CAM, m["n_map_kf"], m["kf_list"], m["npt"], m["nls"], m["pt_obs"], m["pt_uv"], m["ls_obs"],
                           m["ls_l"], homog_th=1e-6)
    assert e.value.code == capi.EINVAL
    n = capi.GBA_MAX_KEYFRAMES + 1
    with pytest.raises(plslam_amd.PlslamError) as e:
        plslam_amd.GbaPlan(ctx, CAM, n + 1, np.arange(1, n + 1), 0, 0, np.zeros((0, 6)), np.zeros((0, 2)), np.zeros((0, 6)),
                           np.zeros((0, 3)))
    assert e.value.code == capi.EINVAL


def _sym(rng, n, spd):
    A = rng.standard_normal((n, n))
    if spd:
        return A @ A.T + n * np.eye(n)
    A = A + A.T
    return A


@pytest.mark.parametrize("n", [6, 60, 64, 65, 600, 2400])
@pytest.mark.parametrize("spd", [True, False])
def test_dense_ldlt_against_numpy(ctx, n, spd):
    rng = np.random.Generator(np.random.PCG64(n * 2 + spd))
    A = _sym(rng, n, spd)
    b = rng.standard_normal(n)
    junk = np.triu(rng.standard_normal((n, n)), 1) * 1e3      # the upper triangle is never read
    x, bad = capi.dense_ldlt_solve(ctx, np.tril(A) + junk, b)
    ref = np.linalg.solve(A, b)
    cond = np.linalg.cond(A)
    assert bad == 0
    # unpivoted L D L^T: backward stable on SPD input; on indefinite input its element growth is bounded here by n
    assert np.abs(x - ref).max() <= max(64, n) * cond * EPS * np.abs(ref).max(), (n, spd, cond)


def test_dense_ldlt_counts_a_zero_pivot(ctx):
    A = np.array([[0.0, 1.0], [1.0, 0.0]])
    _, bad = capi.dense_ldlt_solve(ctx, A, np.ones(2))
    assert bad >= 1
