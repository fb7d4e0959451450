"""The global bundle adjustment on the device (plslam_gba_*, K26-K39) against the numpy restatement of
levMarquardtOptimizationGBA (tests/gba_ref.py), and the device L D L^T alone (plslam_dense_ldlt_solve) against numpy."""
import math

import numpy as np
import pytest

import plslam_amd
from plslam_amd import capi, gba, synth

import gba_cases
import gba_dense
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


def _map(name):
    if name in CASES:
        return gba.trajectory_map(**dict(dict(obs_per_lm=3, loop=False, seed=41), **CASES[name]))
    return (gba_cases.INPUTS.get(name) or gba_cases.DEGENERATE[name])()


@pytest.mark.parametrize("name", list(CASES) + list(gba_cases.INPUTS))
def test_optimize_equals_the_restatement(ctx, name):
    m = _map(name)
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


# PCG64(2 n + spd) draws an indefinite 33 x 33 that meets a pivot of 2.6e-3: |L| up to 1e4, rho = 1.1e5, and numpy's own
# unpivoted factorisation of it misses the bound tenfold.  That matrix tests the draw, not the tiling; another seed gives n = 33
# a matrix with the growth of its neighbours (rho = 90; 94 at n = 31, 76 at n = 32)
LDLT_SEED = {(33, False): 1003}


def _growth(A):
    n = A.shape[0]
    M, L, d = A.copy(), np.eye(n), np.zeros(n)
    for j in range(n):
        d[j] = M[j, j]
        L[j + 1:, j] = M[j + 1:, j] / d[j]
        M[j + 1:, j + 1:] -= np.outer(L[j + 1:, j], L[j + 1:, j] * d[j])
    return (np.abs(L) * np.abs(d) @ np.abs(L).T).max() / np.abs(A).max()


@pytest.mark.parametrize("n", [6, 31, 32, 33, 60, 64, 65, 95, 96, 97, 600, 2400])
@pytest.mark.parametrize("spd", [True, False])
def test_dense_ldlt_against_numpy(ctx, n, spd):
    """Sizes on both sides of one and of three 32-wide tiles included.  The largest order the entry point takes, 6 * 4096
    (a 4.8 GB matrix), stays untested."""
    rng = np.random.Generator(np.random.PCG64(LDLT_SEED.get((n, spd), n * 2 + spd)))
    A = _sym(rng, n, spd)
    b = rng.standard_normal(n)
    junk = np.triu(rng.standard_normal((n, n)), 1) * 1e3      # the upper triangle is never read
    x, bad = capi.dense_ldlt_solve(ctx, np.tril(A) + junk, b)
    ref = np.linalg.solve(A, b)
    cond = np.linalg.cond(A)
    assert bad == 0
    # unpivoted L D L^T: backward stable on SPD input (|L| |D| |L^T| <= |A| there); on indefinite input only as far as the
    # element growth rho = max(|L| |D| |L^T|) / max|A| stays moderate, which is a property of the draw: below 2.1e3 for every
    # indefinite matrix here up to n = 97 (asserted; 3.3e4 at n = 600)
    if n < 100:
        assert _growth(A) < (2.0 if spd else 1e4)
    bound = max(64, n) * cond * EPS * np.abs(ref).max()
    assert np.abs(x - ref).max() <= bound, (n, spd, cond)


def test_dense_ldlt_counts_a_zero_pivot(ctx):
    A = np.array([[0.0, 1.0], [1.0, 0.0]])
    _, bad = capi.dense_ldlt_solve(ctx, A, np.ones(2))
    assert bad >= 1


def test_dense_ldlt_counts_the_pivots_of_the_system_only(ctx):
    """A 70 x 70 matrix (padded to 96 on the device) with an exact zero pivot at index 40, and one with a NaN at (50, 50):
    every later pivot is non-finite, the 26 of the identity padding too -- those are not pivots of the system and are not
    counted, so the count is the unpadded restatement's."""
    n = 70
    rng = np.random.Generator(np.random.PCG64(70))
    L = np.tril(rng.integers(-1, 2, (n, n)).astype(np.float64), -1) * (rng.uniform(0, 1, (n, n)) < 0.2) + np.eye(n)
    d = rng.integers(1, 4, n).astype(np.float64)
    d[40] = 0.0
    A = (L * d) @ L.T                                   # small integers: the elimination is exact and meets d[40] = 0
    b = rng.standard_normal(n)
    with np.errstate(all="ignore"):
        _, bad_ref = gba_ref.ldlt_solve(A, b)
    assert bad_ref == 30
    assert capi.dense_ldlt_solve(ctx, A, b)[1] == bad_ref
    A = _sym(rng, n, True)
    A[50, 50] = np.nan
    with np.errstate(all="ignore"):
        _, bad_ref = gba_ref.ldlt_solve(A, b)
    assert bad_ref == 20
    assert capi.dense_ldlt_solve(ctx, A, b)[1] == bad_ref


def _pose_step_ld(x0, dp):
    """K38's update in long double, by the full formulas"""
    return gba_dense.logmap_ld(gba_dense.expmap_ld(x0) @ gba_dense.inverse_ld(gba_dense.expmap_ld(dp))).astype(np.float64)


@pytest.mark.parametrize("name", list(gba_cases.SMALL))
def test_first_solve_equals_a_long_double_elimination_of_the_whole_system(ctx, name):
    """The one place where the device meets something that is not its restatement: the state after one applied solve against
    Gaussian elimination of the whole damped system in long double (no Schur complement, no L D L^T, no blocks), the pose
    update by the full SE(3) formulas.  Only the first pass's H and g come from gba_ref (pinned to the reference's own loops
    in test_gba_cpu.py).  The bound is _check_against's forward-error form with the condition number of the full damped H;
    two of tumbling's keyframes take expmap_se3's small-angle branch, whose truncation (|w| <= 1e-6 per entry of x, times
    (1 + |t|_1) for the translation part) is added for them."""
    m = gba_cases.SMALL[name]()
    P = gba_ref.Problem(CAM, m)
    B = P.blocks(True, m["x_kf"], m["Xw"], m["Lw"])
    with _closing(_plan(ctx, m)) as plan:
        got = plan.optimize(m["T_kf_w"], m["x_kf"], m["Xw"], m["Lw"], max_iters=1)
    lam = got["trace"][0]["lam"]
    assert lam == 1e-5 * math.trunc(np.abs(np.diag(P.full_H(B)[0])).max())
    Hd, g = gba_dense.damped_system(P, B, lam)
    sol = gba_dense.solve_long_double(Hd, g)
    n6 = 6 * P.nkf
    x = np.stack([_pose_step_ld(x0, dp) for x0, dp in zip(m["x_kf"], sol[:n6].reshape(-1, 6))])
    X = m["Xw"] + sol[n6:n6 + 3 * P.npt].astype(np.float64).reshape(-1, 3)
    Lw = m["Lw"] + sol[n6 + 3 * P.npt:].astype(np.float64).reshape(-1, 6)
    a, b, start = _state(got["x_kf"], got["Xw"], got["Lw"]), _state(x, X, Lw), _state(m["x_kf"], m["Xw"], m["Lw"])
    cond = np.linalg.cond(Hd)
    assert 100.0 * cond * EPS <= 1e-2            # the bound stays below a hundredth of the largest step
    bound = np.full(a.shape, 1e-9 * np.abs(b).max() + 100.0 * cond * EPS * np.abs(b - start).max())
    for k in np.flatnonzero(np.linalg.norm(m["x_kf"][:, 3:], axis=1) < 1e-6):
        bound[6 * k:6 * k + 6] += 1e-6 * (1.0 + np.abs(m["x_kf"][k, :3]).sum())
    err = np.abs(a - b)
    assert (err <= bound).all(), f"{name}: {err.max():.3e} > {bound.min():.3e} (cond(H) = {cond:.3e})"
    assert got["trace"][0]["n_singular"] == 0 and got["trace"][0]["n_bad_pivots"] == 0


def test_first_solve_turns_with_the_world_frame(ctx):
    """ragged's points seen from a world frame turned by a quarter about x and moved: after one solve the landmarks are the
    turned landmarks and the poses relative to the frame are the same.  tests/test_gba_cpu.py shows from the restatement where
    this holds: Marquardt's lambda diag(H) turns with the frame only under a signed permutation of the axes, and the first
    pass's transposed pose x line blocks do not turn at all, hence the quarter turn and the points.  Tolerance: the case's
    _check_against bound, twice -- each run carries it."""
    m = gba_cases.points_only(gba_cases.ragged())
    G = gba_cases.QUARTER_TURN
    got = []
    for mm in (m, gba_cases.world_transform(m, G)):
        with _closing(_plan(ctx, mm)) as plan:
            got.append(plan.optimize(mm["T_kf_w"], mm["x_kf"], mm["Xw"], mm["Lw"], max_iters=1))
    assert got[0]["trace"][0]["lam"] == got[1]["trace"][0]["lam"]
    x, X, L, S = gba_ref.one_step(gba_ref.Problem(CAM, m), True, m["x_kf"], m["Xw"], m["Lw"], got[0]["trace"][0]["lam"])
    cond = np.linalg.cond(np.tril(S) + np.tril(S, -1).T)
    b, start = _state(x, X, L), _state(m["x_kf"], m["Xw"], m["Lw"])
    bound = 1e-9 * np.abs(b).max() + 100.0 * cond * EPS * np.abs(b - start).max()
    a = _state(got[0]["x_kf"], got[0]["Xw"], got[0]["Lw"])
    back = _state(*gba_cases.moved(gba_ref.inverse_se3(G), got[1]["x_kf"], got[1]["Xw"], got[1]["Lw"]))
    err = np.abs(back - a).max()
    print(f"frame invariance: {err:.3e} against 2 x {bound:.3e}; largest step {np.abs(a - start).max():.3e}")
    assert err <= 2 * bound, (err, bound)
    assert np.abs(a - start).max() > 1e6 * bound                      # the steps that turn are not small ones
    # the poses themselves, not only their logarithms: T' = G T
    Tb = np.stack([G @ T.reshape(4, 4) for T in got[0]["T"]]).reshape(got[1]["T"].shape)
    assert np.abs(Tb - got[1]["T"]).max() <= 2 * bound


def test_the_loop_stops_on_the_step_norm(ctx):
    """PLSLAM_GBA_STOP_DX: tests/test_gba_cpu.py shows that no solve's ||DX|| lies within a factor of 2 of eps"""
    name, iters = gba_cases.STOP_DX_CASE, gba_cases.STOP_DX_ITERS
    m = _map(name)
    ref = gba_ref.gba_lm(gba_ref.Problem(CAM, m), m["x_kf"], m["Xw"], m["Lw"], max_iters=iters)
    assert ref["stop_reason"] == 2
    with _closing(_plan(ctx, m)) as plan:
        got = plan.optimize(m["T_kf_w"], m["x_kf"], m["Xw"], m["Lw"], max_iters=iters)
    assert (got["stop_reason"], got["iters"], got["n_solves"]) == (capi.GBA_STOP_DX, ref["iters"], len(ref["trace"]))
    assert [t["lam"] for t in got["trace"]] == [t["lam"] for t in ref["trace"]] and got["lam"] == ref["lam"]
    for t, r in zip(got["trace"], ref["trace"]):
        assert np.isclose(t["dx_norm"], r["dx_norm"], rtol=1e-5)


def test_heavily_damped_steps_keep_the_small_angle_keyframes_small(ctx):
    """tumbling under lambda_lm = 1e3: no step reaches 1e-6, so the keyframes with w = 0 and |w| = 5e-7 take the small-angle
    branch of expmap_se3 and of logmap_se3 in every solve, and |w| = 2e-6 the full one (test_gba_cpu.py counts them)."""
    m = gba_cases.tumbling()
    P = gba_ref.Problem(CAM, m)
    n, lam = gba_cases.DAMPED_ITERS, gba_cases.DAMPED_LAMBDA
    ref = gba_ref.gba_lm(P, m["x_kf"], m["Xw"], m["Lw"], max_iters=n, lambda_lm=lam)
    with _closing(_plan(ctx, m)) as plan:
        got = plan.optimize(m["T_kf_w"], m["x_kf"], m["Xw"], m["Lw"], max_iters=n, lambda_lm=lam)
    assert got["n_solves"] == n == 4 and [t["lam"] for t in got["trace"]] == [t["lam"] for t in ref["trace"]]
    a, b = _state(got["x_kf"], got["Xw"], got["Lw"]), _state(ref["x_kf"], ref["Xw"], ref["Lw"])
    start = _state(m["x_kf"], m["Xw"], m["Lw"])
    cond = max(np.linalg.cond(np.tril(t["S"]) + np.tril(t["S"], -1).T) for t in ref["trace"])
    # four solves, each to the forward-error form of _check_against, its absolute term the rounding of K38's round trip
    # logmap_se3(expmap_se3(x)): 16 eps times |V^-1| <= 4 (test_se3_maps_against_the_full_formulas_in_long_double)
    assert np.abs(b - start).max() < 1e-6
    assert np.abs(a - b).max() <= 4 * (64 * EPS * np.abs(b).max() + 100.0 * cond * EPS * np.abs(b - start).max())
    assert np.array_equal(got["x_kf"][0, 3:], np.zeros(3)) and np.array_equal(got["x_kf"][1, 3:], np.zeros(3))
    assert abs(np.linalg.norm(got["x_kf"][2, 3:]) - 2e-6) < 1e-9
    np.testing.assert_allclose(got["T"], np.stack([gba_ref.expmap_se3(v) for v in got["x_kf"]]), rtol=0, atol=1e-12)


def test_gaps_in_the_slot_numbering_change_nothing(ctx):
    """gaps against the same map with its slots packed: only slot numbers differ, so every bit of the result is the same; the
    returned T rows are expmap_se3 of the returned x_kf in kf_list order."""
    m = gba_cases.gaps()
    r = gba_cases.renumbered(m)
    out = []
    for mm in (m, r):
        with _closing(_plan(ctx, mm)) as plan:
            out.append(plan.optimize(mm["T_kf_w"], mm["x_kf"], mm["Xw"], mm["Lw"]))
    for k in ("x_kf", "T", "Xw", "Lw"):
        assert np.isfinite(out[0][k]).all() and np.array_equal(out[0][k], out[1][k]), k
    assert [tuple(t.values()) for t in out[0]["trace"]] == [tuple(t.values()) for t in out[1]["trace"]]
    np.testing.assert_allclose(out[0]["T"], np.stack([gba_ref.expmap_se3(v) for v in out[0]["x_kf"]]), rtol=0, atol=1e-12)


@pytest.mark.parametrize("name", list(gba_cases.DEGENERATE))
def test_degenerate_inputs_count_and_poison_as_the_restatement(ctx, name):
    """NaN arithmetic, no bad address.  n_singular and n_bad_pivots solve by solve, trunc(hmax) despite NaN diagonals (K26),
    the set of unknowns that are still finite after every number of solves, and the usual bound where both are finite.
    no_obs_keyframe and nan_landmark have 6 nkf = 96, a multiple of the tile: a non-finite pivot also turns the identity
    padding behind it non-finite, which the device does not count (test_dense_ldlt_counts_the_pivots_of_the_system_only).
    The device multiplies through zeros (0 * NaN = NaN) in its triangular solves, as the restatement's numpy products do, and
    K38 turns a NaN step into the pose (NaN, NaN, NaN, 0, 0, 0): logmap_se3's clamps are comparisons, which a NaN passes, so
    w keeps its zeros (gba_ref.logmap_se3 restates exactly that, pinned in test_gba_cpu.py).  With that the poisoned sets
    agree and nothing is pinned beyond the header.
    The bound: no_point_obs never meets a bad pivot and goes through _check_against whole, the usual bound at every solve.
    Behind a bad pivot S is singular or holds NaN: its condition number is infinite or undefined, and every unknown that
    passes through S is NaN on both sides.  What stays finite does not depend on S at all: the points that only the fixed
    keyframe sees (X += V g, a damped 3 x 3 block of its own, well conditioned by lambda diag) and the zero rotation parts.
    After the first solve they get the usual form without S's condition number, 1e-9 max|b| + 100 eps max|step|; after 2 and
    15 solves, where each side has relinearised from its own state, _check_against's whole-trajectory bound, 1e-6 relative."""
    m = _map(name)
    P = gba_ref.Problem(CAM, m)
    with np.errstate(all="ignore"):
        ref = gba_ref.gba_lm(P, m["x_kf"], m["Xw"], m["Lw"], max_iters=15)
    with _closing(_plan(ctx, m)) as plan:
        got = plan.optimize(m["T_kf_w"], m["x_kf"], m["Xw"], m["Lw"], max_iters=15)
        assert (got["iters"], got["stop_reason"], got["n_solves"]) == (ref["iters"], ref["stop_reason"], len(ref["trace"]))
        assert math.trunc(got["hmax"]) == math.trunc(ref["hmax"]) > 0
        for t, r in zip(got["trace"], ref["trace"]):
            assert (t["n_singular"], t["n_bad_pivots"], t["accepted"]) == (r["n_singular"], r["n_bad_pivots"], r["accepted"])
            assert t["lam"] == r["lam"] and _same_nonfinite(t["dx_norm"], r["dx_norm"]) and _same_nonfinite(t["err_raw"], r["err_raw"])
        if name == "no_obs_keyframe":
            assert got["trace"][0]["n_bad_pivots"] == 6
        prev = (m["x_kf"], m["Xw"], m["Lw"])
        for it in (1, 2, 15):
            g = got if it == 15 else plan.optimize(m["T_kf_w"], m["x_kf"], m["Xw"], m["Lw"], max_iters=it)
            r = ref["trace"][it - 1]
            a, b = _state(g["x_kf"], g["Xw"], g["Lw"]), _state(r["x_kf"], r["Xw"], r["Lw"])
            assert np.array_equal(np.isfinite(a), np.isfinite(b)), (name, it, np.flatnonzero(np.isfinite(a)), np.flatnonzero(np.isfinite(b)))
            fin = np.isfinite(b)
            if it == 1 and fin.any():
                S = r["S"]
                cond = np.linalg.cond(np.tril(S) + np.tril(S, -1).T) if r["n_bad_pivots"] == 0 else 1.0
                assert math.isfinite(cond)
                start = _state(*prev)
                bound = 1e-9 * np.abs(b[fin]).max() + 100.0 * cond * EPS * np.abs(b - start)[fin].max()
                assert np.abs(a - b)[fin].max() <= bound
            elif fin.any():
                assert np.abs(a - b)[fin].max() <= 1e-6 * np.abs(b[fin]).max()
        if name == "no_point_obs":
            assert all(np.isfinite(r["S"]).all() for r in ref["trace"]) and np.isfinite(a).all()
            _check_against(name, m, P, ref, plan)
        else:
            assert not np.isfinite(a).all()
    assert np.isfinite(a).any()
