"""tests/golden/lba_lm_dev_edges_golden.npz (make_lba_lm_dev_edges_golden.py) is what its cases are named for -- from the fixture
alone, no GPU, no oracle: the number of key frames and so the route of the solve (one workgroup up to 6 nkf = 120 -- above 64 kB of
dynamic LDS from nkf = 15 --, the padded copy above it), the stop, the applied / rejected pattern, the counts of points and lines,
and that every recorded decision keeps the generator's distance of 1e-6 from its threshold -- but for the equal errs behind a
rejection, which have to be EQUAL."""
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
SOLVE_MAX_N6 = 120                                       # plslam_amd/csrc/lba_lm_dev.hip: LM_SOLVE_MAX_N6
GAP = 1e-6
MEC_DEFAULT = 1e-7

# name -> nkf, the route, stop, the applied pattern (None: see the test), points, lines, observations per landmark
WANT = {
    "n84": (14, "lds_below_64k", 1, [1, 1, 1, 1], 150, 40, 6),
    "n90": (15, "lds_above_64k", 1, [1, 1, 1, 1, 1], 150, 40, 6),
    "n120": (20, "lds_above_64k", 0, [1, 1, 1], 150, 40, 6),
    "n120_dx": (20, "lds_above_64k", 2, [1, 1], 150, 40, 6),
    "wide_max": (21, "padded", 0, [1, 1, 1], 150, 40, 6),
    "wide_dx": (21, "padded", 2, [1, 1], 150, 40, 6),
    "wide_reject": (21, "padded", 1, [1, 1, 0], 120, 40, 3),
    "wide_retry": (21, "padded", 0, None, 120, 40, 3),
    "retry": (4, "lds_below_64k", 0, None, 120, 40, 3),
    "iters0": (6, "lds_below_64k", 0, [1], 400, 120, 4),
    "iters2": (6, "lds_below_64k", 0, [1, 1], 400, 120, 4),
}
SAME_PROBLEM = [("n120_dx", "n120"), ("wide_dx", "wide_max"), ("wide_retry", "wide_reject"), ("iters2", "iters0")]
_files = {}


def _npz(fixture="lba_lm_dev_edges_golden.npz"):
    if fixture not in _files:
        _files[fixture] = dict(np.load(os.path.join(GOLDEN, fixture)))
    return _files[fixture]


def _where(name):
    """(arrays, case) that hold the problem of `name`"""
    g = _npz()
    if f"{name}_problem" not in g:
        return g, name
    fixture, case = str(g[f"{name}_problem"]).split(":")
    assert f"{case}_problem" not in _npz(fixture)         # one step, no chains
    return _npz(fixture), case


def _lds_bytes(n6):
    return (n6 * (n6 + 1) + n6) * 8                      # lm_solve_lds_bytes: S with a row stride of n6 + 1, and the right-hand side


def test_the_fixture_holds_exactly_the_named_cases():
    g = _npz()
    assert sorted(k[:-4] for k in g if k.endswith("_cfg")) == sorted(WANT)
    assert os.path.getsize(os.path.join(GOLDEN, "lba_lm_dev_edges_golden.npz")) < os.path.getsize(os.path.join(GOLDEN, "lba_lm_dev_golden.npz"))
    assert (_lds_bytes(84), _lds_bytes(90), _lds_bytes(120)) == (57792, 66240, 117120) and _lds_bytes(84) < 65536 < _lds_bytes(90)


@pytest.mark.parametrize("name", sorted(WANT))
def test_a_case_is_what_it_is_named_for(name):
    g = _npz()
    nkf, route, stop, applied, npt, nls, obs = WANT[name]
    src, case = _where(name)
    a = lambda k: src[f"{case}_{k}"]                                             # noqa: E731
    cfg = g[f"{name}_cfg"]
    max_iters, mec, me = int(cfg[3]), float(cfg[4]), float(cfg[5])
    # ---- the problem ----
    assert int(a("nkf")) == nkf and int(a("n_kf_map")) == nkf + 1 and a("T_map").reshape(-1, 16).shape[0] == nkf + 1
    n6 = 6 * nkf
    got_route = "padded" if n6 > SOLVE_MAX_N6 else "lds_above_64k" if _lds_bytes(n6) > 65536 else "lds_below_64k"
    assert got_route == route
    assert a("Xw").reshape(-1, 3).shape[0] == npt and a("Lw").reshape(-1, 6).shape[0] == nls
    assert a("pt_lm").size == npt * obs and a("ls_lm").size == nls * obs and a("pt_uv").size == 2 * npt * obs and a("ls_l").size == 3 * nls * obs
    assert np.array_equal(np.unique(a("pt_lm")), np.arange(npt)) and np.array_equal(np.unique(a("ls_lm")), np.arange(nls))
    for kind in ("pt", "ls"):
        assert np.array_equal(a(f"{kind}_kf_loc"), a(f"{kind}_kf_map") - 1)
        assert a(f"{kind}_kf_map").min() >= 0 and a(f"{kind}_kf_map").max() == nkf
        assert np.array_equal(np.unique(a(f"{kind}_kf_loc")[a(f"{kind}_kf_loc") >= 0]), np.arange(nkf))   # every optimised key frame is observed
    assert g[f"{name}_ref_X"].size == 6 * nkf + 3 * npt + 6 * nls and np.isfinite(g[f"{name}_ref_X"]).all()
    # ---- the run ----
    e, lam, iters = g[f"{name}_ref_err"], g[f"{name}_ref_lam"], int(g[f"{name}_ref_iters"])
    got_applied = [1] + [0 if e[i] > e[i - 1] else 1 for i in range(1, len(e))]
    got_stop = 0 if iters >= max_iters else 1 if len(e) == iters else 2
    assert got_stop == stop == int(g[f"{name}_ref_stop"]) and got_applied == g[f"{name}_ref_applied"].tolist()
    assert len(lam) == len(e) and np.isinf(e[0]) and np.isfinite(e[1:]).all() and np.isfinite(lam).all() and (lam > 0).all()
    if stop == 0:
        assert iters == len(e) == max(max_iters, 1)
    elif stop == 1:
        assert iters == len(e) < max_iters
    else:
        assert iters == len(e) - 1 and len(e) - 1 < max_iters
    if applied is not None:
        assert got_applied == applied
    else:                       # the retry runs: behind the two first solves rejection and retry alternate up to max_iters
        assert mec == 0.0 and len(got_applied) == max_iters >= 12
        assert got_applied == [1, 1] + [0, 1] * ((max_iters - 2) // 2) + [0] * (max_iters % 2)
    # ---- lambda: the second solve at lambda0, then times k behind an applied step and over k behind a rejected one ----
    k = float(cfg[2])
    assert len(lam) < 2 or lam[1] == lam[0]
    for i in range(2, len(lam)):
        assert lam[i] == (lam[i - 1] * k if got_applied[i - 1] else lam[i - 1] / k)
    # ---- every decision away from its threshold; the one exemption has to be exact ----
    pairs = [(i, e[i], e[i - 1]) for i in range(2, len(e))]
    if stop == 1:
        pairs.append((len(e), float(g[f"{name}_ref_err_last"]), float(g[f"{name}_ref_err_prev"])))
    for i, x, y in pairs:
        assert mec == 0.0 or abs(abs(x - y) - mec) >= GAP * mec
        assert abs(x - me) >= GAP * me
        if i < len(e):
            if mec == 0.0 and got_applied[i - 1] == 0:
                assert x == y                                  # the build behind a rejection: the state it had, the err it had
            else:
                assert abs(x - y) >= GAP * max(abs(x), abs(y))
    if name == "wide_reject":   # the default thresholds: the build behind the rejection is the one that stops the loop, on an equal err
        assert mec == MEC_DEFAULT and float(g[f"{name}_ref_err_last"]) == float(g[f"{name}_ref_err_prev"]) == e[-1]
    if name.endswith("_dx"):
        assert mec > MEC_DEFAULT and max_iters == 15
    if name in ("n120", "wide_max"):
        assert (max_iters, mec) == (3, 0.0)


@pytest.mark.parametrize("a,b", SAME_PROBLEM, ids=[a for a, _ in SAME_PROBLEM])
def test_the_twin_cases_run_one_problem(a, b):
    (ga, ca), (gb, cb) = _where(a), _where(b)
    assert ga is gb and ca == cb
    assert not np.array_equal(_npz()[f"{a}_cfg"], _npz()[f"{b}_cfg"])


def test_the_cases_taken_from_the_other_fixtures_name_them():
    g = _npz()
    assert str(g["retry_problem"]) == "lba_lm_golden.npz:reject" and str(g["iters0_problem"]) == "lba_lm_golden.npz:main"
    # retry is `reject` with min_error_change = 0: the same two first errs, and the rejection that ended `reject` is its first
    lm = _npz("lba_lm_golden.npz")
    n = len(lm["reject_ref_err"])
    assert np.array_equal(g["retry_ref_err"][:n], lm["reject_ref_err"]) and g["retry_ref_applied"][n - 1] == 0
    assert np.array_equal(g["iters2_ref_err"], lm["main_ref_err"][:2]) and np.array_equal(g["iters2_ref_lam"], lm["main_ref_lam"][:2])
