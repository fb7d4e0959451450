"""plslam_lba_plan_optimize_dev (LbaPlan.optimize_dev): the whole LM loop of levMarquardtOptimizationLBA
(src/mapHandler.cpp:1334-1812) on the device in one call, against the REFERENCE'S OWN text run on the same inputs -- every case of
tests/golden/lba_lm_golden.npz and of tests/golden/lba_lm_dev_golden.npz (make_lba_lm_dev_golden.py: the first solve alone, the
loop running out, a lines-only map, one key frame, 21 key frames -- above the one-workgroup solve's boundary --, an exit by the
||DX|| test).  The comparisons and tolerances are tests/test_gpu_lba_lm.py's: control flow, iters and stop exact; lambda to 1e-12
relative; err to 1e-9 relative; the final state to 1e-9 of its scale (+ 100 cond EPS max|step| for the rank-deficient cases); the
first err infinite.  Then: the stop word's predication (lba_loop_peek 1 against 0, a host-built plan against a device-built one, to
the bit), rejected steps, the solve kernel alone, the not-positive-definite exit, the chain gather -> create_dev -> optimize_dev ->
apply_lba, and the refusals."""
import ctypes as C
import os

import numpy as np
import pytest

import plslam_amd
from plslam_amd import capi
from plslam_amd import synth
from plslam_amd.capi import EINVAL, LbaPlan, PlslamError

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = {"lm": os.path.join(ROOT, "tests", "golden", "lba_lm_golden.npz"), "dev": os.path.join(ROOT, "tests", "golden", "lba_lm_dev_golden.npz"),
        "edges": os.path.join(ROOT, "tests", "golden", "lba_lm_dev_edges_golden.npz")}     # (tests/test_gpu_lba_optimize_dev_edges.py)
CASES = [("lm", n) for n in ("main", "reject", "reject_later", "points_only", "two_views", "fixed_heavy")] + \
        [("dev", n) for n in ("first_only", "main_3", "lines_only", "one_kf", "wide", "dx_stop")]
IDS = [n for _, n in CASES]
RANK_DEFICIENT = ("two_views", "fixed_heavy")
EPS = np.finfo(np.float64).eps
_cache = {}


def _gold(which):
    if which not in _cache:
        _cache[which] = dict(np.load(GOLD[which]))
    return _cache[which]


def _cam():
    return plslam_amd.make_cam(**synth.EUROC)


def _problem(which, name):
    g = _gold(which)
    src, case = g, name
    if f"{name}_problem" in g:                 # "<fixture file>:<case>": the problem's arrays are stored there, once
        fixture, case = str(g[f"{name}_problem"]).split(":")
        src = _gold({os.path.basename(v): k for k, v in GOLD.items()}[fixture])
    a = lambda k: src[f"{case}_{k}"]                                            # noqa: E731
    cfg = g[f"{name}_cfg"] if f"{name}_cfg" in g else g["cfg"]
    n_map, nkf = int(a("n_kf_map")), int(a("nkf"))
    # pose slots: the stored T_kf_w of every key frame, then the estimate slots -- which hold the stored poses on entry (:1369)
    T = np.concatenate([a("T_map").reshape(-1, 16), a("T_map").reshape(-1, 16)[1:1 + nkf]])
    return dict(n_map=n_map, nkf=nkf, npt=a("Xw").shape[0], nls=a("Lw").shape[0], T=T, x_kf=a("x_kf").reshape(nkf, 6).copy(),
                Xw=a("Xw").reshape(-1, 3), Lw=a("Lw").reshape(-1, 6),
                cols=dict(pt_lm=a("pt_lm").astype(np.int32), pt_slot=np.where(a("pt_kf_loc") >= 0, n_map + a("pt_kf_loc"), a("pt_kf_map")).astype(np.int32),
                          pt_kf_loc=a("pt_kf_loc").astype(np.int32), pt_obs_uv=a("pt_uv").reshape(-1, 2),
                          ls_lm=a("ls_lm").astype(np.int32), ls_slot=a("ls_kf_map").astype(np.int32), ls_kf_loc=a("ls_kf_loc").astype(np.int32),
                          ls_l_obs=a("ls_l").reshape(-1, 3)),
                th=float(cfg[0]), prm=dict(lambda_lm=float(cfg[1]), lambda_k=float(cfg[2]), max_iters=int(cfg[3]),
                                           min_error_change=float(cfg[4]), min_error=float(cfg[5])),
                ref={k: g[f"{name}_ref_{k}"] for k in ("X", "lam", "err", "iters", "err_last", "err_prev", "lam_last")})


def _host_plan(ctx, p):
    c = p["cols"]
    plan = LbaPlan(ctx, _cam(), p["th"], p["n_map"] + p["nkf"], p["nkf"], p["npt"], p["nls"], c["pt_lm"], c["pt_slot"], c["pt_kf_loc"],
                   c["pt_obs_uv"], c["ls_lm"], c["ls_slot"], c["ls_kf_loc"], c["ls_l_obs"])
    plan.iterate_dev(p["T"], p["Xw"], p["Lw"], want_g=False)               # "a plan that an earlier iterate call has filled"
    return plan


def _dev_plan(ctx, p):
    import torch
    dev = torch.device("cuda", ctx.device)
    keep = {k: torch.from_numpy(np.ascontiguousarray(v) if v.size else np.zeros(1, v.dtype)).to(dev)
            for k, v in dict(p["cols"], Xw=p["Xw"], Lw=p["Lw"]).items()}
    torch.cuda.synchronize()
    q = lambda k, n: keep[k].data_ptr() if n else 0                            # noqa: E731
    c = p["cols"]
    plan = LbaPlan.from_device(ctx, _cam(), p["th"], p["n_map"] + p["nkf"], p["nkf"], p["npt"], p["nls"], q("pt_lm", c["pt_lm"].size),
                               q("pt_slot", c["pt_lm"].size), q("pt_kf_loc", c["pt_lm"].size), q("pt_obs_uv", c["pt_lm"].size), c["pt_lm"].size,
                               q("ls_lm", c["ls_lm"].size), q("ls_slot", c["ls_lm"].size), q("ls_kf_loc", c["ls_lm"].size),
                               q("ls_l_obs", c["ls_lm"].size), c["ls_lm"].size, q("Xw", p["npt"]), q("Lw", p["nls"]))
    plan._keep = keep
    return plan


def _slots(ctx, plan):
    """the pose slots as the device holds them (plslam_lba_plan_device_state)"""
    import torch
    st = plan.device_state()
    t = torch.empty(st["n_pose_slots"] * 16, dtype=torch.float64, device=torch.device("cuda", ctx.device))
    torch.cuda.synchronize()
    assert capi._hip_memcpy_dtod(t.data_ptr(), st["T_kf_w"], t.numel() * 8) == 0
    torch.cuda.synchronize()
    return t.cpu().numpy()


def _run(ctx, p, peek=1, make=_host_plan, **over):
    ctx.set_option("lba_loop_peek", peek)
    try:
        plan = make(ctx, p)
        out = plan.optimize_dev(p["T"], p["x_kf"], p["n_map"], **dict(p["prm"], **over))
        out["Xw"], out["Lw"] = plan.get_landmarks()
        out["slots"] = _slots(ctx, plan)
        plan.close()
    finally:
        ctx.set_option("lba_loop_peek", 1)
    return out


def _run_cached(ctx, which, name, peek=1):
    key = ("run", which, name, peek)
    if key not in _cache:
        _cache[key] = _run(ctx, _problem(which, name), peek)
    return _cache[key]


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


def _same_run(a, b, what):
    for k in ("x_kf", "T", "lam", "err_raw", "err", "dx_norm", "n_singular", "n_bad_pivots", "applied", "Xw", "Lw", "slots"):
        assert a[k].shape == b[k].shape and np.array_equal(_bits(a[k]), _bits(b[k])), (what, k)
    for k in ("iters", "n_builds", "stop_reason", "hmax", "lam_last", "err_prev"):
        assert a[k] == b[k], (what, k)
    assert a["err_last"] == b["err_last"] or (np.isnan(a["err_last"]) and np.isnan(b["err_last"])), what


def _first_solve_cond(p):
    """cond of H + lambda0 diag(H) at the run's start (tests/test_gpu_lba_lm.py: _first_solve_cond)"""
    from oracle import oracle as O
    cam = O.make_cam(*[synth.EUROC[k] for k in ("fx", "fy", "cx", "cy")])
    c, T = p["cols"], p["T"][:p["n_map"]]
    g = _gold("lm")
    kfm = lambda kind, name: g[f"{name}_{kind}_kf_map"]                          # noqa: E731
    name = p["name"]
    rp = O.lba_point_rows(cam, p["th"], T, p["Xw"], c["pt_obs_uv"], c["pt_lm"], kfm("pt", name))
    rl = O.lba_line_rows(cam, p["th"], T, p["Lw"], c["ls_l_obs"], c["ls_lm"], kfm("ls", name))
    H, _, _ = O.lba_accumulate("points", p["nkf"], p["npt"], p["nls"], c["pt_lm"], c["pt_kf_loc"], *rp)
    H, _, _ = O.lba_accumulate("lines", p["nkf"], p["npt"], p["nls"], c["ls_lm"], c["ls_kf_loc"], *rl, H=H)
    lam0 = p["prm"]["lambda_lm"] * np.abs(np.diag(H)).max()
    return float(np.linalg.cond(H + lam0 * np.diag(np.diag(H))))


# ---- 3. every case of both fixtures against the reference's stored run -----------------------------------------------------------
@pytest.mark.parametrize("which,name", CASES, ids=IDS)
def test_the_loop_on_the_device_equals_the_references_own_text(ctx, which, name):
    _equals_the_references_own_text(ctx, which, name)


def _equals_the_references_own_text(ctx, which, name):
    p = _problem(which, name)
    p["name"] = name
    got, ref = _run_cached(ctx, which, name), p["ref"]
    nkf, npt, nls, k = p["nkf"], p["npt"], p["nls"], p["prm"]["lambda_k"]
    solved = got["applied"] >= 0
    e = ref["err"]
    # ---- control flow: exact ----
    assert int(solved.sum()) == len(ref["lam"]) and got["iters"] == int(ref["iters"]) and got["n_builds"] == len(got["applied"])
    ref_applied = [1] + [0 if e[i] > e[i - 1] else 1 for i in range(1, len(e))]
    assert got["applied"][solved].tolist() == ref_applied
    n_solves, iters = len(e), int(ref["iters"])
    ref_stop = 0 if iters >= p["prm"]["max_iters"] else 1 if n_solves == iters else 2
    if which != "lm":
        assert ref_stop == int(_gold(which)[f"{name}_ref_stop"]) and ref_applied == _gold(which)[f"{name}_ref_applied"].tolist()
    assert got["stop_reason"] == ref_stop
    assert (got["applied"][-1] == -1) == (ref_stop == 1) and (got["applied"][:-1] >= 0).all()
    if name.startswith("reject"):
        assert 0 in ref_applied and got["stop_reason"] == 1
    # ---- lambda: the first to 1e-12 (a sum the device adds in another order), the schedule exactly ----
    lam = got["lam"][solved]
    assert np.allclose(lam, ref["lam"], rtol=1e-12, atol=0), (lam, ref["lam"])
    assert len(lam) < 2 or lam[1] == lam[0]
    assert all(lam[i] in (lam[i - 1] * k, lam[i - 1] / k) for i in range(2, len(lam)))
    assert abs(got["lam_last"] - float(ref["lam_last"])) <= 1e-12 * float(ref["lam_last"])
    assert got["hmax"] * p["prm"]["lambda_lm"] == lam[0]
    # ---- err: the first one the sum over two counters that are never incremented; the others to 1e-9 ----
    assert np.isinf(got["err"][0]) and np.isinf(e[0])
    assert np.allclose(got["err"][solved][1:], e[1:], rtol=1e-9, atol=0)
    if len(got["err"]) > 1:
        assert abs(got["err_last"] - float(ref["err_last"])) <= 1e-9 * abs(float(ref["err_last"]))
        assert got["err_last"] == got["err"][-1]
    if np.isfinite(float(ref["err_prev"])):
        assert abs(got["err_prev"] - float(ref["err_prev"])) <= 1e-9 * abs(float(ref["err_prev"]))
    else:
        assert np.isinf(got["err_prev"])
    # ---- the final state: to rounding ----
    Xref, extra = ref["X"], 0.0
    if name in RANK_DEFICIENT:
        cond = _first_solve_cond(p)
        assert 100 * cond * EPS <= 1e-2
        start = np.concatenate([p["x_kf"].reshape(-1), p["Xw"].reshape(-1), p["Lw"].reshape(-1)])
        extra = 100 * cond * EPS * float(np.abs(Xref - start).max())
    for what, a, b in (("x_kf", got["x_kf"].reshape(-1), Xref[:6 * nkf]), ("Xw", got["Xw"].reshape(-1), Xref[6 * nkf:6 * nkf + 3 * npt]),
                       ("Lw", got["Lw"].reshape(-1), Xref[6 * nkf + 3 * npt:])):
        if b.size:
            tol = 1e-9 * max(1.0, np.max(np.abs(b))) + extra
            print(f"{name}: {what} off by {np.max(np.abs(a - b)):.3g}, allowed {tol:.3g}")
            assert np.max(np.abs(a - b)) <= tol, (what, np.max(np.abs(a - b)))
    # T_out = expmap_se3(x_kf_out) (:1822-1826), and the estimate slots hold it
    from oracle import oracle as O
    for kf in range(nkf):
        assert np.allclose(got["T"][kf], O.expmap_se3(got["x_kf"][kf]).reshape(4, 4), rtol=0, atol=1e-12)
    assert np.array_equal(_bits(got["slots"].reshape(-1, 16)[p["n_map"]:]), _bits(got["T"].reshape(-1, 16)))
    assert np.array_equal(_bits(got["slots"].reshape(-1, 16)[:p["n_map"]]), _bits(p["T"][:p["n_map"]]))
    assert (got["n_singular"] == 0).all() and (got["n_bad_pivots"] == 0).all()
    assert np.all(got["dx_norm"][solved] > 0)


# ---- 4. predication: passes enqueued behind the stop change nothing ----------------------------------------------------------------
@pytest.mark.parametrize("which,name", CASES, ids=IDS)
def test_passes_behind_the_stop_change_nothing(ctx, which, name):
    p = _problem(which, name)
    a, b = _run_cached(ctx, which, name, 1), _run_cached(ctx, which, name, 0)
    _same_run(a, b, "lba_loop_peek 1 against 0")
    assert b["n_enqueued_passes"] == max(p["prm"]["max_iters"], 1)
    assert a["n_builds"] <= a["n_enqueued_passes"] <= b["n_enqueued_passes"]
    print(f"{name}: builds {a['n_builds']}, enqueued with the peek {a['n_enqueued_passes']}, without {b['n_enqueued_passes']}")


@pytest.mark.parametrize("which,name", CASES, ids=IDS)
def test_a_device_built_plan_gives_the_host_built_plans_bits(ctx, which, name):
    p = _problem(which, name)
    for peek in (1, 0):
        _same_run(_run_cached(ctx, which, name, peek), _run(ctx, p, peek, make=_dev_plan), f"plslam_lba_plan_create_dev, peek {peek}")


# ---- 5. a rejected step leaves the state as it was -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["reject", "reject_later"])
def test_a_rejected_step_leaves_landmarks_and_poses_untouched(ctx, name):
    p = _problem("lm", name)
    full = _run_cached(ctx, "lm", name)
    r = int(np.flatnonzero(full["applied"] == 0)[0])
    assert r >= 2
    before = _run(ctx, p, max_iters=r)                  # builds 0 .. r - 1 and their steps
    after = _run(ctx, p, max_iters=r + 1)               # ... and build r, whose step is rejected
    assert before["n_builds"] == r and after["n_builds"] == r + 1 and after["applied"].tolist() == [1] * r + [0]
    assert before["stop_reason"] == after["stop_reason"] == 0
    for k in ("x_kf", "T", "Xw", "Lw", "slots"):
        assert np.array_equal(_bits(before[k]), _bits(after[k])), k
    assert after["lam_last"] == after["lam"][-1] / p["prm"]["lambda_k"] and after["dx_norm"][-1] > 0
    assert after["err_prev"] == after["err"][-1]        # err_prev = err after a rejected step too (:1811)


# ---- 6. the solve alone ----------------------------------------------------------------------------------------------------------------
def _spd(n, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    Q, _ = np.linalg.qr(rng.standard_normal((n, n)))
    A = (Q * np.geomspace(1.0, 1e4, n)) @ Q.T
    return (A + A.T) / 2, rng.standard_normal(n)


# 84 | 90: the one-workgroup solve either side of 64 kB of LDS; 120 | 121: its last size and the padded route's first, n no multiple
# of 6; 126, 128, 129, 160: on and either side of the 32-wide tile the padded copy is rounded to
@pytest.mark.parametrize("n", [1, 6, 54, 84, 90, capi.LBA_SOLVE_MAX_N6, capi.LBA_SOLVE_MAX_N6 + 1, capi.LBA_SOLVE_MAX_N6 + 6, 128, 129, 160])
def test_reduced_ldlt_solve_against_numpy(ctx, n):
    assert capi.LBA_SOLVE_MAX_N6 == 120
    A, b = _spd(n, 100 + n)
    cond = float(np.linalg.cond(A))
    assert cond <= 1e8
    x, nbad = ctx.lba_reduced_ldlt_solve(A, b)
    ref = np.linalg.solve(A, b)
    tol = 100 * cond * EPS * np.abs(ref).max()
    print(f"n {n}: cond {cond:.3g}, off by {np.abs(x - ref).max():.3g}, allowed {tol:.3g}")
    assert nbad == 0 and np.abs(x - ref).max() <= tol
    # only the lower triangle is read
    U = np.tril(A) + np.triu(np.full((n, n), np.nan), 1)
    x2, _ = ctx.lba_reduced_ldlt_solve(U, b)
    assert np.array_equal(_bits(x2), _bits(x))
    # one negative pivot: an ordinary numeric outcome
    Q, _ = np.linalg.qr(np.random.Generator(np.random.PCG64(n)).standard_normal((n, n)))
    d = np.linspace(1.0, 2.0, n)
    d[n // 2] = -1.0
    Aneg = (Q * d) @ Q.T
    _, nbad = ctx.lba_reduced_ldlt_solve((Aneg + Aneg.T) / 2, b)
    assert nbad >= 1


def test_refusals_of_the_solve(ctx):
    L, one = ctx._L, np.ones(1)
    p = lambda a: a.ctypes.data_as(C.c_void_p)                                  # noqa: E731
    for args in ((None, 1, p(one), p(one), p(one)), (ctx.handle, 0, p(one), p(one), p(one)), (ctx.handle, 1, None, p(one), p(one)),
                 (ctx.handle, 1, p(one), None, p(one)), (ctx.handle, 1, p(one), p(one), None)):
        assert L.plslam_lba_reduced_ldlt_solve(*args, None) == EINVAL


def test_a_keyframe_without_observations_ends_the_loop_not_positive_definite(ctx):
    """an optimised key frame that no observation names: its block of the reduced system is zero, its pivots are zero -- stop
    reason 3 at the first solve, with the state of before that solve"""
    p = _problem("lm", "points_only")
    p["nkf"] += 1
    p["T"] = np.concatenate([p["T"], p["T"][:1]])
    p["x_kf"] = np.concatenate([p["x_kf"], np.full((1, 6), 0.01)])
    got = _run(ctx, p)
    assert got["stop_reason"] == capi.LBA_STOP_NOT_PD and got["iters"] == 0 and got["n_builds"] == 1
    assert got["applied"].tolist() == [0] and got["n_bad_pivots"][0] >= 1 and got["lam"][0] > 0 and np.isinf(got["err"][0])
    assert np.array_equal(_bits(got["x_kf"]), _bits(p["x_kf"])) and np.array_equal(_bits(got["Xw"]), _bits(p["Xw"]))
    assert np.array_equal(_bits(got["slots"].reshape(-1, 16)), _bits(p["T"]))
    from oracle import oracle as O
    for kf in range(p["nkf"]):
        assert np.allclose(got["T"][kf], O.expmap_se3(p["x_kf"][kf]).reshape(4, 4), rtol=0, atol=1e-12)
    _same_run(got, _run(ctx, p, 0), "not positive definite, lba_loop_peek 0")


# ---- 7. the chain on the image ---------------------------------------------------------------------------------------------------------
def test_the_chain_gather_plan_optimize_apply_equals_the_host_built_route(ctx):
    import test_gpu_lba_plan_dev as PD
    m, p, T = PD._scene()
    th = 0.01
    ix, lm, c = PD._gathered(ctx, m, p)
    g = lm.download()
    Ts, nkf, npt = PD._slots(T, g), c["nkf"], c["npt"]
    x_kf = g["X_aux"][:6 * nkf].reshape(nkf, 6)
    dev = PD._plan_from_gather(ctx, m, lm, c)
    a = dev.optimize_dev(Ts, x_kf, m["n_map_kf"], max_iters=4)
    moved = lm.apply_lba(dev, ix, th)
    image_dev = PD._image(ix)
    host = PD._host_plan_from_gather(ctx, m, g)
    x = g["X_aux"][6 * nkf:]
    host.iterate_dev(Ts, x[:3 * npt].reshape(-1, 3), x[3 * npt:].reshape(-1, 6), want_g=False)
    b = host.optimize_dev(Ts, x_kf, m["n_map_kf"], max_iters=4)
    for k in ("x_kf", "T", "lam", "err", "dx_norm", "applied"):
        assert np.array_equal(_bits(a[k]), _bits(b[k])), k
    assert a["applied"][0] == 1 and a["n_builds"] >= 2 and (a["iters"], a["stop_reason"]) == (b["iters"], b["stop_reason"])
    Xn, Ln = host.get_landmarks()
    want, (mp, ml) = PD._write_back(m, g, Xn, Ln, th)
    assert moved == dict(n_pt_moved=int(mp.sum()), n_ls_moved=int(ml.sum()))
    assert not np.array_equal(Xn, x[:3 * npt].reshape(-1, 3))            # not vacuous: the loop moved the landmarks
    from plslam_amd import local_map as LM
    m2 = dict(m, points=dict(m["points"], X=want["points.X"], inlier=want["points.inlier"]),
              lines=dict(m["lines"], X=want["lines.X"], inlier=want["lines.inlier"]))
    image_host = PD._image(LM.DeviceMapIndex(m2, ctx.device))
    for k in image_dev:
        PD._same(image_dev[k], image_host[k], "the image after apply_lba: " + k)
    for q in (dev, host, lm):
        q.close()


# ---- 8. the refusals: PLSLAM_EINVAL, nothing launched ------------------------------------------------------------------------------------
def test_refusals(ctx):
    p = _problem("lm", "points_only")
    L = ctx._L
    plan = _host_plan(ctx, p)
    n = p["n_map"]
    prm = capi.LbaLmParams(1e-5, 10.0, 15, 0, 1e-7, 1e-7)
    xo, res = np.empty((p["nkf"], 6)), capi.LbaResult()
    T, x = np.ascontiguousarray(p["T"]), np.ascontiguousarray(p["x_kf"])
    q = lambda a: a.ctypes.data_as(C.c_void_p)                                  # noqa: E731

    def call(h=plan._h, prm_=prm, T_=q(T), x_=q(x), first=n, xo_=q(xo), res_=C.byref(res)):
        return L.plslam_lba_plan_optimize_dev(h, C.byref(prm_) if prm_ is not None else None, T_, x_, first, xo_, None, None, res_)
    before = plan.get_landmarks()
    assert call(h=None) == EINVAL and call(prm_=None) == EINVAL and call(T_=None) == EINVAL and call(x_=None) == EINVAL
    assert call(xo_=None) == EINVAL and call(res_=None) == EINVAL
    assert call(prm_=capi.LbaLmParams(1e-5, 0.0, 15, 0, 1e-7, 1e-7)) == EINVAL
    assert call(first=-1) == EINVAL and call(first=n + 1) == EINVAL
    after = plan.get_landmarks()
    assert all(np.array_equal(_bits(u), _bits(v)) for u, v in zip(before, after))
    assert call() == 0 and res.n_builds >= 1                                   # (the same arguments, none of them wrong)
    plan.close()
    # no optimised key frame; landmarks that are not resident
    c = p["cols"]
    none = LbaPlan(ctx, _cam(), p["th"], n, 0, p["npt"], 0, c["pt_lm"], c["pt_kf_loc"] + 1, np.full_like(c["pt_kf_loc"], -1), c["pt_obs_uv"],
                   c["ls_lm"], c["ls_slot"], c["ls_kf_loc"], c["ls_l_obs"])
    none.iterate_dev(p["T"][:n], p["Xw"], p["Lw"], want_g=False)
    assert call(h=none._h, first=0) == EINVAL
    none.close()
    fresh = LbaPlan(ctx, _cam(), p["th"], n + p["nkf"], p["nkf"], p["npt"], p["nls"], c["pt_lm"], c["pt_slot"], c["pt_kf_loc"], c["pt_obs_uv"],
                    c["ls_lm"], c["ls_slot"], c["ls_kf_loc"], c["ls_l_obs"])
    with pytest.raises(PlslamError) as e:
        fresh.optimize_dev(p["T"], p["x_kf"], n)
    assert e.value.code == EINVAL
    fresh.close()
