"""The LM loop of levMarquardtOptimizationLBA (src/mapHandler.cpp:1334-1812) as a drop-in: PLSLAM::LbaPlanSolver::optimize
(plslam_amd/host/lba_rows.hpp, C++ over the C ABI: resident plan, Schur step, host LDL^T of the reduced camera system) against
the REFERENCE'S OWN text run on the same inputs -- tests/golden/lba_lm_golden.npz, written by tests/golden/make_lba_lm_golden.py
from oracle/_ref (ref_wrap_lba_lm.cpp compiles the function body where it lies).  Compared: which steps were applied, the lambda
schedule, the number of iterations and the stop (exactly), the lambda of every solve (1e-12: lambda0 scales with a sum the
device adds in another order), every err (1e-9 relative) and the final state (1e-9 of its
scale; the reference solves all N unknowns with one LDL^T, the product the Schur complement: equal to rounding)."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "lba_lm_golden.npz")
CASES = ("main", "reject", "reject_later", "points_only", "two_views", "fixed_heavy")
# two views per landmark: every landmark block lacks rank (2 of 3, 2 of 6) and only the damping makes it invertible; fixed_heavy:
# half the observations by the key frame that is not optimised.  Their numbers are compared at
#     1e-9 * scale + 100 * cond * EPS * max|step|
# with cond the condition number of the first pass's damped H at lambda0 (lambda grows on success in this loop, so the first solve
# is the worst conditioned) and max|step| the largest move of an unknown over the run; control flow stays exact as for the others
RANK_DEFICIENT = ("two_views", "fixed_heavy")
EPS = np.finfo(np.float64).eps
EUROC = (458.654, 457.296, 367.215, 248.375)          # config/dataset_params/euroc_params.yaml:2 (synth.EUROC)


def _compile(tmp):
    exe = os.path.join(tmp, "test_lm_loop")
    cmd = [shutil.which("g++") or "g++", "-O2", "-std=c++17", "-pthread", os.path.join(ROOT, "tests", "cpp", "test_lm_loop.cpp"),
           "-I" + os.path.join(ROOT, "include"), "-L" + os.path.join(ROOT, "plslam_amd", "lib"), "-lplslam_hip",
           "-L" + os.path.join(ROOT, "oracle"), "-lplslam_oracle",
           "-Wl,-rpath," + os.path.join(ROOT, "plslam_amd", "lib"), "-Wl,-rpath," + os.path.join(ROOT, "oracle"),
           "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib", "-lamdhip64", "-o", exe]
    subprocess.run(cmd, check=True)
    return exe


def _write_problem(path, g, name):
    i32 = lambda k: np.ascontiguousarray(g[f"{name}_{k}"], np.int32)          # noqa: E731
    f64 = lambda k: np.ascontiguousarray(g[f"{name}_{k}"], np.float64)        # noqa: E731
    nkf, n_kf_map = int(g[f"{name}_nkf"]), int(g[f"{name}_n_kf_map"])
    npt, nls = f64("Xw").shape[0], f64("Lw").shape[0]
    with open(path, "wb") as f:
        f.write(struct.pack("<6i", nkf, n_kf_map, npt, nls, i32("pt_lm").size, i32("ls_lm").size))
        f.write(np.ascontiguousarray(g["cfg"], np.float64).tobytes())
        f.write(np.array(EUROC, np.float64).tobytes())
        for k in ("T_map", "x_kf", "Xw", "Lw"):
            f.write(f64(k).tobytes())
        for k in ("pt_lm", "pt_kf_map", "pt_kf_loc"):
            f.write(i32(k).tobytes())
        f.write(f64("pt_uv").tobytes())
        for k in ("ls_lm", "ls_kf_map", "ls_kf_loc"):
            f.write(i32(k).tobytes())
        f.write(f64("ls_l").tobytes())
    return nkf, npt, nls


def _read_result(path, nkf, npt, nls):
    b = open(path, "rb").read()
    n, iters, stop, nsing = struct.unpack_from("<4i", b, 0)
    off = 16
    take = lambda dt, cnt: np.frombuffer(b, dt, cnt, off)                       # noqa: E731
    out = dict(iters=iters, stop=stop, n_singular=nsing)
    for key, dt, cnt in (("err", np.float64, n), ("lam", np.float64, n), ("applied", np.int32, n), ("x_kf", np.float64, 6 * nkf),
                         ("Xw", np.float64, 3 * npt), ("Lw", np.float64, 6 * nls), ("moved_p", np.uint8, npt), ("moved_l", np.uint8, nls)):
        out[key] = take(dt, cnt).copy()
        off += out[key].nbytes
    assert off == len(b)
    return out


def _first_solve_cond(g, name):
    """cond of H + lambda0 diag(H), lambda0 = lambdaLbaLM * max H(i,i) (:1544-1556), H from the oracle's rows and dense accumulation
    at the run's initial state"""
    import sys
    sys.path.insert(0, ROOT)
    from oracle import oracle as O
    cam = O.make_cam(*EUROC)
    a = lambda k: g[f"{name}_{k}"]                                              # noqa: E731
    nkf, npt, nls = int(a("nkf")), a("Xw").shape[0], a("Lw").shape[0]
    rp = O.lba_point_rows(cam, float(g["cfg"][0]), a("T_map"), a("Xw"), a("pt_uv"), a("pt_lm"), a("pt_kf_map"))
    rl = O.lba_line_rows(cam, float(g["cfg"][0]), a("T_map"), a("Lw"), a("ls_l"), a("ls_lm"), a("ls_kf_map"))
    H, _, _ = O.lba_accumulate("points", nkf, npt, nls, a("pt_lm"), a("pt_kf_loc"), *rp)
    H, _, _ = O.lba_accumulate("lines", nkf, npt, nls, a("ls_lm"), a("ls_kf_loc"), *rl, H=H)
    lam0 = float(g["cfg"][1]) * np.abs(np.diag(H)).max()
    return float(np.linalg.cond(H + lam0 * np.diag(np.diag(H)))), lam0


def test_the_fixture_holds_the_cases_and_the_new_ones_are_what_they_are_named_for():
    """CPU: every case is in the fixture with a finite run of the reference's text; two_views has two observations per landmark,
    fixed_heavy half of its observations by key frame 0; for both 100 * cond * EPS <= 1e-2 and lambda0 is the fixture's"""
    g = np.load(GOLD)
    for name in CASES:
        assert all(np.isfinite(g[f"{name}_ref_{k}"]).all() for k in ("X", "lam", "err_last")), name
    for name in RANK_DEFICIENT:
        assert (int(g[f"{name}_n_kf_map"]), g[f"{name}_Xw"].shape[0], g[f"{name}_Lw"].shape[0]) == (5, 90, 30)
        assert (np.bincount(g[f"{name}_pt_lm"]) == 2).all() and (np.bincount(g[f"{name}_ls_lm"]) == 2).all()
        cond, lam0 = _first_solve_cond(g, name)
        print(f"{name}: cond {cond:.3g}, 100 cond EPS {100 * cond * EPS:.2e}, lambda0 {lam0:.6g}")
        assert 100 * cond * EPS <= 1e-2
        assert abs(lam0 - g[f"{name}_ref_lam"][0]) <= 1e-12 * lam0
    kf = np.concatenate([g["fixed_heavy_pt_kf_map"], g["fixed_heavy_ls_kf_map"]])
    assert 2 * int((kf == 0).sum()) == kf.size and (g["fixed_heavy_pt_kf_loc"] == g["fixed_heavy_pt_kf_map"] - 1).all()


def test_lm_test_program_compiles_against_the_abi(tmp_path):
    """CPU: LbaPlanSolver::optimize and its test program compile and link against the C-ABI library."""
    _compile(str(tmp_path))


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASES)
def test_lm_loop_equals_the_references_own_text(tmp_path, name):
    g = np.load(GOLD)
    exe = _compile(str(tmp_path))
    prob, res = str(tmp_path / "p.bin"), str(tmp_path / "r.bin")
    nkf, npt, nls = _write_problem(prob, g, name)
    r = subprocess.run([exe, prob, res], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-1000:] + r.stderr[-2000:]
    got = _read_result(res, nkf, npt, nls)
    ref = {k: g[f"{name}_ref_{k}"] for k in ("X", "lam", "err", "iters", "err_last", "err_prev", "lam_last")}
    solved = got["applied"] >= 0                         # the product's trace has one entry per H / g build, the reference's per solve
    # ---- control flow: exact ----
    assert int(solved.sum()) == len(ref["lam"]) and got["iters"] == int(ref["iters"])
    # lambda0 = lambdaLbaLM * max |H(i,i)|: the largest diagonal entry is a key frame's, and the device adds a key frame's
    # observations in chunk order where the reference adds them in list order (equal to rounding, not to the bit); from there on
    # every lambda is the one before times or over lambda_k -- the SCHEDULE is compared exactly through `applied` below
    assert np.allclose(got["lam"][solved], ref["lam"], rtol=1e-12, atol=0), (got["lam"], ref["lam"])
    lam = got["lam"][solved]
    assert lam[1] == lam[0] and all(lam[i] in (lam[i - 1] * 10.0, lam[i - 1] / 10.0) for i in range(2, len(lam)))
    # which steps were applied: the first one always; later ones unless err > err_prev (the reference's :1786)
    e = ref["err"]
    ref_applied = [1] + [0 if (i >= 1 and e[i] > e[i - 1]) else 1 for i in range(1, len(e))]
    assert got["applied"][solved].tolist() == ref_applied
    if name.startswith("reject"):
        assert 0 in ref_applied and got["stop"] == 1     # a rejected step, then the same err again: the first stop test
    # the first pass's err: the sum over the two never-incremented counters (:1541) -- +inf on both sides
    assert np.isinf(got["err"][0]) and np.isinf(e[0])
    # ---- numbers: to rounding ----
    assert np.allclose(got["err"][solved][1:], e[1:], rtol=1e-9, atol=0)
    assert abs(got["err"][-1] - float(ref["err_last"])) <= 1e-9 * abs(float(ref["err_last"]))
    Xref = ref["X"]
    extra = 0.0
    if name in RANK_DEFICIENT:
        cond = _first_solve_cond(g, name)[0]
        assert 100 * cond * EPS <= 1e-2
        start = np.concatenate([g[f"{name}_x_kf"].reshape(-1), g[f"{name}_Xw"].reshape(-1), g[f"{name}_Lw"].reshape(-1)])
        extra = 100 * cond * EPS * float(np.abs(Xref - start).max())
    for a, b_ in ((got["x_kf"], Xref[:6 * nkf]), (got["Xw"], Xref[6 * nkf:6 * nkf + 3 * npt]), (got["Lw"], Xref[6 * nkf + 3 * npt:])):
        if b_.size:
            print(f"{name}: final state off by {np.max(np.abs(a - b_)):.3g}, allowed {1e-9 * max(1.0, np.max(np.abs(b_))) + extra:.3g}")
            assert np.max(np.abs(a - b_)) <= 1e-9 * max(1.0, np.max(np.abs(b_))) + extra, np.max(np.abs(a - b_))
    assert got["n_singular"] == 0
    # the write-back's flags (:1825, :1840): landmarks that moved by more than 0.01
    mp = np.linalg.norm(Xref[6 * nkf:6 * nkf + 3 * npt].reshape(-1, 3) - g[f"{name}_Xw"], axis=1) > 0.01
    ml = np.linalg.norm(Xref[6 * nkf + 3 * npt:].reshape(-1, 6) - g[f"{name}_Lw"], axis=1) > 0.01 if nls else np.zeros(0, bool)
    # (a landmark within 1e-9 of the threshold could flip; none is in these fixtures)
    assert np.array_equal(got["moved_p"].astype(bool), mp) and np.array_equal(got["moved_l"].astype(bool), ml)


@pytest.mark.gpu
def test_resident_iteration_time_at_c3_native(tmp_path):
    """One LM iteration at the C3 map (9 optimised key frames, 10 000 points, 2 000 lines, 60 000 observations) as
    LbaPlanSolver::optimize runs it -- plslam_lba_plan_iterate_schur + the host's 54 x 54 LDL^T + plslam_lba_plan_apply_step --
    timed host to host from C++ (no interpreter in the loop).  Written to gpurun_out/lm_iteration_native.json; the bound here is
    a loose one against a regression to per-kernel synchronisation, not the target."""
    import json
    import re
    import sys
    sys.path.insert(0, ROOT)
    from oracle import oracle as O
    from plslam_amd import synth
    lm = synth.local_map()
    n_kf_map = lm["T_kf_w"].shape[0]
    x = np.stack([O.logmap_se3(T) for T in lm["T_kf_w"].reshape(-1, 4, 4)])
    g = {"cfg": np.array([1e-7, 1e-5, 10.0, 15, 1e-7, 1e-7]), "c3_nkf": n_kf_map - 1, "c3_n_kf_map": n_kf_map,
         "c3_T_map": lm["T_kf_w"], "c3_x_kf": x[1:].reshape(-1), "c3_Xw": lm["Xw"], "c3_Lw": lm["Lw"],
         "c3_pt_lm": lm["pt_lm"], "c3_pt_kf_map": lm["pt_kf"], "c3_pt_kf_loc": lm["pt_kf"] - 1, "c3_pt_uv": lm["obs_uv"],
         "c3_ls_lm": lm["ls_lm"], "c3_ls_kf_map": lm["ls_kf"], "c3_ls_kf_loc": lm["ls_kf"] - 1, "c3_ls_l": lm["l_obs"]}
    exe = _compile(str(tmp_path))
    prob = str(tmp_path / "c3.bin")
    nkf, npt, nls = _write_problem(prob, g, "c3")
    assert (nkf, npt, nls) == (9, 10000, 2000)
    r = subprocess.run([exe, prob, "--time", "300"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-1000:] + r.stderr[-2000:]
    m = re.search(r"median ([0-9.]+) us, p10 ([0-9.]+), p90 ([0-9.]+)", r.stdout)
    assert m, r.stdout
    med, p10, p90 = (float(v) for v in m.groups())
    out = os.path.join(ROOT, "gpurun_out")
    os.makedirs(out, exist_ok=True)
    with open(os.path.join(out, "lm_iteration_native.json"), "w") as f:
        json.dump({"what": "one LM iteration, state and blocks resident, C3 sizes, C++ host to host: plslam_lba_plan_iterate_schur + "
                           "dense LDL^T of the 54 x 54 reduced system + plslam_lba_plan_apply_step (no update)",
                   "us_median": med, "us_p10": p10, "us_p90": p90, "reps": 300}, f)
    print(r.stdout.strip())
    assert med < 400.0
