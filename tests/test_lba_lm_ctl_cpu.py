"""The control logic of plslam_lba_plan_optimize_dev (plslam_amd/csrc/lba_lm_ctl.hpp: what its control kernels run on one lane)
without a GPU: tests/cpp/test_lba_lm_ctl.cpp is compiled with g++ alone against plslam_amd/csrc and include.  Its hand cases run
once, every case one test here.  The same program replays every recorded run of the reference's own text -- the six cases of
tests/golden/lba_lm_golden.npz, the six of tests/golden/lba_lm_dev_golden.npz and the eleven of
tests/golden/lba_lm_dev_edges_golden.npz (whose two retry runs are the first to take lm_on_step through lambda / k and then
lambda * k): it is fed the errs the fixtures store (times
Npt + Nls: the raw sums the device hands the function) and must give the reference's iters, its applied / rejected pattern, its
lambda schedule (each lambda the one before times or over lambda_k, exactly) and its stop reason, and must stop consuming builds by
itself.  The fixtures do not store ||DX|| (the text does not hand it out): the replay feeds a step far above the threshold for
every solve but the one behind which the reference left by the :1808 test (a run that ended below max_iters with a solve as its
last build), which gets a zero step.  The program built with the address and undefined-behaviour sanitizers runs stand-alone and
must come out clean."""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HAND = ["first_pass", "first_pass_zero_sum_is_nan", "max_iters_1", "max_iters_0", "schedule_reject_then_stop", "schedule_reject_then_retry",
        "min_error", "dx_test",
        "not_positive_definite", "runs_out"]
SANITIZE = ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]
GOLDEN = [("lba_lm_golden.npz", n) for n in ("main", "reject", "reject_later", "points_only", "two_views", "fixed_heavy")] + \
         [("lba_lm_dev_golden.npz", n) for n in ("first_only", "main_3", "lines_only", "one_kf", "wide", "dx_stop")] + \
         [("lba_lm_dev_edges_golden.npz", n) for n in ("n84", "n90", "n120", "n120_dx", "wide_max", "wide_dx", "wide_reject", "wide_retry",
                                                       "retry", "iters0", "iters2")]
RETRY = ("wide_retry", "retry")


def _build(exe, extra):
    inc = ["-I" + os.path.join(ROOT, d) for d in (os.path.join("plslam_amd", "csrc"), "include")]
    subprocess.run([shutil.which("g++") or "g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror"] + extra +
                   [os.path.join(ROOT, "tests", "cpp", "test_lba_lm_ctl.cpp")] + inc + ["-o", exe], check=True)
    return exe


def _hand(exe):
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    res = {}
    for line in r.stdout.splitlines():
        if line.startswith(("PASS ", "FAIL ")):
            res[line.split(" ", 1)[1].split(":")[0]] = line
    return res, r.returncode, r.stderr


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return _build(str(tmp_path_factory.mktemp("lba_lm_ctl") / "test_lba_lm_ctl"), [])


@pytest.fixture(scope="module")
def exe_san(tmp_path_factory):
    return _build(str(tmp_path_factory.mktemp("lba_lm_ctl_san") / "test_lba_lm_ctl_san"), SANITIZE)


@pytest.fixture(scope="module")
def hand_results(exe):
    return _hand(exe)


@pytest.mark.parametrize("case", HAND)
def test_lba_lm_ctl_hand_case(hand_results, case):
    res = hand_results[0]
    assert case in res, f"{case}: the driver did not run it"
    assert res[case].startswith("PASS "), res[case]


def test_lba_lm_ctl_driver_ran_exactly_the_listed_cases(hand_results):
    res, rc, _ = hand_results
    assert sorted(res) == sorted(HAND)
    assert rc == (0 if all(v.startswith("PASS ") for v in res.values()) else 1)


def test_lba_lm_ctl_clean_under_sanitizers(exe_san):
    """The hand cases in a build of the program with the sanitizers: run as a program, nothing is loaded into Python"""
    res, rc, err = _hand(exe_san)
    assert rc == 0 and not err.strip(), err[-3000:]
    assert sorted(res) == sorted(HAND) and all(v.startswith("PASS ") for v in res.values())


def _case_file(path, fixture, name):
    g = np.load(os.path.join(ROOT, "tests", "golden", fixture))
    cfg = g[f"{name}_cfg"] if f"{name}_cfg" in g.files else g["cfg"]
    lam_lm, lam_k, max_iters, mec, me = float(cfg[1]), float(cfg[2]), int(cfg[3]), float(cfg[4]), float(cfg[5])
    e, lam, iters = g[f"{name}_ref_err"], g[f"{name}_ref_lam"], int(g[f"{name}_ref_iters"])
    src, case = g, name
    if f"{name}_problem" in g.files:                   # "<fixture file>:<case>": where the problem's arrays are stored
        src, case = str(g[f"{name}_problem"]).split(":")
        src = np.load(os.path.join(ROOT, "tests", "golden", src))
    n_lm = float(src[f"{case}_Xw"].shape[0] + src[f"{case}_Lw"].shape[0])
    stop = 0 if iters >= max_iters else 1 if len(e) == iters else 2
    builds = [(1.0 if i == 0 else float(e[i]) * n_lm, 0.5, 0.0 if (stop == 2 and i == len(e) - 1) else 0.5) for i in range(len(e))]
    if stop == 2:
        builds[-1] = (builds[-1][0], 0.0, 0.0)
    if stop == 1:
        builds.append((float(g[f"{name}_ref_err_last"]) * n_lm, 0.5, 0.5))
    consumed = len(builds)
    while len(builds) < max(max_iters, 1) + 2:         # more than the loop may take: it has to stop by itself
        builds.append((builds[-1][0] * 0.5, 0.5, 0.5))
    with open(path, "w") as f:
        f.write(f"{lam_lm!r} {lam_k!r} {max_iters} {mec!r} {me!r} {n_lm!r} {float(lam[0]) / lam_lm!r} {len(builds)}\n")
        for b in builds:
            f.write(f"{b[0]!r} {b[1]!r} {b[2]!r} 0\n")
    e_all = list(e) + ([float(g[f"{name}_ref_err_last"])] if stop == 1 else [])
    return dict(stop=stop, iters=iters, lam=lam, e=e_all, consumed=consumed, lam_k=lam_k, lam_last=float(g[f"{name}_ref_lam_last"]),
                err_last=float(g[f"{name}_ref_err_last"]), err_prev=float(g[f"{name}_ref_err_prev"]))


def _replay(exe, path):
    r = subprocess.run([exe, path], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and not r.stderr.strip(), r.stderr[-2000:]
    B = [ln.split()[1:] for ln in r.stdout.splitlines() if ln.startswith("B ")]
    R = [ln.split()[1:] for ln in r.stdout.splitlines() if ln.startswith("R ")]
    assert len(R) == 1
    return ([(float(a), float(b), int(c)) for a, b, c in B],
            dict(iters=int(R[0][0]), n_builds=int(R[0][1]), stop=int(R[0][2]), lam=float(R[0][3]), err=float(R[0][4]), err_prev=float(R[0][5])))


@pytest.mark.parametrize("fixture,name", GOLDEN, ids=[n for _, n in GOLDEN])
@pytest.mark.parametrize("san", [False, True], ids=["plain", "sanitized"])
def test_lba_lm_ctl_replays_the_references_run(exe, exe_san, tmp_path, fixture, name, san):
    want = _case_file(str(tmp_path / "case.txt"), fixture, name)
    B, R = _replay(exe_san if san else exe, str(tmp_path / "case.txt"))
    e, lam, k = want["e"], want["lam"], want["lam_k"]
    assert R["iters"] == want["iters"] and R["stop"] == want["stop"] and R["n_builds"] == len(B) == want["consumed"]
    applied = [b[2] for b in B]
    ref_applied = [1] + [0 if e[i] > e[i - 1] else 1 for i in range(1, len(lam))] + ([-1] if want["stop"] == 1 else [])
    assert applied == ref_applied
    got_lam = [b[0] for b in B if b[2] >= 0]
    assert np.allclose(got_lam, lam, rtol=1e-12, atol=0)
    assert len(got_lam) < 2 or got_lam[1] == got_lam[0]
    for i in range(2, len(got_lam)):                   # times lambda_k behind an applied step, over it behind a rejected one: exactly
        assert got_lam[i] == (got_lam[i - 1] * k if applied[i - 1] == 1 else got_lam[i - 1] / k)
    if name in RETRY:                                  # lambda / k behind a rejection, the SAME err, the retry applied, lambda * k
        rej = [i for i in range(len(applied) - 2) if applied[i] == 0]
        assert rej and all(applied[i + 1] == 1 and B[i + 1][1] == B[i][1] for i in rej)
        assert all(got_lam[i + 1] == got_lam[i] / k and got_lam[i + 2] == got_lam[i + 1] * k for i in rej)
    assert abs(R["lam"] - want["lam_last"]) <= 1e-12 * want["lam_last"]
    assert np.isinf(B[0][1]) and np.allclose([b[1] for b in B[1:]], e[1:], rtol=1e-15, atol=0)
    if len(B) > 1:
        assert abs(R["err"] - want["err_last"]) <= 1e-15 * want["err_last"]
    assert (np.isinf(R["err_prev"]) and np.isinf(want["err_prev"])) or abs(R["err_prev"] - want["err_prev"]) <= 1e-15 * want["err_prev"]
