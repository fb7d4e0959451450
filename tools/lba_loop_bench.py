"""The local BA's whole LM loop, host to host from C++ (no interpreter in the loop): PLSLAM::LbaPlanSolver::optimizeResident -- the
route every client had so far: two calls and two synchronisations per iteration, the 6 nkf x 6 nkf solve and the SE(3) maps on the
host -- against LbaPlanSolver::optimizeOnDevice (plslam_lba_plan_optimize_dev: one call, one synchronisation), at C3 (9 optimised
key frames, 10 000 points, 2 000 lines) and at the size of the golden fixture's `main` case.  tests/cpp/test_lm_loop_ondev.cpp
--bench runs --calls calls of each in the order parent / new / parent within one process; this tool writes the problems, runs it
once per size with lba_loop_peek 1 and adds the launch and synchronisation counts per call (counted from the sources, see below).

    python tools/lba_loop_bench.py [--calls 30] [--out profiles/lba_loop_dev_bench.json]

Verdict: the new route counts as faster or slower only if its median differs from the mean of the parent's two medians by more
than those two differ from each other (DESIGN.md's criterion for obs_src); otherwise "no difference".
"""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (_ROOT, os.path.join(_ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

from plslam_amd import synth  # noqa: E402
from test_gpu_lba_lm import GOLD, _write_problem  # noqa: E402
from test_gpu_lba_optimize_dev_shim import _compile  # noqa: E402


def _c3():
    from oracle import oracle as O
    lm = synth.local_map()
    n = lm["T_kf_w"].shape[0]
    x = np.stack([O.logmap_se3(T) for T in lm["T_kf_w"].reshape(-1, 4, 4)])
    return {"cfg": np.array([1e-7, 1e-5, 10.0, 15, 1e-7, 1e-7]), "c3_nkf": n - 1, "c3_n_kf_map": n, "c3_T_map": lm["T_kf_w"],
            "c3_x_kf": x[1:].reshape(-1), "c3_Xw": lm["Xw"], "c3_Lw": lm["Lw"], "c3_pt_lm": lm["pt_lm"], "c3_pt_kf_map": lm["pt_kf"],
            "c3_pt_kf_loc": lm["pt_kf"] - 1, "c3_pt_uv": lm["obs_uv"], "c3_ls_lm": lm["ls_lm"], "c3_ls_kf_map": lm["ls_kf"],
            "c3_ls_kf_loc": lm["ls_kf"] - 1, "c3_ls_l": lm["l_obs"]}


def _counts(r):
    """launches / synchronisations per call, counted from the sources.  parent (lba_rows.hpp lmLoop): the first pass is setPoses
    (sync), iterate_resident (3 launches, sync), diag_max (1, sync), schur (3, sync), apply_step (1, sync); a later build is
    iterate_schur (4, sync) and, when it solves, apply_step (1, sync).  new (lba_lm_dev.hip, 6 nkf <= 120): 10 launches for the first
    pass, 7 for every later ENQUEUED pass (the ones behind the stop return at once), 1 for the result; one synchronisation."""
    b = r["builds_parent"]
    solves = b - (1 if r["stop"] == 1 else 0)
    e = r["n_enqueued_passes"]
    return {"parent": {"launches": 8 + 4 * (b - 1) + (solves - 1), "synchronisations": 5 + (b - 1) + (solves - 1)},
            "new": {"launches": 10 + 7 * (e - 1) + 1, "synchronisations": 1, "passes_enqueued_behind_the_stop": e - r["builds"]}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(_ROOT, "profiles", "lba_loop_dev_bench.json"))
    a = ap.parse_args()
    out = {"what": "LbaPlanSolver::optimizeResident (parent) against optimizeOnDevice (new), C++ host to host, microseconds per call",
           "order": "parent_1 / new / parent_2 within one process", "sizes": {}}
    with tempfile.TemporaryDirectory() as tmp:
        exe = _compile(tmp)
        for name, g in (("c3", _c3()), ("main", np.load(GOLD))):
            prob = os.path.join(tmp, name + ".bin")
            _write_problem(prob, g, name)
            r = subprocess.run([exe, prob, "--bench", str(a.calls)], capture_output=True, text=True, timeout=600)
            if r.returncode != 0:
                raise SystemExit(r.stdout[-1000:] + r.stderr[-2000:])
            rec = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("BENCH ")][0][6:])
            p1, p2, new = rec["parent_1_us"]["median"], rec["parent_2_us"]["median"], rec["new_us"]["median"]
            spread, diff = abs(p1 - p2), new - 0.5 * (p1 + p2)
            rec["parent_spread_us"], rec["new_minus_parent_us"] = spread, diff
            rec["verdict"] = "no difference" if abs(diff) <= spread else ("new route faster" if diff < 0 else "new route slower")
            rec["per_call"] = _counts(rec)
            out["sizes"][name] = rec
            print(json.dumps({name: rec}))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
