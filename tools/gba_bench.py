"""Time of the global bundle adjustment on the device (plslam_gba_optimize: 1 + 14 solves at max_iters_lba = 15) on
trajectory-shaped maps -- G1: 400 keyframes, 40 k points, 6 k lines, 4 observations per landmark, one loop; G2: 1500 keyframes,
150 k points, 20 k lines -- and, at G1, the time of the numpy restatement of the same loop (tests/gba_ref.py: a restatement,
not the reference).  Prints one JSON line: median milliseconds per whole call (plan creation excluded).  The per-phase device
split comes from a kernel trace of this tool (rocprofv3 --kernel-trace --stats), grouped by the kernel names of gba.hip and
ldlt_dense.hip.

    python tools/gba_bench.py [--reps 3] [--no-restatement]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (_ROOT, os.path.join(_ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import plslam_amd  # noqa: E402
from plslam_amd import gba, synth  # noqa: E402

SIZES = {"G1": dict(n_kf=400, n_pt=40000, n_ls=6000), "G2": dict(n_kf=1500, n_pt=150000, n_ls=20000)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-restatement", action="store_true")
    ap.add_argument("--sizes", default="G1,G2")
    args = ap.parse_args()
    ctx = plslam_amd.Context(0)
    c = synth.EUROC
    cam = plslam_amd.make_cam(c["fx"], c["fy"], c["cx"], c["cy"])
    out = {"tool": "gba_bench", "unit": "ms (median)", "reps": args.reps, "cases": []}
    for name in args.sizes.split(","):
        m = gba.trajectory_map(obs_per_lm=4, loop=True, seed=11, **SIZES[name])
        t0 = time.perf_counter()
        plan = plslam_amd.GbaPlan(ctx, cam, m["n_map_kf"], m["kf_list"], m["npt"], m["nls"], m["pt_obs"], m["pt_uv"],
                                  m["ls_obs"], m["ls_l"])
        create_ms = (time.perf_counter() - t0) * 1e3
        ts = []
        for _ in range(args.reps + 1):
            t0 = time.perf_counter()
            r = plan.optimize(m["T_kf_w"], m["x_kf"], m["Xw"], m["Lw"])
            ts.append((time.perf_counter() - t0) * 1e3)
        plan.close()
        case = dict(size=name, nkf=len(m["kf_list"]), npt=m["npt"], nls=m["nls"], solves=r["n_solves"],
                    plan_create_ms=round(create_ms, 1), optimize_ms=round(float(np.median(ts[1:])), 2),
                    optimize_first_ms=round(ts[0], 2))
        if name == "G1" and not args.no_restatement:
            import gba_ref
            from oracle import oracle as O
            t0 = time.perf_counter()
            gba_ref.gba_lm(gba_ref.Problem(O.make_cam(**c), m), m["x_kf"], m["Xw"], m["Lw"])
            case["numpy_restatement_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
        out["cases"].append(case)
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
