"""Time of the loop-closure correction on the device on drifted pose graphs (plslam_amd.pgo.pose_graph) -- P1: 120 keyframes,
1 loop; P2: 400 keyframes, 2 loops; P3: 1500 keyframes, 3 loops -- with the envelope L D L^T (the product) and with the dense
L D L^T of the global BA (context option pgo_solver = 1, a comparison path of this tool), plus plslam_lc_correct_map_dev on
40 k and 150 k points (4 dir_list entries each) and, at P1, the numpy restatement (tests/pgo_ref.py: a restatement, not the
reference).  Prints one JSON line: median milliseconds per whole call.

    python tools/pgo_bench.py [--reps 3] [--sizes P1,P2,P3] [--no-restatement] [--no-dense]
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
from plslam_amd import capi, pgo  # noqa: E402

SIZES = {"P1": dict(n_kf=120, n_loops=1), "P2": dict(n_kf=400, n_loops=2), "P3": dict(n_kf=1500, n_loops=3)}


def _time_optimize(ctx, m, reps, solver):
    ctx.set_option("pgo_solver", solver)
    try:
        t0 = time.perf_counter()
        plan = plslam_amd.PgoPlan(ctx, m["kf_valid"], m["full_graph"], m["lc_idx"])
        create_ms = (time.perf_counter() - t0) * 1e3
        ts = []
        for _ in range(reps + 1):
            t0 = time.perf_counter()
            r = plan.optimize(m["T_kf_w"], m["x_kf_w"], m["lc_pose"])
            ts.append((time.perf_counter() - t0) * 1e3)
        plan.close()
    finally:
        ctx.set_option("pgo_solver", 0)
    opt = float(np.median(ts[1:]))
    return r, dict(plan_create_ms=round(create_ms, 2), optimize_ms=round(opt, 2), optimize_first_ms=round(ts[0], 2),
                   iterations=r["iterations"], trials=r["trials"], ms_per_trial=round(opt / max(r["trials"], 1), 3))


def _time_correct(ctx, n_pt, reps):
    import torch
    dev = torch.device("cuda", 0)
    n_kf = 1500
    m = pgo.pose_graph(n_kf=n_kf, n_loops=3, seed=3)
    lm = pgo.anchored_landmarks(n_kf, n_pt, n_dir=4, seed=31, vary_dirs=False)
    Tc = torch.from_numpy(np.stack([pgo.se3_exp(0.01 * np.ones(6))] * n_kf).reshape(n_kf, 16).copy()).to(dev)
    co = torch.ones(n_kf, dtype=torch.uint8, device=dev)
    d = {k: torch.from_numpy(np.ascontiguousarray(lm[k])).to(dev) for k in
         ("anchor_ptr", "anchor_idx", "valid", "X", "med_dir", "dir_ptr", "dirs")}
    p = {k: t.data_ptr() for k, t in d.items()}
    p.update(n=n_pt, n_anchor=lm["anchor_idx"].shape[0], n_dir=lm["dirs"].shape[0])
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps + 1):
        t0 = time.perf_counter()
        capi.correct_map_dev(ctx, n_kf, Tc.data_ptr(), co.data_ptr(), p, None)
        ts.append((time.perf_counter() - t0) * 1e3)
    return round(float(np.median(ts[1:])), 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--sizes", default="P1,P2,P3")
    ap.add_argument("--no-restatement", action="store_true")
    ap.add_argument("--no-dense", action="store_true")
    args = ap.parse_args()
    ctx = plslam_amd.Context(0)
    out = {"tool": "pgo_bench", "unit": "ms (median)", "reps": args.reps, "cases": []}
    for name in args.sizes.split(","):
        m = pgo.pose_graph(seed=3, **SIZES[name])
        r, env = _time_optimize(ctx, m, args.reps, 0)
        case = dict(size=name, n_kf=m["n_map_kf"], n_lc=int(m["lc_idx"].shape[0]), n_active=r["n_active"], n_edges=r["n_edges"],
                    env_width=r["env_width"], env_entries=r["env_entries"], chi_initial=r["chi_initial"],
                    chi_final=r["chi_final"], envelope=env)
        if not args.no_dense:
            rd, den = _time_optimize(ctx, m, max(1, args.reps // 2), 1)
            den["max_abs_x_diff_vs_envelope"] = float(np.abs(rd["x"] - r["x"]).max())
            case["dense"] = den
            case["envelope_speedup"] = round(den["optimize_ms"] / env["optimize_ms"], 2)
        if name == "P1" and not args.no_restatement:
            import pgo_ref
            t0 = time.perf_counter()
            P = pgo_ref.Pgo(m["kf_valid"], m["full_graph"], m["lc_idx"])
            P.optimize(m["T_kf_w"], m["x_kf_w"], m["lc_pose"])
            case["numpy_restatement_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
        out["cases"].append(case)
        print(json.dumps(case), file=sys.stderr, flush=True)
    out["correct_map_dev_ms"] = {f"{n // 1000}k_points": _time_correct(ctx, n, args.reps) for n in (40000, 150000)}
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
