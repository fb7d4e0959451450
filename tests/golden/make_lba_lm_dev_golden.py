#!/usr/bin/env python3
"""tests/golden/make_lba_lm_dev_golden.py -- writes tests/golden/lba_lm_dev_golden.npz: the runs of the REFERENCE'S OWN
Levenberg-Marquardt text (oracle.ref_lba_lm: src/mapHandler.cpp:1334-1812 compiled where it lies) that lba_lm_golden.npz lacks and
plslam_lba_plan_optimize_dev has to reproduce (tests/test_gpu_lba_optimize_dev.py):
    first_only   main's problem with max_iters = 1: the first solve only
    main_3       main's problem with max_iters = 3: the loop runs out (stop 0)
    lines_only   a map without points
    one_kf       one optimised key frame (6 x 6 reduced system)
    wide         21 optimised key frames: 6 nkf = 126, above the one-workgroup solve's boundary of 120; few landmarks
    dx_stop      a run that leaves by the ||DX|| test (:1808): main's problem with min_error_change raised above the second
                 solve's ||DX|| (found by a search here: the loop's own schedule never makes the steps small -- a restart from a
                 finished run's state moves as far as the run before it -- so the threshold comes up to the step)
Layout as make_lba_lm_golden.py's, plus <name>_cfg (each case has its own thresholds) and <name>_ref_stop / _ref_applied.
Every decision of every run must be far from its threshold -- 1e-6 relative, a thousand times the 1e-9 to which the device's err
agrees -- so that rounding cannot flip a branch; a candidate that is not is dropped, and a case without a candidate left is an error:
    :1775   | |err - err_prev| - min_error_change | >= 1e-6 min_error_change and |err - min_error| >= 1e-6 min_error, every build
    :1786   |err - err_prev| >= 1e-6 max(err, err_prev), every solve behind the first
    :1808   the text does not hand ||DX|| out: the run is repeated with min_error_change scaled by 1 - 1e-6 and by 1 + 1e-6; the
            :1775 decisions cannot change (the check above), so an unchanged control flow says no ||DX|| lies in between
Run where the reference tree is built into oracle/_ref (python tests/golden/make_lba_lm_dev_golden.py); the GPU tests only read the fixture."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
import make_lba_lm_golden as G  # noqa: E402

GAP = 1e-6
MAIN = G.CASES["main"]


def flow(r, cfg):
    """(stop, applied per solve) of a reference run"""
    n_solves, iters = len(r["lam"]), r["iters"]
    if iters >= int(cfg["max_iters"]):
        stop = 0
    elif n_solves == iters:
        stop = 1                     # the build of iteration `iters` ended the loop before its solve
    else:
        assert n_solves == iters + 1
        stop = 2
    e = r["err"]
    applied = [1] + [0 if e[i] > e[i - 1] else 1 for i in range(1, len(e))]
    return stop, applied


def far_from_thresholds(p, cfg, r, equal_behind_a_rejection=False):
    """equal_behind_a_rejection (make_lba_lm_dev_edges_golden.py): with min_error_change = 0 the build behind a rejected step
    recomputes the state it had, so its err EQUALS the one before, bit for bit; such a pair is left out of the :1786 gap -- only
    when it is exactly equal, and only behind a rejection"""
    mec, me = cfg["min_err_change"], cfg["min_err"]
    stop, applied = flow(r, cfg)
    e = list(r["err"])
    exempt = [equal_behind_a_rejection and mec == 0 and i >= 2 and applied[i - 1] == 0 and e[i] == e[i - 1] for i in range(len(e))]
    pairs = [(e[i], e[i - 1]) for i in range(1, len(e)) if not exempt[i]]
    builds = pairs + ([(r["err_last"], r["err_prev"])] if stop == 1 else [])
    for a, b in builds:                                                   # :1775
        if np.isfinite(b) and abs(abs(a - b) - mec) < GAP * mec:
            return False
        if abs(a - me) < GAP * me:
            return False
    for a, b in pairs:                                                    # :1786
        if np.isfinite(b) and abs(a - b) < GAP * max(abs(a), abs(b)):
            return False
    for s in (1.0 - GAP, 1.0 + GAP):                                      # :1808
        r2 = G.run_ref(p, dict(cfg, min_err_change=mec * s))
        if (r2["iters"], len(r2["lam"])) != (r["iters"], len(r["lam"])) or flow(r2, cfg) != (stop, applied):
            return False
    return True


def candidates():
    """name -> list of (problem, cfg, expected stop or None), tried in order"""
    base = G.CFG
    loose = [dict(base, min_err_change=v) for v in (1e-4, 3e-4, 1e-3)]
    main = G.problem(**MAIN)
    return {
        "first_only": [(main, dict(base, max_iters=1), 0)],
        "main_3": [(main, dict(base, max_iters=3), 0)],
        "lines_only": [(G.problem(n_kf_map=5, n_pt=0, n_ls=120, obs=3, seed=s, sigma_lm=0.05, sigma_pose=0.01), c, None)
                       for s in (41, 42, 43) for c in loose],
        "one_kf": [(G.problem(n_kf_map=2, n_pt=90, n_ls=30, obs=2, seed=s, sigma_lm=0.05, sigma_pose=0.01), c, None)
                   for s in (51, 52, 53) for c in loose],
        "wide": [(G.problem(n_kf_map=22, n_pt=150, n_ls=40, obs=6, seed=s, sigma_lm=0.05, sigma_pose=0.01), c, None)
                 for s in (61, 62, 63) for c in loose],
        "dx_stop": [(main, dict(base, min_err_change=v), 2) for v in (1.0, 2.0, 4.0)],
    }


def main():
    out = {}
    for name, cands in candidates().items():
        for p, cfg, want_stop in cands:
            r = G.run_ref(p, cfg)
            if r is None:
                raise SystemExit("oracle/_ref/libplslam_ref.so (ref_lba_lm) is not available: build it where the reference tree is")
            stop, applied = flow(r, cfg)
            # (the first pass's err is +inf by the text's own division: a run of one build ends with it)
            finite = all(np.isfinite(np.asarray(r[k], np.float64)).all() for k in ("X", "lam")) and np.isfinite(r["err"][1:]).all()
            if not finite or (want_stop is not None and stop != want_stop) or not far_from_thresholds(p, cfg, r):
                print(f"{name}: candidate dropped (stop {stop}, finite {finite})")
                continue
            print(f"{name}: N = {r['X'].size}, solves {len(r['lam'])}, iters {r['iters']}, stop {stop}, applied {applied}, err {r['err']}, "
                  f"last err {r['err_last']:.9g} prev {r['err_prev']:.9g}")
            for k, v in p.items():
                out[f"{name}_{k}"] = np.asarray(v)
            for k, v in r.items():
                out[f"{name}_ref_{k}"] = np.asarray(v)
            out[f"{name}_ref_stop"] = np.asarray(stop)
            out[f"{name}_ref_applied"] = np.asarray(applied, np.int32)
            out[f"{name}_cfg"] = np.array([cfg[k] for k in ("homog_th", "lambda_lm", "lambda_k", "max_iters", "min_err_change", "min_err")],
                                          np.float64)
            break
        else:
            raise SystemExit(f"{name}: no candidate is far from every threshold")
    assert 6 * int(out["wide_nkf"]) > 120 and out["lines_only_Xw"].shape[0] == 0 and int(out["one_kf_nkf"]) == 1
    np.savez_compressed(os.path.join(HERE, "lba_lm_dev_golden.npz"), **out)


if __name__ == "__main__":
    main()
