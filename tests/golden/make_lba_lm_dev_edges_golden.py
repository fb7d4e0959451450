#!/usr/bin/env python3
"""tests/golden/make_lba_lm_dev_edges_golden.py -- writes tests/golden/lba_lm_dev_edges_golden.npz: runs of the REFERENCE'S OWN
Levenberg-Marquardt text (oracle.ref_lba_lm: src/mapHandler.cpp:1334-1812 compiled where it lies) on the branches of
plslam_lba_plan_optimize_dev that lba_lm_golden.npz and lba_lm_dev_golden.npz never reach (tests/test_gpu_lba_optimize_dev_edges.py):
    n84, n90     14 and 15 optimised key frames: the one-workgroup solve either side of 64 kB of dynamic LDS
    n120         20 key frames, the last size that solve takes; max_iters = 3 and min_error_change = 0: three solves, the loop runs out
    n120_dx      n120's problem, an exit by the ||DX|| test (:1808)
    wide_max     21 key frames (the padded route), max_iters = 3 and min_error_change = 0: the loop runs out
    wide_dx      wide_max's problem, an exit by the ||DX|| test
    wide_reject  21 key frames from a rough start: a rejected step, then the exit by the first test (:1775)
    wide_retry   wide_reject's problem with min_error_change = 0: the loop goes on behind every rejection -- lambda / k, the SAME
                 err again, the retry applied, lambda * k -- until it runs out
    retry        lba_lm_golden.npz's `reject` with min_error_change = 0: the same on the one-workgroup solve
    iters0, iters2   lba_lm_golden.npz's `main` with max_iters 0 and 2 (the text's first solve lies outside its loop)
Layout as make_lba_lm_dev_golden.py's (<name>_cfg, <name>_ref_*, <name>_ref_stop / _ref_applied).  A case whose problem another
case or another fixture already stores does not store it again: it carries <name>_problem = "<fixture file>:<case>" in place of
the problem's arrays (this generator checks that those arrays are, byte for byte, the problem it ran).
Every decision of every run is >= 1e-6 relative from its threshold (make_lba_lm_dev_golden.far_from_thresholds); a candidate that
is not is dropped for its neighbour, and a case with no candidate left is an error.  ONE exemption: with min_error_change = 0 the
build behind a REJECTED step recomputes the state it had, so its err equals the one before EXACTLY, in the reference and on the
device; that pair -- only when it is bit-equal, only behind a rejection -- is left out of the :1786 gap.  It cannot flip: the
text's test is err > err_prev, the device computes the same sums on the same state twice, and the GPU test asserts the equal bits.
Run where the reference tree is built into oracle/_ref (python tests/golden/make_lba_lm_dev_edges_golden.py); a second run
reproduces the file byte for byte."""
import os
import sys
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
import make_lba_lm_golden as G  # noqa: E402
import make_lba_lm_dev_golden as D  # noqa: E402

OUT = "lba_lm_dev_edges_golden.npz"
CFG_KEYS = ("homog_th", "lambda_lm", "lambda_k", "max_iters", "min_err_change", "min_err")
NKF = dict(n84=14, n90=15, n120=20, n120_dx=20, wide_max=21, wide_dx=21, wide_reject=21, wide_retry=21, retry=4, iters0=6, iters2=6)
STOP = dict(n84=1, n90=1, n120=0, n120_dx=2, wide_max=0, wide_dx=2, wide_reject=1, wide_retry=0, retry=0, iters0=0, iters2=0)


def _smooth(nkf, seed):
    return G.problem(n_kf_map=nkf + 1, n_pt=150, n_ls=40, obs=6, seed=seed, sigma_lm=0.05, sigma_pose=0.01)


def _rough(seed):
    return G.problem(n_kf_map=22, n_pt=120, n_ls=40, obs=3, seed=seed, sigma_lm=2.0, sigma_pose=0.3)


def _retries(applied):
    """a rejected solve with an applied one behind it"""
    return any(a == 0 and b == 1 for a, b in zip(applied, applied[1:]))


def candidates():
    """name -> list of (problem key, problem, cfg, what the run must be), tried in order.  The problem key names the problem: two
    cases with the same key share one stored copy"""
    base = G.CFG
    seeds = (61, 62, 63)
    runs_out = dict(base, max_iters=3, min_err_change=0.0)
    keep_going = dict(base, min_err_change=0.0)
    any_run = lambda stop, applied: True                                         # noqa: E731
    c = {}
    for name, nkf in (("n84", 14), ("n90", 15)):
        c[name] = [((nkf, s), _smooth(nkf, s), dict(base, min_err_change=v), any_run) for s in seeds for v in (3e-4, 1e-4, 1e-3)]
    c["n120"] = [((20, s), _smooth(20, s), runs_out, lambda stop, applied: len(applied) == 3) for s in seeds]
    c["n120_dx"] = [((20, s), _smooth(20, s), dict(base, min_err_change=v), any_run) for s in seeds for v in (1e-4, 2e-4, 5e-5)]
    c["wide_max"] = [((21, s), _smooth(21, s), runs_out, lambda stop, applied: len(applied) == 3) for s in seeds]
    c["wide_dx"] = [((21, s), _smooth(21, s), dict(base, min_err_change=v), any_run) for s in seeds for v in (1.0, 2.0, 4.0)]
    c["wide_reject"] = [(("rough", s), _rough(s), base, lambda stop, applied: applied[-1] == 0) for s in (77, 86)]
    c["wide_retry"] = [(("rough", s), _rough(s), keep_going, lambda stop, applied: _retries(applied)) for s in (77, 86)]
    c["retry"] = [("lba_lm_golden.npz:reject", G.problem(**G.CASES["reject"]), dict(keep_going, max_iters=m),
                   lambda stop, applied: _retries(applied)) for m in (15, 12, 8, 6)]
    main = G.problem(**G.CASES["main"])
    c["iters0"] = [("lba_lm_golden.npz:main", main, dict(base, max_iters=0), lambda stop, applied: len(applied) == 1)]
    c["iters2"] = [("lba_lm_golden.npz:main", main, dict(base, max_iters=2), lambda stop, applied: len(applied) == 2)]
    return c


def _same_problem(p, stored, case):
    return all(np.asarray(v).dtype == stored[f"{case}_{k}"].dtype and np.asarray(v).tobytes() == stored[f"{case}_{k}"].tobytes()
               for k, v in p.items())


def _write(path, out):
    """np.savez_compressed with every member's timestamp fixed: the same arrays give the same bytes"""
    import io
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for k in sorted(out):
            b = io.BytesIO()
            np.lib.format.write_array(b, np.asanyarray(out[k]), allow_pickle=False)
            z.writestr(zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0)), b.getvalue(), zipfile.ZIP_DEFLATED)


def main():
    out, stored, flows = {}, {}, {}
    for name, cands in candidates().items():
        for key, p, cfg, is_the_case in cands:
            r = G.run_ref(p, cfg)
            if r is None:
                raise SystemExit("oracle/_ref/libplslam_ref.so (ref_lba_lm) is not available: build it where the reference tree is")
            stop, applied = D.flow(r, cfg)
            finite = all(np.isfinite(np.asarray(r[k], np.float64)).all() for k in ("X", "lam")) and np.isfinite(r["err"][1:]).all()
            if not finite or stop != STOP[name] or not is_the_case(stop, applied) or \
                    not D.far_from_thresholds(p, cfg, r, equal_behind_a_rejection=True):
                print(f"{name}: candidate dropped (stop {stop}, finite {finite}, applied {applied})")
                continue
            print(f"{name}: N = {r['X'].size}, solves {len(r['lam'])}, iters {r['iters']}, stop {stop}, applied {applied}, err {r['err']}, "
                  f"last err {r['err_last']:.9g} prev {r['err_prev']:.9g}")
            if key == (21, 61) and _same_problem(p, np.load(os.path.join(HERE, "lba_lm_dev_golden.npz")), "wide"):
                key = "lba_lm_dev_golden.npz:wide"         # (that fixture's 21 key frames are this problem)
            if isinstance(key, str):                       # the problem is a case of another fixture
                fixture, case = key.split(":")
                if not _same_problem(p, np.load(os.path.join(HERE, fixture)), case):
                    raise SystemExit(f"{name}: {key} is not the problem that was run")
                out[f"{name}_problem"] = np.array(key)
            elif key in stored:                            # ... or of this one
                out[f"{name}_problem"] = np.array(f"{OUT}:{stored[key]}")
            else:
                stored[key] = name
                for k, v in p.items():
                    out[f"{name}_{k}"] = np.asarray(v)
            for k, v in r.items():
                out[f"{name}_ref_{k}"] = np.asarray(v)
            out[f"{name}_ref_stop"] = np.asarray(stop)
            out[f"{name}_ref_applied"] = np.asarray(applied, np.int32)
            out[f"{name}_cfg"] = np.array([cfg[k] for k in CFG_KEYS], np.float64)
            flows[name] = (key, p, stop, applied, cfg)
            break
        else:
            raise SystemExit(f"{name}: no candidate is far from every threshold")
    # ---- what each case is for ----
    for name, (key, p, stop, applied, cfg) in flows.items():
        assert 6 * p["nkf"] == 6 * NKF[name] and stop == STOP[name], name
    assert flows["n120_dx"][0] == flows["n120"][0] and flows["wide_dx"][0] == flows["wide_max"][0], "the _dx cases run their twin's problem"
    assert flows["wide_retry"][0] == flows["wide_reject"][0], "wide_retry runs wide_reject's problem"
    for name in ("wide_retry", "retry"):
        applied, cfg = flows[name][3], flows[name][4]
        assert _retries(applied) and len(applied) == cfg["max_iters"] and cfg["min_err_change"] == 0.0, name
    assert 0 in flows["wide_reject"][3] and flows["wide_reject"][3][-1] == 0
    assert len(flows["n120"][3]) == len(flows["wide_max"][3]) == 3
    assert (len(flows["iters0"][3]), len(flows["iters2"][3])) == (1, 2)
    _write(os.path.join(HERE, OUT), out)
    print(f"{OUT}: {os.path.getsize(os.path.join(HERE, OUT))} bytes")


if __name__ == "__main__":
    main()
