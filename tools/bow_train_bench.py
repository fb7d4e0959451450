"""Times the vocabulary training host to host: plslam_amd.bow_train.train_vocabulary on the device, and -- where oracle/_ref
carries the DBoW2 wrapper -- the reference's own TemplatedVocabulary::create on this box's CPU (single-threaded, as it is
written).  Uniform random descriptors only: on clustered inputs the reference reads a released matrix (DESIGN.md section 5,
"Training a vocabulary").  Two sizes; the larger is at least 10^6 descriptors with k = 10, L = 5.  Writes medians and p10 / p90.

    python tools/bow_train_bench.py [--reps 5] [--small 20000] [--large 1000000] [--ref-reps 1] [--no-ref-large]
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import plslam_amd  # noqa: E402
from plslam_amd import bow, bow_train  # noqa: E402


def _docs(rng, n, n_docs):
    d = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    cuts = np.linspace(0, n, n_docs + 1).astype(int)
    return [d[a:b] for a, b in zip(cuts[:-1], cuts[1:])]


def _summary(ts):
    ts = np.array(ts)
    return {"median_s": float(np.median(ts)), "p10_s": float(np.percentile(ts, 10)), "p90_s": float(np.percentile(ts, 90)),
            "runs": len(ts)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--ref-reps", type=int, default=1)
    ap.add_argument("--small", type=int, default=20000)
    ap.add_argument("--large", type=int, default=1000000)
    ap.add_argument("--no-ref-large", action="store_true", help="skip the reference at the larger size")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bow_train_bench.json"))
    ap.add_argument("--ref-child", type=int, default=0, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.ref_child:                         # one reference run in a process of its own (it never opens the GPU): prints seconds
        from oracle import oracle as O
        docs = _docs(np.random.default_rng(a.ref_child), a.ref_child, 100)
        t0 = time.perf_counter()
        rv = O.ref_dbow_train(10, 5, bow.BOW_TF_IDF, docs, 1)
        print("REF_SECONDS", time.perf_counter() - t0, flush=True)
        rv.close()
        return
    ref = None
    try:
        from oracle import oracle as O
        if O.ref_lib() is not None and hasattr(O.ref_lib(), "ref_dbow_train"):
            ref = O
    except Exception:
        ref = None
    ctx = plslam_amd.Context(0)
    out = {"tool": "python tools/bow_train_bench.py", "k": 10, "L": 5, "weighting": "TF_IDF", "input": "uniform random descriptors",
           "reference": "TemplatedVocabulary::create from oracle/_ref on this box's CPU, one thread" if ref else "absent", "sizes": {}}
    for name, n in (("small", a.small), ("large", a.large)):
        rng = np.random.default_rng(n)
        docs = _docs(rng, n, 100)
        bow_train.train_vocabulary(ctx, docs[:2], 10, 5, bow.BOW_TF_IDF, 1)          # warm the library
        ts, stats = [], None
        for r in range(a.reps):
            t0 = time.perf_counter()
            voc, stats = bow_train.train_vocabulary(ctx, docs, 10, 5, bow.BOW_TF_IDF, 1)
            ts.append(time.perf_counter() - t0)
        rec = {"n": n, "n_docs": len(docs), "device": _summary(ts), "stats": stats}
        print(json.dumps({name + "_device": rec}), flush=True)
        if ref is not None and not (name == "large" and a.no_ref_large):
            # in a child process: where a group runs empty the reference reads a released matrix and may take its process down
            rs = []
            for r in range(a.ref_reps):
                res = subprocess.run([sys.executable, os.path.abspath(__file__), "--ref-child", str(n)], capture_output=True, text=True)
                got = [ln.split()[1] for ln in res.stdout.splitlines() if ln.startswith("REF_SECONDS")]
                if res.returncode != 0 or not got:
                    rec["reference_failed"] = f"exit status {res.returncode}"
                    break
                rs.append(float(got[0]))
            if rs:
                rec["reference"] = _summary(rs)
                rec["speedup_median"] = rec["reference"]["median_s"] / rec["device"]["median_s"]
        out["sizes"][name] = rec
        print(json.dumps({name: rec}), flush=True)
    ctx.close()
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
