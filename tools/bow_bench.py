"""Bag-of-words step of MapHandler::addKeyFrame (src/mapHandler.cpp:196-201 -> insertKFBowVectorPL, :3063-3128) on the device:
prints one JSON line.

  insert_us        median latency of plslam_bow_db_insert (host pointers) for one keyframe of 1500 ORB + 200 LBD descriptors
                   against 0 / 100 / 1000 / 10000 earlier live keyframes (PL mode, two k = 10, L = 6 synthetic vocabularies)
  insert_dev_us    the same through plslam_bow_db_insert_dev (device pointers), timed to completion (one stream sync)
  transform_desc_per_s   plslam_bow_transform_dev over 64 sets of 1500 descriptors
  score_pairs_per_s      plslam_bow_db_score: 64 queries against 10000 stored keyframes (host output)

Usage: python tools/bow_bench.py [--reps N] [--levels 0,100,1000,10000]"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import plslam_amd  # noqa: E402
from plslam_amd import bow  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--levels", default="0,100,1000,10000")
    ap.add_argument("--n-orb", type=int, default=1500)
    ap.add_argument("--n-lbd", type=int, default=200)
    a = ap.parse_args()
    import torch
    levels = [int(x) for x in a.levels.split(",")]
    rng = np.random.default_rng(7)
    t0 = time.time()
    vp = bow.synth_vocabulary(rng, k=10, L=6)
    vl = bow.synth_vocabulary(rng, k=10, L=6)
    ctx = plslam_amd.Context(0)
    gp, gl = plslam_amd.BowVocabulary(ctx, vp), plslam_amd.BowVocabulary(ctx, vl)
    setup_s = time.time() - t0
    # 32 keyframe descriptor sets around 8 places (keyframes share words, as consecutive views do)
    places_p = [bow.near_leaf_descriptors(rng, vp, 3000) for _ in range(8)]
    places_l = [bow.near_leaf_descriptors(rng, vl, 400) for _ in range(8)]
    kfs = [(places_p[i % 8][rng.choice(3000, a.n_orb, replace=False)], places_l[i % 8][rng.choice(400, a.n_lbd, replace=False)])
           for i in range(32)]
    stats = (a.n_orb, a.n_lbd, 123.0, 98.0)
    nmax = max(levels)
    db = plslam_amd.BowDatabase(ctx, gp, gl, capacity_hint=nmax + 1)
    dead = np.zeros(nmax, np.uint8)
    for k in range(nmax):                                 # fill: every keyframe stored, nothing scored but the self entry
        pd, ld = kfs[k % 32]
        db.insert(k, pd, ld, stats, dead[:k])
    res = {"tool": "bow_bench", "vocab": "k=10,L=6 synthetic (1111110 nodes) x 2", "n_orb": a.n_orb, "n_lbd": a.n_lbd,
           "reps": a.reps, "setup_s": round(setup_s, 2), "insert_us": {}, "insert_dev_us": {}}
    row = np.full(nmax + 1, np.nan)
    d_row = torch.full((nmax + 1,), float("nan"), dtype=torch.float64, device="cuda")
    dev_sets = [(torch.from_numpy(pd).cuda(), torch.from_numpy(ld).cuda()) for pd, ld in kfs]
    for n in levels:
        alive = np.ones(n, np.uint8)
        d_alive = torch.ones(n + 1, dtype=torch.uint8, device="cuda")
        # the keyframe at index n is inserted again and again: same row length, n live keyframes in front of it
        t = []
        for r in range(a.reps + 3):
            pd, ld = kfs[r % 32]
            s = time.perf_counter()
            db.insert(n, pd, ld, stats, alive, row)
            t.append(time.perf_counter() - s)
        res["insert_us"][str(n)] = round(float(np.median(t[3:])) * 1e6, 1)
        t = []
        for r in range(a.reps + 3):
            dp, dl = dev_sets[r % 32]
            s = time.perf_counter()
            db.insert_dev(n, dp.data_ptr(), a.n_orb, dl.data_ptr(), a.n_lbd, stats, d_alive.data_ptr(), d_row.data_ptr())
            torch.cuda.synchronize()
            t.append(time.perf_counter() - s)
        res["insert_dev_us"][str(n)] = round(float(np.median(t[3:])) * 1e6, 1)
    # transform throughput (device pointers, 64 sets)
    nsets = 64
    d = np.concatenate([kfs[i % 32][0] for i in range(nsets)])
    off = np.arange(nsets + 1, dtype=np.int32) * a.n_orb
    dd, doff = torch.from_numpy(d).cuda(), torch.from_numpy(off).cuda()
    tot = d.shape[0]
    outs = [torch.empty(tot, dtype=torch.int32, device="cuda"), torch.empty(tot, dtype=torch.float64, device="cuda"),
            torch.empty(tot, dtype=torch.int32, device="cuda"), torch.empty(tot, dtype=torch.float64, device="cuda"),
            torch.empty(nsets, dtype=torch.int32, device="cuda")]
    ptrs = [o.data_ptr() for o in outs]
    for _ in range(3):
        gp.transform_dev(dd.data_ptr(), doff.data_ptr(), nsets, tot, a.n_orb, *ptrs)
    torch.cuda.synchronize()
    it = 20
    s = time.perf_counter()
    for _ in range(it):
        gp.transform_dev(dd.data_ptr(), doff.data_ptr(), nsets, tot, a.n_orb, *ptrs)
    torch.cuda.synchronize()
    res["transform_desc_per_s"] = round(tot * it / (time.perf_counter() - s))
    # db_score throughput
    q = np.arange(64, dtype=np.int32) * max(1, nmax // 64)
    db.score(q)
    t = []
    for _ in range(5):
        s = time.perf_counter()
        db.score(q)
        t.append(time.perf_counter() - s)
    res["score_pairs_per_s"] = round(q.size * db.size / float(np.median(t)))
    res["score_pairs"] = int(q.size * db.size)
    res["launches_per_insert"] = "1 H2D copy + 3 kernels + 1 D2H copy, 1 stream synchronisation"
    print(json.dumps(res))
    db.close()
    gp.close()
    gl.close()
    ctx.close()


if __name__ == "__main__":
    main()
