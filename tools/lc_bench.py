"""Latency of the loop-closure check (K25): plslam_loop_closure_verify (host pointers, one synchronisation) and
plslam_loop_closure_verify_dev (device pointers, timed to a stream synchronisation), against the device calls of the composition it
replaces -- 2 x plslam_match and one plslam_pose_gn_accumulate per Gauss-Newton iteration, through the C ABI with the
arguments prepared in advance -- on the same inputs in the same run.  That is a lower bound of the composition: its host
work (correspondences, the 6 x 6 solves, the SE(3) updates, the outlier pass, the decision) is not timed.  Prints one JSON
line: median microseconds per call.

    python tools/lc_bench.py [--reps 50]

--batch B: the batched check (K54) instead -- B distinct pairs of --size features in one plslam_lc_batch_verify_dev call
against B plslam_loop_closure_verify_dev calls enqueued back to back behind one synchronisation, in the same process on the
same device arrays; the same 2 B match problems as a match plan of their own give the plan's share of the batched call, the
rest is K54's.  Prints one JSON record.

    python tools/lc_bench.py --batch 1024 [--size 1500 200] [--reps 20]
"""
from __future__ import annotations

import argparse
import ctypes
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
from plslam_amd import loop_closure as LC, synth  # noqa: E402


def _median_us(fn, reps, warm=3):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts) * 1e6)


def bench_batch(args):
    import torch
    B, (n_pt, n_ls) = args.batch, args.size
    ctx = plslam_amd.Context(0)
    dev = torch.device("cuda:0")
    p = LC.params()
    keep = []

    def put(a):
        t = torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        keep.append(t)
        return t.data_ptr() if t.numel() else 0

    r0, r1 = [], []
    for k0, k1, _ in LC.keyframe_batch(3, B, sizes=((n_pt, n_ls),), variants=(dict(),)):
        for kf, recs in ((k0, r0), (k1, r1)):
            recs.append(dict({k: put(kf[k]) for k in ("pdesc", "P", "pl", "pt_idx", "ldesc", "sPeP", "le", "ls_idx")},
                             n_pt=n_pt, n_ls=n_ls))
    rsz = ctypes.sizeof(plslam_amd.LcResult)
    res = torch.zeros(B * rsz, dtype=torch.uint8, device=dev)
    pc = torch.zeros((B * n_pt, 4), dtype=torch.int32, device=dev)
    pi = torch.zeros(B * n_pt, dtype=torch.uint8, device=dev)
    lcb = torch.zeros((B * n_ls, 4), dtype=torch.int32, device=dev)
    li = torch.zeros(B * n_ls, dtype=torch.uint8, device=dev)
    res1, pc1, pi1, lcb1, li1 = (torch.zeros_like(t) for t in (res, pc, pi, lcb, li))
    stream = torch.cuda.Stream(dev)
    batch = plslam_amd.LcBatch(ctx, p, B)

    def run_batched():
        batch.verify_dev(r0, r1, res.data_ptr(), pc.data_ptr(), pi.data_ptr(), lcb.data_ptr(), li.data_ptr(),
                         stream=stream.cuda_stream)
        stream.synchronize()

    def run_singles():
        for b in range(B):
            ctx.loop_closure_verify_dev(p, r0[b], r1[b], res1.data_ptr() + b * rsz, pc1.data_ptr() + 16 * b * n_pt,
                                        pi1.data_ptr() + b * n_pt, lcb1.data_ptr() + 16 * b * n_ls, li1.data_ptr() + b * n_ls,
                                        stream=stream.cuda_stream)
        stream.synchronize()

    # the batch's match problems as a plan of their own (tables of its own)
    m12 = torch.zeros(B * (n_pt + n_ls), dtype=torch.int32, device=dev)
    cnt = torch.zeros(2 * B, dtype=torch.int32, device=dev)
    probs = []
    for b in range(B):
        probs.append((r0[b]["pdesc"], n_pt, r1[b]["pdesc"], n_pt, p.min_ratio_12_p, p.mutual, m12.data_ptr() + 4 * b * n_pt,
                      cnt.data_ptr() + 8 * b))
        probs.append((r0[b]["ldesc"], n_ls, r1[b]["ldesc"], n_ls, p.min_ratio_12_l, p.mutual,
                      m12.data_ptr() + 4 * (B * n_pt + b * n_ls), cnt.data_ptr() + 8 * b + 4))
    plan = plslam_amd.MatchPlan(ctx, probs)

    def run_plan():
        plan.run(stream.cuda_stream)
        stream.synchronize()

    t_b = _median_us(run_batched, args.reps)
    t_p = _median_us(run_plan, args.reps)
    t_s = _median_us(run_singles, max(3, args.reps // 4), warm=1)
    same = bool(torch.equal(res.view(-1, rsz)[:, :rsz - 16], res1.view(-1, rsz)[:, :rsz - 16])) and \
        bool(torch.equal(pi, pi1)) and bool(torch.equal(li, li1))
    recs = [plslam_amd.LcResult.from_buffer_copy(x.tobytes()) for x in res.view(-1, rsz).cpu().numpy()]
    r = recs[0].as_dict()
    clk = np.array([x.clk_total for x in recs]) / 100.0            # 100 MHz wall clock
    out = {"tool": "lc_bench", "mode": "batch", "unit": "us (median)", "reps": args.reps, "B": B, "n_pt": n_pt, "n_ls": n_ls,
           "max_iters": p.max_iters, "max_iters_ref": p.max_iters_ref, "systems": r["iters_1"] + r["iters_2"],
           "accepted": int(sum(x.is_lc for x in recs)),
           "batched_us": t_b, "singles_us": t_s, "ratio": t_s / t_b, "per_pair_us": t_b / B, "match_plan_us": t_p,
           "k54_us": t_b - t_p, "match_plan_share": t_p / t_b, "k54_share": 1.0 - t_p / t_b,
           "workgroup_us_min_mean_max": [float(clk.min()), float(clk.mean()), float(clk.max())],
           "workgroup_serial_us_mean": float(np.mean([x.clk_serial for x in recs]) / 100.0),
           "batched_equals_singles": same}
    batch.close()
    ctx.close()
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--batch", type=int, default=0, help="B > 0: the batched check against B single device calls")
    ap.add_argument("--size", type=int, nargs=2, default=(1500, 200), metavar=("N_PT", "N_LS"))
    args = ap.parse_args()
    if args.batch > 0:
        return bench_batch(args)
    import torch
    import lc_ref
    from oracle import oracle as O
    ctx = plslam_amd.Context(0)
    cam = plslam_amd.make_cam(**synth.EUROC)
    ocam = O.make_cam(**synth.EUROC)
    dev = torch.device("cuda:0")
    out = {"tool": "lc_bench", "unit": "us (median)", "reps": args.reps, "cases": []}
    for size in ((1500, 200), (800, 100), (4000, 600)):
        kf0, kf1, _ = LC.keyframe_pair(7 + size[0], *size)
        for iters in ({}, LC.KITTI_ITERS):
            p = LC.params(**iters)
            prm = LC.params_dict(p)
            res = ctx.loop_closure_verify(p, kf0, kf1)[0]

            keep = []

            def put(a):
                t = torch.from_numpy(np.ascontiguousarray(a)).to(dev)
                keep.append(t)
                return t.data_ptr()

            recs = [dict(pdesc=put(k["pdesc"]), P=put(k["P"]), pl=put(k["pl"]), pt_idx=put(k["pt_idx"]), ldesc=put(k["ldesc"]),
                         sPeP=put(k["sPeP"]), le=put(k["le"]), ls_idx=put(k["ls_idx"]), n_pt=size[0], n_ls=size[1])
                    for k in (kf0, kf1)]
            rbuf = torch.zeros(ctypes.sizeof(plslam_amd.LcResult), dtype=torch.uint8, device=dev)
            pc = torch.zeros((size[0], 4), dtype=torch.int32, device=dev)
            pi = torch.zeros(size[0], dtype=torch.uint8, device=dev)
            lcb = torch.zeros((size[1], 4), dtype=torch.int32, device=dev)
            li = torch.zeros(size[1], dtype=torch.uint8, device=dev)
            stream = torch.cuda.Stream(dev)

            def run_dev():
                ctx.loop_closure_verify_dev(p, recs[0], recs[1], rbuf.data_ptr(), pc.data_ptr(), pi.data_ptr(), lcb.data_ptr(),
                                            li.data_ptr(), stream=stream.cuda_stream)
                stream.synchronize()

            # the composition's device calls on the same inputs: 2 x plslam_match and one plslam_pose_gn_accumulate per
            # assembled system, at the T_inc / inlier masks the restatement visits.  Called through the C ABI with every
            # argument prepared outside the timed region: a LOWER bound of the composition, whose host solve, SE(3) update,
            # correspondence building and outlier pass (C++ / Eigen in the reference) only add to it.
            ref = lc_ref.is_loop_closure(prm, ocam, kf0, kf1)
            assert ref["is_lc"] == res["is_lc"]
            P, pl, S, le = ref["corr_inputs"]
            L = plslam_amd.load()
            h = ctx._h
            d0p, d1p = np.ascontiguousarray(kf0["pdesc"]), np.ascontiguousarray(kf1["pdesc"])
            d0l, d1l = np.ascontiguousarray(kf0["ldesc"]), np.ascontiguousarray(kf1["ldesc"])
            m12p, m12l = np.empty(size[0], np.int32), np.empty(size[1], np.int32)
            nm = ctypes.c_int32()
            P, pl, S, le = (np.ascontiguousarray(x) for x in (P, pl, S, le))
            ones_p, ones_l = np.ones(len(P), np.uint8), np.ones(len(S), np.uint8)
            inl_p, inl_l = ref["pt_inlier"].astype(np.uint8), ref["ls_inlier"].astype(np.uint8)
            Ts = [np.ascontiguousarray(t["T"].reshape(16)) for t in ref["trace"]]
            masks = [(ones_p, ones_l) if t["stage"] == 0 else (inl_p, inl_l) for t in ref["trace"]]
            H, g, e, n = np.empty(36), np.empty(6), np.empty(1), np.empty(2, np.int32)
            camr = ctypes.byref(cam)
            calls = [(T.ctypes.data, mp.ctypes.data, ml.ctypes.data) for T, (mp, ml) in zip(Ts, masks)]

            def composition_device():
                L.plslam_match(h, d0p.ctypes.data, size[0], d1p.ctypes.data, size[0], prm["min_ratio_12_p"], prm["mutual"], m12p.ctypes.data,
                               ctypes.byref(nm))
                L.plslam_match(h, d0l.ctypes.data, size[1], d1l.ctypes.data, size[1], prm["min_ratio_12_l"], prm["mutual"], m12l.ctypes.data,
                               ctypes.byref(nm))
                for t, mp, ml in calls:
                    L.plslam_pose_gn_accumulate(h, camr, prm["homog_th"], t, P.ctypes.data, pl.ctypes.data, mp, len(P), S.ctypes.data,
                                                le.ctypes.data, ml, len(S), H.ctypes.data, g.ctypes.data, e.ctypes.data,
                                                n.ctypes.data)

            case = {"n_pt": size[0], "n_ls": size[1], "max_iters": prm["max_iters"], "max_iters_ref": prm["max_iters_ref"],
                    "systems": res["iters_1"] + res["iters_2"], "systems_composition": len(calls), "is_lc": res["is_lc"],
                    "verify_us": _median_us(lambda: ctx.loop_closure_verify(p, kf0, kf1), args.reps),
                    "verify_dev_us": _median_us(run_dev, args.reps),
                    "composition_device_calls_us": _median_us(composition_device, args.reps)}
            r = ctx.loop_closure_verify(p, kf0, kf1)[0]
            case["kernel_us"] = r["clk_total"] / 100.0          # 100 MHz wall clock
            case["kernel_serial_us"] = r["clk_serial"] / 100.0
            out["cases"].append(case)
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
