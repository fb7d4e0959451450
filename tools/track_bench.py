"""What tracking a batch of stereo pairs on the device costs beside the match plan it follows (include/plslam_track.h), by device
events around enqueued work, warmed, medians with p10 / p90 over --reps repetitions:

  plan_ms            the headline step alone: StereoBatchMatcher's match plan with the stereo gates
  plan_track_ms      the same step with TrackBatch.run behind it on the same stream; alternated with plan_ms repetition by
                     repetition, so that both see the same machine: their difference is what the tracker adds to a step
  track_ms           TrackBatch.run alone on tables that stand (K108 + K109 + K110 + K54)
  k54_ms             plslam_relpose_robust_gn_batched_dev alone on the rows and offsets the tracker left
  rows_ms            track_ms - k54_ms per repetition: K108-K110, with their bytes counted from the tables (every table entry
                     and every row array once per kernel that touches it) and the share of the HBM peak that makes
  host_route_bytes   for scale: what the same link costs over PCIe on the host route -- the four match tables, the gate outputs
                     and the disparities down, the packed rows and offsets up

at the headline shape (4096 pairs, 1500 + 200) and at 512 pairs.  The synthetic geometry of synth.stereo_geometry has no common
motion per pair: K54 solves on whatever the tables pair up, which costs what a real pair costs per iteration and runs every
iteration of its budget.  Pair 0's prev frame is the halo, which has no stereo table: it stands in with curr's.

    python tools/track_bench.py [--reps 30] [--pairs 4096 512] [--out profiles/track_bench.json]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if _ROOT not in sys.path:
    sys.path.insert(0, _ROOT)

import plslam_amd  # noqa: E402
from plslam_amd import frontend, loop_closure as LC, synth, track as TR  # noqa: E402

HBM_PEAK = 8.0e12          # bytes / s (MI355X)


def _stats(ms):
    a = np.asarray(ms, np.float64)
    return dict(median=float(np.median(a)), p10=float(np.percentile(a, 10)), p90=float(np.percentile(a, 90)), n=int(a.size))


def _timed(torch, stream, fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    fn()
    b.record(stream)
    return a, b


def bench(ctx, B, n_orb, n_lbd, reps, warm=3):
    import torch
    print(f"[track_bench] {B} pairs: building the stream", flush=True)
    stream = synth.stereo_stream(B, n_orb, n_lbd)
    geom = synth.stereo_geometry(stream)
    bm = frontend.StereoBatchMatcher(ctx, stream, geometry=geom, gates=synth.KITTI_GATES)
    sl = frontend.table_slices(n_orb, n_lbd)
    tb, st, sd = bm.table.data_ptr(), bm.stereo.data_ptr(), bm.stereo_disp.data_ptr()
    kl, gl = bm.g["kp_l"].data_ptr(), bm.g["seg_l"].data_ptr()
    pairs = []
    for i in range(B):
        j = max(i - 1, 0)                   # prev's stereo tables: the ones pair i - 1 wrote for its curr frame
        t_i, s_c, s_p, d_p = tb + 4 * bm.stride * i, st + 4 * (n_orb + n_lbd) * i, st + 4 * (n_orb + n_lbd) * j, sd + 8 * (n_orb + 2 * n_lbd) * j
        pairs.append(TR.track_pair(
            m_pt=t_i + 4 * sl["orb_pc"].start, st_pt_prev=s_p, disp_pt_prev=d_p, kp_prev=kl + 8 * n_orb * i, st_pt_curr=s_c,
            kp_curr=kl + 8 * n_orb * (i + 1), n_pt_prev=n_orb, n_pt_curr=n_orb,
            m_ls=t_i + 4 * sl["lbd_pc"].start, st_ls_prev=s_p + 4 * n_orb, disp_ls_prev=d_p + 8 * n_orb, seg_prev=gl + 16 * n_lbd * i,
            st_ls_curr=s_c + 4 * n_orb, seg_curr=gl + 16 * n_lbd * (i + 1), n_ls_prev=n_lbd, n_ls_curr=n_lbd))
    prm = LC.params(cam=synth.KITTI00)
    tr = TR.TrackBatch(ctx, prm, pairs)
    buf = tr.device_buffers()
    s = bm.stream
    run_plan = lambda: bm.plan.run(s.cuda_stream)                                  # noqa: E731
    run_track = lambda: tr.run(s.cuda_stream)                                      # noqa: E731
    run_k54 = lambda: ctx.relpose_robust_gn_batched_dev(prm, buf.P, buf.pl_obs, buf.pt_off, buf.sPeP, buf.le_obs, buf.ls_off, B,  # noqa: E731
                                                        buf.results, buf.pt_inlier, buf.ls_inlier, stream=s.cuda_stream)
    both = lambda: (run_plan(), run_track())                                       # noqa: E731
    print(f"[track_bench] {B} pairs: warming", flush=True)
    for _ in range(warm):
        both()
        run_k54()
    s.synchronize()
    ev = {k: [] for k in ("plan_ms", "plan_track_ms", "track_ms", "k54_ms")}
    for _ in range(reps):
        ev["plan_ms"].append(_timed(torch, s, run_plan))
        ev["plan_track_ms"].append(_timed(torch, s, both))
        ev["track_ms"].append(_timed(torch, s, run_track))
        ev["k54_ms"].append(_timed(torch, s, run_k54))
        s.synchronize()
    ms = {k: [a.elapsed_time(b) for a, b in v] for k, v in ev.items()}
    ms["rows_ms"] = [t - k for t, k in zip(ms["track_ms"], ms["k54_ms"])]
    ms["added_ms"] = [b - a for a, b in zip(ms["plan_ms"], ms["plan_track_ms"])]
    # the bytes of K108-K110, from the tables as they stand
    dl = tr.download()
    n_pt_rows, n_ls_rows = int(dl["pt_off"][-1]), int(dl["ls_off"][-1])
    table = bm.table.cpu().numpy()
    stereo = bm.stereo.cpu().numpy()
    in_range = 0
    st_prev_ok = 0
    for name, n, o in (("orb_pc", n_orb, 0), ("lbd_pc", n_lbd, n_orb)):
        m = table[:, sl[name]]
        ok = (m >= 0) & (m < n)
        in_range += int(ok.sum())
        prev = stereo[np.maximum(np.arange(B) - 1, 0), o:o + n]
        st_prev_ok += int((ok & (prev >= 0)).sum())
    predicate = 4 * B * (n_orb + n_lbd) + 4 * in_range + 4 * st_prev_ok + B * 2 * 112       # m, st_prev, st_curr, the records
    k108 = predicate + 4 * 2 * B
    k109 = 2 * 4 * 2 * B + 4 * 2 * (B + 1)
    k110 = predicate + 2 * 4 * 2 * B + n_pt_rows * (8 + 8 + 8 + 8 + 24 + 16) + n_ls_rows * (16 + 16 + 16 + 8 + 48 + 24)
    rows_bytes = k108 + k109 + k110
    rows_med = float(np.median(ms["rows_ms"]))
    down = B * (4 * bm.stride + 4 * (n_orb + n_lbd) + 8 * (n_orb + 2 * n_lbd))
    up = n_pt_rows * 40 + n_ls_rows * 72 + 2 * 4 * (B + 1)
    out = dict(pairs=B, n_orb=n_orb, n_lbd=n_lbd, reps=reps, pt_rows=n_pt_rows, ls_rows=n_ls_rows,
               **{k: _stats(v) for k, v in ms.items()},
               rows_bytes=dict(k108=k108, k109=k109, k110=k110, total=rows_bytes),
               rows_share_of_hbm_peak=(rows_bytes / (rows_med * 1e-3)) / HBM_PEAK if rows_med > 0 else None,
               k54_iters_mean=float(np.mean([r["iters_1"] + r["iters_2"] for r in dl["results"]])),
               host_route_bytes=dict(download=down, upload=up, total=down + up))
    tr.close()
    bm.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--pairs", type=int, nargs="+", default=[4096, 512])
    ap.add_argument("--orb", type=int, default=1500)
    ap.add_argument("--lbd", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(_ROOT, "profiles", "track_bench.json"))
    a = ap.parse_args()
    ctx = plslam_amd.Context(0)
    rec = dict(tool="tools/track_bench.py", hbm_peak_bytes_per_s=HBM_PEAK, shapes=[bench(ctx, B, a.orb, a.lbd, max(a.reps, 30)) for B in a.pairs])
    ctx.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
