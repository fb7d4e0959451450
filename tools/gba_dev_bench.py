"""The global bundle adjustment of a map that LIVES ON THE DEVICE (a plslam_map_index), host to host, by two routes, medians of
--reps runs each in the same process (tools/gba_bench.py times plslam_gba_optimize alone and is left as it is):

  device route   plslam_local_map_form_all + _gather + plslam_gba_plan_create_dev, then plslam_gba_optimize_dev +
                 plslam_local_map_apply_gba: nothing but the poses crosses to the host
  host route     download of the image arrays the gather reads, the gather on the host, plslam_gba_plan_create,
                 plslam_gba_optimize, upload of the landmarks into the image.  The host gather is a VECTORISED numpy equivalent of
                 the loops of src/mapHandler.cpp:1995-2092 (an inverse table instead of the linear kf_list search per observation,
                 np.repeat instead of the per-landmark loop): it flatters the host route against the C++ loops of
                 host/local_map.hpp, whose search is O(nkf) per observation.

Sizes as tools/gba_bench.py: G1 400 keyframes / 40 k points / 6 k lines, G2 1500 / 150 k / 20 k, 4 observations per landmark, one
loop.  Before every run the image's landmarks are put back (not timed), so every run optimises the same map.  Prints one JSON line;
--out FILE writes it there too.

    python tools/gba_dev_bench.py [--reps 5] [--sizes G1,G2] [--out profiles/gba_dev_bench.json]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if _ROOT not in sys.path:
    sys.path.insert(0, _ROOT)

import plslam_amd  # noqa: E402
from plslam_amd import gba, synth  # noqa: E402
from plslam_amd import local_map as LM  # noqa: E402

SIZES = {"G1": dict(n_kf=400, n_pt=40000, n_ls=6000), "G2": dict(n_kf=1500, n_pt=150000, n_ls=20000)}
ITERS = 15


def host_gather(img):
    """the GBA gather over host arrays, vectorised -> kf_list, per kind (list, rows (n, 6), observations, X)"""
    kf_valid = img["kf_valid"]
    kf_list = np.flatnonzero(kf_valid).astype(np.int32)
    kf_list = kf_list[kf_list != 0]
    inv = np.full(kf_valid.size, -1, np.int32)
    inv[kf_list] = np.arange(kf_list.size, dtype=np.int32)
    out = [kf_list]
    for K in (img["points"], img["lines"]):
        lst = np.flatnonzero(K["valid"]).astype(np.int32)
        cnt = (K["obs_ptr"][1:] - K["obs_ptr"][:-1])[lst]
        lm = np.repeat(lst, cnt)
        loc = np.repeat(np.arange(lst.size, dtype=np.int32), cnt)
        start = np.repeat(np.cumsum(cnt) - cnt, cnt)
        o = (np.arange(lm.size) - start).astype(np.int32)
        src = K["obs_ptr"][lm] + o
        kf = K["obs_kf"][src]
        rows = np.stack([lm, loc, o, kf, inv[kf], np.ones(lm.size, np.int32)], 1).astype(np.int32)
        out.append((lst, rows, K["obs_val"].reshape(K["obs_kf"].size, -1)[src], K["X"].reshape(K["valid"].size, -1)[lst]))
    return out


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sizes", default="G1,G2")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    ctx = plslam_amd.Context(0)
    c = synth.EUROC
    cam = plslam_amd.make_cam(c["fx"], c["fy"], c["cx"], c["cy"])
    out = {"tool": "gba_dev_bench", "unit": "ms (median, host to host)", "reps": args.reps, "max_iters": ITERS,
           "device": torch.cuda.get_device_name(0), "host_gather": "vectorised numpy equivalent", "cases": []}
    for name in args.sizes.split(","):
        m = gba.trajectory_map(obs_per_lm=4, loop=True, seed=11, **SIZES[name])
        img = gba.map_image(m)
        ix = LM.DeviceMapIndex(img, ctx.device)
        lm = LM.LocalMap(ctx)
        X0 = {k: ix._t[k + ".X"][0].clone() for k in ("points", "lines")}
        names = ["kf_valid", "x_kf_w"] + [f"{k}.{f}" for k in ("points", "lines") for f in ("valid", "X", "obs_ptr", "obs_kf", "obs_val")]

        def restore():
            for k in X0:
                ix._t[k + ".X"][0].copy_(X0[k])
            torch.cuda.synchronize()

        def device_route():
            t = [time.perf_counter()]
            lm.form_all(ix)
            g = lm.gather(ix)
            b = lm.device_buffers()
            plan = plslam_amd.GbaPlan.from_device(ctx, cam, m["n_map_kf"], g["nkf"], b["kf_list"], g["npt"], g["nls"], b["pt_obs"],
                                                  b["pt_obs_uv"], g["n_pt_obs"], b["ls_obs"], b["ls_l_obs"], g["n_ls_obs"])
            t.append(time.perf_counter())
            x = b["X_aux"]
            r = plan.optimize_dev(m["T_kf_w"], x, x + 48 * g["nkf"], x + 48 * g["nkf"] + 24 * g["npt"], max_iters=ITERS)
            lm.apply_gba(plan, ix)
            t.append(time.perf_counter())
            plan.close()
            return r, t

        def host_route():
            t = [time.perf_counter()]
            h = {n: ix._t[n][0].cpu().numpy() for n in names}
            himg = dict(kf_valid=h["kf_valid"], points={f: h["points." + f] for f in ("valid", "X", "obs_ptr", "obs_kf", "obs_val")},
                        lines={f: h["lines." + f] for f in ("valid", "X", "obs_ptr", "obs_kf", "obs_val")})
            kf_list, P, L = host_gather(himg)
            x_kf = h["x_kf_w"].reshape(-1, 6)[kf_list]
            plan = plslam_amd.GbaPlan(ctx, cam, m["n_map_kf"], kf_list, P[0].size, L[0].size, P[1], P[2], L[1], L[2])
            t.append(time.perf_counter())
            r = plan.optimize(m["T_kf_w"], x_kf, P[3], L[3], max_iters=ITERS)
            for key, lst, new in (("points.X", P[0], r["Xw"]), ("lines.X", L[0], r["Lw"])):
                X = h[key].reshape(-1, new.shape[1]).copy()
                X[lst] = new
                ix._t[key][0].copy_(torch.from_numpy(X.reshape(-1)))
            torch.cuda.synchronize()
            t.append(time.perf_counter())
            plan.close()
            return r, t

        case = dict(size=name, nkf=len(m["kf_list"]), npt=m["npt"], nls=m["nls"])
        res = {}
        for route, fn in (("device", device_route), ("host", host_route)):
            ts = []
            for _ in range(args.reps + 1):                   # the first run warms the allocators and is dropped
                restore()
                r, t = fn()
                ts.append(t)
            res[route] = (r, {k: ix.host(k + ".X") for k in ("points", "lines")})
            ts = np.diff(np.array(ts[1:]), axis=1) * 1e3
            case[route + "_plan_ms"] = round(float(np.median(ts[:, 0])), 2)
            case[route + "_optimize_ms"] = round(float(np.median(ts[:, 1])), 2)
            case[route + "_total_ms"] = round(float(np.median(ts.sum(1))), 2)
            case["solves"] = r["n_solves"]
        # the two routes compute the same thing
        same = all(res["device"][1][k].tobytes() == res["host"][1][k].tobytes() for k in ("points", "lines")) and \
            res["device"][0]["T"].tobytes() == res["host"][0]["T"].tobytes()
        case["routes_bit_identical"] = bool(same)
        out["cases"].append(case)
        lm.close()
    ctx.close()
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
