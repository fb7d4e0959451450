"""What keeping desc_list / dir_list / pts_list in the device-resident map costs and saves, per keyframe, host to host (a host
clock around work that ends in a synchronisation; medians over --reps calls):

  carry_us        plslam_map_insert_carry behind a KF <-> KF insert, the keyframe's rows already on the device, to a device
                  synchronisation: the gather by obs_src and the refresh of the touched landmarks
  host_route_us   what an integrator who keeps the lists on the host does instead: plslam_map_insert_download of ev / dir /
                  obs_src, a numpy gather of desc / dir / pts, plslam_median_desc_batched over the touched landmarks' lists, the
                  upload of med_desc.  The re-upload of the lists themselves is NOT counted: a lower bound of that route.
  insert_us       plslam_map_insert_kf2kf itself on this tree
  --parent-lib P  ... and on another build of the library (the parent commit's), in the same process on the same device arrays,
                  alternating parent / this / parent per repetition: what the obs_src store costs K65, against the spread between
                  the parent's own two series

at the C3 map (10 000 points, 2 000 lines, a keyframe of 1500 + 200) and at 1 000 000 landmarks.  Prints one JSON record.

    python tools/map_lists_bench.py [--reps 20] [--parent-lib path/to/libplslam_hip.so] [--out profiles/map_lists_bench.json]
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if _ROOT not in sys.path:
    sys.path.insert(0, _ROOT)

import plslam_amd  # noqa: E402
from plslam_amd import local_map as LM, map_insert as MI, map_lists as ML  # noqa: E402
from plslam_amd.capi import _p  # noqa: E402

WORKLOADS = {
    "c3": dict(map=dict(n_kf=60, n_pt=10_000, n_ls=2_000, seed=7, max_obs=9),
               kf=dict(n_pt=1500, n_ls=200, points=dict(n_new=400, n_exist=700, n_same_lm=20), lines=dict(n_new=50, n_exist=100))),
    "1m": dict(map=dict(n_kf=60, n_pt=1_000_000, n_ls=20_000, seed=8, max_obs=4),
               kf=dict(n_pt=1500, n_ls=200, points=dict(n_new=400, n_exist=700, n_same_lm=20), lines=dict(n_new=50, n_exist=100))),
}


def _times_us(fns, reps, warm=3):
    """the calls of `fns` one after the other per repetition (alternating: they share the machine's moods) -> per fn the samples"""
    for _ in range(warm):
        for f in fns:
            f()
    ts = [[] for _ in fns]
    for _ in range(reps):
        for i, f in enumerate(fns):
            t0 = time.perf_counter()
            f()
            ts[i].append((time.perf_counter() - t0) * 1e6)
    return ts


def _stats(t):
    t = np.asarray(t)
    return dict(median_us=round(float(np.median(t)), 1), p10_us=round(float(np.percentile(t, 10)), 1), p90_us=round(float(np.percentile(t, 90)), 1))


def _raw_insert(lib_path, device, src, dst, kf):
    """plslam_map_insert_kf2kf through a library loaded from lib_path (its own context and handle), on the given device images"""
    L = C.CDLL(lib_path)
    vp, i32 = C.c_void_p, C.c_int32
    L.plslam_ctx_create.argtypes = [C.c_int, C.POINTER(vp)]
    L.plslam_map_insert_create.argtypes = [vp, C.POINTER(vp)]
    L.plslam_map_insert_kf2kf.argtypes = [vp, vp, vp, i32, i32, vp, vp, vp, vp, vp, vp]
    L.plslam_map_insert_destroy.argtypes = [vp]
    L.plslam_ctx_destroy.argtypes = [vp]
    L.plslam_map_insert_destroy.restype = L.plslam_ctx_destroy.restype = None
    ctx, h = vp(), vp()
    assert L.plslam_ctx_create(device, C.byref(ctx)) == 0 and L.plslam_map_insert_create(ctx, C.byref(h)) == 0
    ks, keep = [], []
    for kind in ("points", "lines"):
        s, k = MI._kind_struct(kf.get(kind), "kf2kf")
        ks.append(s)
        keep.append(k)
    row, cnt = np.zeros(src.n_map_kf, np.int32), MI.MapInsertCounts()
    T1, T2 = (np.ascontiguousarray(kf[k], np.float64).reshape(16) for k in ("T1", "T2"))
    dst_copy = MI.MapInsertDst.from_buffer_copy(dst.dst)          # (the call writes the counts into it: not into the caller's)

    def call():
        rc = L.plslam_map_insert_kf2kf(h, C.addressof(src.struct), C.addressof(dst_copy), int(kf["kf1"]), int(kf["kf2"]), _p(T1), _p(T2),
                                       *[C.addressof(k) if k is not None else None for k in ks], _p(row), C.addressof(cnt))
        assert rc == 0, rc

    def close():
        L.plslam_map_insert_destroy(h)
        L.plslam_ctx_destroy(ctx)
    call.keep = (keep, row, cnt, T1, T2, dst_copy)
    return call, close, cnt


def bench(name, w, reps, parent_lib):
    import torch
    ctx = plslam_amd.Context(0)
    dev = torch.device("cuda", ctx.device)
    m0 = LM.synthetic_map(**w["map"])
    m, kf = MI.synthetic_keyframe(m0, w["kf"]["n_pt"], w["kf"]["n_ls"], 3, w["kf"]["points"], w["kf"]["lines"])
    lists = ML.synthetic_lists(m, seed=5, with_med=False)        # (the representatives: on the device, below)
    rows_h = ML.keyframe_rows(kf, seed=6)
    cap = MI.insert_bounds(m, kf, "kf2kf")
    src, dst = LM.DeviceMapIndex(m, ctx.device), MI.DeviceMapImage(m, **cap, device=ctx.device)
    sl, dl = ML.DeviceMapLists(lists, device=ctx.device), ML.DeviceMapLists(None, **cap, device=ctx.device)
    rows = ML.insert_rows(rows_h, ctx.device)
    mi, ml = MI.MapInsert(ctx), ML.MapLists(ctx)
    ml.refresh(src, sl)
    for kind in ("points", "lines"):
        lists[kind]["med_idx"], lists[kind]["med_desc"] = sl.host(f"{kind}.med_idx"), sl.host(f"{kind}.med_desc")
    counts = mi.kf2kf(src, dst, kf)

    def insert():
        mi.kf2kf(src, dst, kf)

    def carry():
        ml.insert_carry(mi, src, sl, dst, dl, rows)
        torch.cuda.synchronize(dev)

    med_host = {k: np.concatenate([lists[k]["med_desc"], np.zeros((cap[t + "_cap"] - lists[k]["med_desc"].shape[0], 32), np.uint8)])
                for k, t in (("points", "pt"), ("lines", "ls"))}

    def host_route():
        rec = mi.download()
        for kind in ("points", "lines"):
            s, ev, L, R = rec[kind]["obs_src"], rec[kind]["ev"], lists[kind], rows_h[kind]
            old = s >= 0
            e, side = (-1 - s[~old]) >> 1, (-1 - s[~old]) & 1
            r = ev[e, 1 + side]
            desc = np.empty((s.size, 32), np.uint8)
            desc[old] = L["desc"][s[old]]
            desc[~old] = np.where(side[:, None] == 0, R["desc1"][np.minimum(r, R["desc1"].shape[0] - 1)], R["desc2"][np.minimum(r, R["desc2"].shape[0] - 1)])
            dirs = np.empty((s.size, 3))
            dirs[old] = L["dir"][s[old]]
            dirs[~old] = rec[kind]["dir"].reshape(-1, 2, 3)[e, side]
            if kind == "lines":
                pts = np.empty((s.size, 4))
                pts[old] = L["pts"][s[old]]
                pts[~old] = np.where(side[:, None] == 0, R["pts1"][np.minimum(r, R["pts1"].shape[0] - 1)], R["pts2"][np.minimum(r, R["pts2"].shape[0] - 1)])
            # the touched landmarks' lists, concatenated: their rows are contiguous in the destination's order
            ptr = dst_ptr[kind]
            touched = np.unique(ev[:, 0])
            lens = ptr[touched + 1] - ptr[touched]
            off = np.zeros(touched.size + 1, np.int32)
            np.cumsum(lens, out=off[1:])
            take = np.repeat(ptr[touched] - off[:-1], lens) + np.arange(int(off[-1]))
            _, gm = ctx.median_desc_batched(np.ascontiguousarray(desc[take]), off)
            med_host[kind][touched] = gm
            up = torch.from_numpy(med_host[kind]).to(dev)
        torch.cuda.synchronize(dev)
        return up

    dst_ptr = {k: dst.host(f"{k}.obs_ptr").astype(np.int64) for k in ("points", "lines")}
    # the two routes leave the same representatives (checked once, outside the timed window)
    carry()
    up = host_route()
    for kind in ("points", "lines"):
        n = dst.struct.points.n if kind == "points" else dst.struct.lines.n
        assert np.array_equal(dl.host(f"{kind}.med_desc")[:n], med_host[kind][:n]), kind
    del up
    t_insert, t_carry, t_host = _times_us([insert, carry, host_route], reps)
    out = dict(workload=name, n_points=int(m["points"]["n"]), n_lines=int(m["lines"]["n"]), n_pt_obs=int(m["points"]["obs_kf"].size),
               n_ls_obs=int(m["lines"]["obs_kf"].size), keyframe=[w["kf"]["n_pt"], w["kf"]["n_ls"]],
               events=dict(points=counts["points"], lines=counts["lines"]), reps=reps,
               insert=_stats(t_insert), carry=_stats(t_carry), host_route=_stats(t_host))
    if parent_lib:
        this_call, this_close, c_this = _raw_insert(plslam_amd.LIB_PATH, ctx.device, src, dst, kf)
        par_call, par_close, c_par = _raw_insert(parent_lib, ctx.device, src, dst, kf)
        ta, tb, tc = _times_us([par_call, this_call, par_call], reps)
        assert (c_this.points.n_events, c_this.lines.n_new) == (c_par.points.n_events, c_par.lines.n_new)
        a, b, c = _stats(ta), _stats(tb), _stats(tc)
        out["insert_ab"] = dict(parent_first=a, this_tree=b, parent_second=c,
                                parent_spread_us=round(abs(a["median_us"] - c["median_us"]), 1),
                                moved_us=round(b["median_us"] - 0.5 * (a["median_us"] + c["median_us"]), 1))
        this_close()
        par_close()
    mi.close()
    ctx.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--workloads", nargs="+", default=list(WORKLOADS), choices=list(WORKLOADS))
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    c = plslam_amd.Context(0)
    info = c.device_info()
    c.close()
    rec = dict(tool="map_lists_bench", device=info, results=[bench(n, WORKLOADS[n], a.reps, a.parent_lib) for n in a.workloads])
    line = json.dumps(rec)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(rec, indent=1) + "\n")


if __name__ == "__main__":
    main()
