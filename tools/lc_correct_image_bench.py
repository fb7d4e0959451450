"""What the loop-closure map correction costs on a device-resident map, host to host (a host clock around a call that ends in a
synchronisation; medians over --reps calls), three routes on the same map:

  image_us        plslam_lc_correct_image: T_corr / corrected / x_kf_w staged, K105-K107 in place on the image and its dir lists
  dev_route_us    the route before it: the anchor CSR of both kinds derived on the host (plslam_amd.local_map.anchor_lists -- an
                  integrator who replays map_*_kf_idx per keyframe instead only has to flatten them, so lists_us is reported apart),
                  its upload with T_corr / corrected, then plslam_lc_correct_map_dev (K50-K53) on the same device arrays
  host_route_us   plslam_lc_correct_map from host arrays (landmarks, dir lists and a prepared CSR up, K50-K53, landmarks back)

at the C3 map (10 000 points, 2 000 lines, about 60 000 observations) and at 1 000 000 landmarks with about 6 observations each.
T_corr is a rotation and translation of 1e-7, so that repeated in-place calls stay finite.  Prints one JSON record.

    python tools/lc_correct_image_bench.py [--reps 30] [--out profiles/lc_correct_image_bench.json]
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
from plslam_amd import capi, local_map as LM, pgo as PG  # noqa: E402
from plslam_amd.capi import _p  # noqa: E402
from plslam_amd.synth import se3_exp  # noqa: E402

WORKLOADS = {
    "c3": dict(n_kf=60, n_pt=10_000, n_ls=2_000, seed=7, max_obs=9),
    "1m": dict(n_kf=60, n_pt=1_000_000, n_ls=20_000, seed=8, max_obs=11),
}
KINDS = ("points", "lines")


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


class _Dirs:
    """the dir lists alone on the device, with the ptr() of a DeviceMapLists"""

    def __init__(self, dirs, dev):
        import torch
        self._t = {f"{k}.dir": torch.from_numpy(np.ascontiguousarray(dirs[k])).to(dev) for k in KINDS}

    def ptr(self, name):
        return self._t[name].data_ptr()


def bench(name, w, reps):
    import torch
    ctx = plslam_amd.Context(0)
    dev = torch.device("cuda", ctx.device)
    rng = np.random.Generator(np.random.PCG64(11))
    m = LM.synthetic_map(**w)
    nk = m["n_map_kf"]
    dirs = {}
    for k in KINDS:
        v = rng.standard_normal((m[k]["obs_kf"].size, 3))
        dirs[k] = v / np.linalg.norm(v, axis=1, keepdims=True)
    T_corr = np.stack([se3_exp(1e-7 * rng.standard_normal(6)) for _ in range(nk)])
    co = np.ones(nk, np.uint8)
    x_new = rng.standard_normal((nk, 6))
    index, lists = LM.DeviceMapIndex(m, ctx.device), _Dirs(dirs, dev)
    med = {k: torch.zeros((max(m[k]["n"], 1), 3), dtype=torch.float64, device=dev) for k in KINDS}
    Tc = np.ascontiguousarray(T_corr.reshape(nk, 16))
    counts = PG.correct_image(ctx, index, T_corr, co, x_new, lists)

    def image():
        PG.correct_image(ctx, index, T_corr, co, x_new, lists)

    parts = dict(lists=[], upload=[], call=[])

    def dev_route():
        t0 = time.perf_counter()
        csr = [LM.anchor_lists(m, k) for k in KINDS]
        t1 = time.perf_counter()
        up = [torch.from_numpy(Tc).to(dev), torch.from_numpy(co).to(dev)]
        args = []
        for k, (ptr, idx) in zip(KINDS, csr):
            up += [torch.from_numpy(ptr).to(dev), torch.from_numpy(idx if idx.size else np.zeros(1, np.int32)).to(dev)]
            args.append(dict(n=m[k]["n"], n_anchor=int(idx.size), n_dir=int(m[k]["obs_kf"].size), anchor_ptr=up[-2].data_ptr(),
                             anchor_idx=up[-1].data_ptr(), valid=index.ptr(f"{k}.valid"), X=index.ptr(f"{k}.X"), med_dir=med[k].data_ptr(),
                             dir_ptr=index.ptr(f"{k}.obs_ptr"), dirs=lists.ptr(f"{k}.dir")))
        torch.cuda.synchronize(dev)
        t2 = time.perf_counter()
        capi.correct_map_dev(ctx, nk, up[0].data_ptr(), up[1].data_ptr(), args[0], args[1])
        t3 = time.perf_counter()
        parts["lists"].append((t1 - t0) * 1e6)
        parts["upload"].append((t2 - t1) * 1e6)
        parts["call"].append((t3 - t2) * 1e6)

    host = []
    for k, dl in zip(KINDS, (3, 6)):
        ptr, idx = LM.anchor_lists(m, k)
        host.append(capi._landmarks(dict(anchor_ptr=ptr, anchor_idx=idx, valid=m[k]["valid"], X=m[k]["X"], med_dir=np.zeros((m[k]["n"], 3)),
                                         dir_ptr=m[k]["obs_ptr"], dirs=dirs[k]), dl))

    def host_route():
        rc = ctx._L.plslam_lc_correct_map(ctx.handle, nk, _p(Tc), _p(co), C.byref(host[0][0]), C.byref(host[1][0]))
        assert rc == 0, rc

    t_img, t_dev, t_host = _times_us([image, dev_route, host_route], reps)
    for v in parts.values():
        del v[:len(v) - reps]                                     # (the warm-up calls)
    assert np.isfinite(index.host("points.X")).all() and np.isfinite(host[0][1]["X"]).all()
    res = dict(image=_stats(t_img), dev_route=_stats(t_dev), host_route=_stats(t_host))
    n_obs = int(m["points"]["obs_kf"].size + m["lines"]["obs_kf"].size)
    moved = 2 * 8 * (3 * counts["n_pt"] + 6 * counts["n_ls"] + 3 * (counts["n_pt_dirs"] + counts["n_ls_dirs"]))
    out = dict(workload=name, n_map_kf=nk, n_points=int(m["points"]["n"]), n_lines=int(m["lines"]["n"]), n_obs=n_obs, counts=counts, reps=reps,
               bytes_read_and_written=moved, **res, dev_route_parts={k: _stats(v) for k, v in parts.items()},
               winner=min(res, key=lambda k: res[k]["median_us"]))
    ctx.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--workloads", nargs="+", default=list(WORKLOADS), choices=list(WORKLOADS))
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    c = plslam_amd.Context(0)
    info = c.device_info()
    c.close()
    rec = dict(tool="lc_correct_image_bench", device=info, results=[bench(n, WORKLOADS[n], a.reps) for n in a.workloads])
    print(json.dumps(rec))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(rec, indent=1) + "\n")


if __name__ == "__main__":
    main()
