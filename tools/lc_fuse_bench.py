"""The loop-closure landmark fusion on the device (plslam_lc_fuse_run) host to host, against what a caller does without it for
the same job when its map image lives on the device: download the image, fuse on host containers, re-pack and upload the whole
image (tools/lc_fuse_host_baseline.cpp, compiled and run by this tool in the same run).  Prints one JSON line.

  sizes    10k: 10 000 point + 2 000 line landmarks, 30 keyframes;  1m: 1 000 000 + 100 000 landmarks, 300 keyframes
  entries  3 of 300 point + 40 line tuples each (75 / 10 per branch A, B, C, D)
  *_us     medians over --reps calls after warm-up calls (the device call: the Python binding's call, one synchronisation,
           graph_delta returned); host_us = download_us + fuse_us + upload_us of the baseline
  check    the baseline's landmark, observation and graph totals against the device call's: the two did the same work

Usage: python tools/lc_fuse_bench.py [--reps N] [--sizes 10k,1m]"""
from __future__ import annotations

import argparse
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import plslam_amd  # noqa: E402
from plslam_amd import lc_fuse as LF  # noqa: E402
from plslam_amd import local_map as LM  # noqa: E402
from plslam_amd import map_insert as MI  # noqa: E402

SIZES = {"10k": dict(n_kf=30, n_pt=10_000, n_ls=2_000), "1m": dict(n_kf=300, n_pt=1_000_000, n_ls=100_000)}


def _median_us(f, reps):
    for _ in range(3):
        f()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        f()
        t.append((time.perf_counter() - t0) * 1e6)
    return round(float(np.median(t)), 1)


def _baseline(exe, m, lc, reps):
    with tempfile.TemporaryDirectory() as d:
        def put(name, a, dt):
            np.ascontiguousarray(a, dt).tofile(os.path.join(d, name + ".bin"))
        put("lc_idx", lc["lc_idx"], np.int32)
        put("T_kf_w", lc["T_kf_w"], np.float64)
        put("kf_valid", m["kf_valid"], np.uint8)
        put("x_kf_w", m["x_kf_w"], np.float64)
        for kind, tag in (("points", "pt"), ("lines", "ls")):
            for f in ("valid", "inlier", "X", "obs_ptr", "obs_kf", "obs_val", "feat_ptr", "feat_idx"):
                put(f"{tag}_{f}", m[kind][f], m[kind][f].dtype)
            put(f"{tag}_tuples", lc[kind]["tuples"], np.int32)
            put(f"{tag}_entry_ptr", lc[kind]["entry_ptr"], np.int32)
            for f in ("P0", "obs0", "P1", "obs1"):
                put(f"{tag}_{f}", lc[kind][f], np.float64)
        r = subprocess.run([exe, d, str(reps)], capture_output=True, text=True, timeout=900)
        if r.returncode != 0:
            raise RuntimeError(r.stderr)
        return json.loads(r.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--sizes", default="10k,1m")
    a = ap.parse_args()
    lib = os.path.dirname(plslam_amd.LIB_PATH)
    tmp = tempfile.mkdtemp()
    exe = os.path.join(tmp, "lc_fuse_host_baseline")
    subprocess.run([shutil.which("g++") or "g++", "-O2", "-std=c++17", "-D__HIP_PLATFORM_AMD__",
                    os.path.join(ROOT, "tools", "lc_fuse_host_baseline.cpp"), "-I" + os.path.join(ROOT, "include"),
                    "-I/opt/rocm/include", "-L" + lib, "-lplslam_hip", "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib",
                    "-L/opt/rocm/lib", "-lamdhip64", "-o", exe], check=True)
    ctx = plslam_amd.Context(0)
    res = {"tool": "lc_fuse_bench", "reps": a.reps, "entries": "3 x (300 + 40)", "sizes": {}}
    mix_pt, mix_ls = dict(n_a=75, n_b=75, n_c=75, n_d=75), dict(n_a=10, n_b=10, n_c=10, n_d=10)
    for name in a.sizes.split(","):
        m = LM.synthetic_map(seed=3, max_obs=4, null_lm_frac=0.0, no_obs_frac=0.0, **SIZES[name])
        nk = m["n_map_kf"]
        entries = ((2, nk - 9, 1), (4, nk - 6, 1), (6, nk - 3, 1))
        lc = LF.synthetic_loop_closure(m, entries, mix_pt, mix_ls, seed=5)
        lf = LF.LcFuse(ctx)
        src = LM.DeviceMapIndex(m, ctx.device)
        dst = MI.DeviceMapImage(m, **LF.fuse_bounds(m, lc), device=ctx.device, blank=0)
        out = dict(SIZES[name], n_pt_obs=int(m["points"]["obs_kf"].size), n_ls_obs=int(m["lines"]["obs_kf"].size))
        got = lf.run(src, dst, lc)
        out["device_us"] = _median_us(lambda: lf.run(src, dst, lc), a.reps)
        out["device_no_graph_us"] = _median_us(lambda: lf.run(src, dst, lc, graph=False), a.reps)
        out["counts"] = got["points"]
        n_after, n_obs_after = int(dst.struct.points.n), int(dst.struct.points.n_obs)
        lf.close()
        del src, dst
        h = _baseline(exe, m, lc, max(3, a.reps // 4) if name == "1m" else a.reps)
        out["host"] = h
        out["host_us"] = round(h["download_us"] + h["fuse_us"] + h["upload_us"], 1)
        out["check"] = bool(h["n_pt_after"] == n_after and h["n_pt_obs_after"] == n_obs_after and h["graph_sum"] == int(got["graph_delta"].sum()))
        res["sizes"][name] = out
    shutil.rmtree(tmp, ignore_errors=True)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
