"""The two map-insertion calls (plslam_map_insert_kf2kf / _map2kf) host to host, against what a caller does without them for the
same job: the host mutation of its containers plus plslam_amd/host/local_map.hpp's re-pack and upload of the whole image
(tools/map_insert_host_baseline.cpp, compiled and run by this tool in the same run).  Prints one JSON line.

  sizes    c3: 10 000 point + 2 000 line landmarks, 30 keyframes;  1m: 1 000 000 + 100 000 landmarks, 300 keyframes
  keyframe 1500 points + 200 lines; KF <-> KF: 500 new + 700 existing point events, 60 + 100 line events; map <-> KF: 150 + 20
  *_us     medians over --reps calls after 3 warm-up calls (the device calls: the Python binding's call, one synchronisation)

Usage: python tools/map_insert_bench.py [--reps N] [--sizes c3,1m]"""
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
sys.path.insert(0, os.path.join(ROOT, "tests"))

import plslam_amd  # noqa: E402
from plslam_amd import local_map as LM  # noqa: E402
from plslam_amd import map_insert as MI  # noqa: E402

SIZES = dict(c3=dict(n_kf=30, n_pt=10_000, n_ls=2_000), **{"1m": dict(n_kf=300, n_pt=1_000_000, n_ls=100_000)})


def _median_us(f, reps):
    for _ in range(3):
        f()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        f()
        t.append((time.perf_counter() - t0) * 1e6)
    return round(float(np.median(t)), 1)


def _baseline(exe, m, kf, kf_b, reps):
    with tempfile.TemporaryDirectory() as d:
        def put(name, a, dt):
            np.ascontiguousarray(a, dt).tofile(os.path.join(d, name + ".bin"))
        put("params", [kf["kf1"], kf["kf2"]], np.int32)
        put("T", np.concatenate([kf["T1"].ravel(), kf["T2"].ravel()]), np.float64)
        put("kf_valid", m["kf_valid"], np.uint8)
        put("x_kf_w", m["x_kf_w"], np.float64)
        for kind, tag in (("points", "pt"), ("lines", "ls")):
            for f in ("valid", "inlier", "X", "obs_ptr", "obs_kf", "obs_val", "feat_ptr", "feat_idx"):
                put(f"{tag}_{f}", m[kind][f], m[kind][f].dtype)
            put(f"{tag}_matches_12", kf[kind]["table"], np.int32)
            put(f"{tag}_map_to_kf", kf_b[kind]["table"], np.int32)
            for f in ("P1", "obs1", "obs2"):
                put(f"{tag}_{f}", kf[kind][f], np.float64)
        r = subprocess.run([exe, d, str(reps)], capture_output=True, text=True, timeout=900)
        if r.returncode != 0:
            raise RuntimeError(r.stderr)
        return json.loads(r.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--sizes", default="c3,1m")
    a = ap.parse_args()
    import map_insert_ref as R
    lib = os.path.dirname(plslam_amd.LIB_PATH)
    tmp = tempfile.mkdtemp()
    exe = os.path.join(tmp, "map_insert_host_baseline")
    subprocess.run([shutil.which("g++") or "g++", "-O2", "-std=c++17", "-D__HIP_PLATFORM_AMD__",
                    os.path.join(ROOT, "tools", "map_insert_host_baseline.cpp"), "-I" + os.path.join(ROOT, "include"),
                    "-I/opt/rocm/include", "-L" + lib, "-lplslam_hip", "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib",
                    "-L/opt/rocm/lib", "-lamdhip64", "-o", exe], check=True)
    ctx = plslam_amd.Context(0)
    res = {"tool": "map_insert_bench", "reps": a.reps, "keyframe": "1500+200", "sizes": {}}
    for name in a.sizes.split(","):
        m0 = LM.synthetic_map(seed=3, max_obs=4, null_lm_frac=0.0, no_obs_frac=0.0, **SIZES[name])
        m, kf = MI.synthetic_keyframe(m0, 1500, 200, 5, dict(n_new=500, n_exist=700), dict(n_new=60, n_exist=100))
        m_a, _ = R.insert_kf2kf(m, kf)
        kf_b = MI.synthetic_map2kf(m_a, kf, seed=6, points=dict(n_events=150), lines=dict(n_events=20))
        mi = MI.MapInsert(ctx)
        src = LM.DeviceMapIndex(m, ctx.device)
        dst = MI.DeviceMapImage(m, **MI.insert_bounds(m, kf, "kf2kf"), device=ctx.device, blank=0)
        dst2 = MI.DeviceMapImage(m, **MI.insert_bounds(m_a, kf_b, "map2kf"), device=ctx.device, blank=0)
        out = dict(SIZES[name], n_pt_obs=int(m["points"]["obs_kf"].size), n_ls_obs=int(m["lines"]["obs_kf"].size))
        out["device_kf2kf_us"] = _median_us(lambda: mi.kf2kf(src, dst, kf), a.reps)
        out["device_map2kf_us"] = _median_us(lambda: mi.map2kf(dst, dst2, kf_b), a.reps)
        mi.close()
        del src, dst, dst2
        out["host"] = _baseline(exe, m, kf, kf_b, max(3, a.reps // 4) if name == "1m" else a.reps)
        h = out["host"]
        out["host_kf2kf_us"] = round(h["kf2kf_mutate_us"] + h["kf2kf_repack_upload_us"], 1)
        out["host_map2kf_us"] = round(h["map2kf_mutate_us"] + h["map2kf_repack_upload_us"], 1)
        res["sizes"][name] = out
    shutil.rmtree(tmp, ignore_errors=True)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
