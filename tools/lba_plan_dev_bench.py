"""The device-built LBA plan and the write-back into the map image, host to host, against the routes a caller has without them.
At the C3 map of synth.local_map(): 10 000 points, 2 000 lines, 60 000 observations, 10 keyframes of which 9 are optimised;
every landmark local.  Both sides of a comparison are timed in the same run; prints one JSON line (--out PATH also writes it).

  (a) plan     device: plslam_lba_plan_create_dev on the gather's device buffers + the Schur lists
               (plslam_lba_plan_list_sizes(prepare_schur), the very builder the first plslam_lba_plan_diag_max runs)
               host:   plslam_local_map_download of the eight columns + plslam_lba_plan_create + the Schur lists the same way
               (plan destruction is outside both timings)
  (b) write-back  device: plslam_local_map_apply_lba
               host:   plslam_lba_plan_get_landmarks + the moved test of LbaPlanSolver::movedLandmarks (numpy, vectorised) +
                       the scatter into X / inlier + upload of both arrays of both kinds
  *_us         medians over --reps calls after 3 warm-up calls, through the Python binding

Usage: python tools/lba_plan_dev_bench.py [--reps N] [--out PATH]"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import plslam_amd  # noqa: E402
from plslam_amd import local_map as LM  # noqa: E402
from plslam_amd import synth  # noqa: E402
from plslam_amd.capi import LbaPlan  # noqa: E402

_COLS = ("pt_lm_loc", "pt_pose_slot", "pt_kf_loc", "pt_obs_uv", "ls_lm_loc", "ls_pose_slot", "ls_kf_loc", "ls_l_obs")


def _median_us(f, reps, after=lambda r: None):
    t = []
    for i in range(reps + 3):
        t0 = time.perf_counter()
        r = f()
        dt = (time.perf_counter() - t0) * 1e6
        after(r)
        if i >= 3:
            t.append(dt)
    return round(float(np.median(t)), 1)


def c3_image():
    """synth.local_map() as a map image: a landmark's observations are consecutive already; every observation has a feature in
    its keyframe that names the landmark"""
    s = synth.local_map()
    n_kf = s["T_kf_w"].shape[0]

    def kind(lm, kf, val, X):
        n = X.shape[0]
        obs_ptr = np.zeros(n + 1, np.int32)
        obs_ptr[1:] = np.cumsum(np.bincount(lm, minlength=n))
        order = np.argsort(kf, kind="stable")
        feat_ptr = np.zeros(n_kf + 1, np.int32)
        feat_ptr[1:] = np.cumsum(np.bincount(kf, minlength=n_kf))
        return dict(n=n, valid=np.ones(n, np.uint8), inlier=np.ones(n, np.uint8), X=X.copy(), obs_ptr=obs_ptr, obs_kf=kf.astype(np.int32),
                    obs_val=val.copy(), feat_ptr=feat_ptr, feat_idx=lm[order].astype(np.int32))
    m = dict(n_map_kf=n_kf, kf_valid=np.ones(n_kf, np.uint8), x_kf_w=np.zeros((n_kf, 6)), row=np.full(n_kf, 100, np.int32),
             points=kind(s["pt_lm"], s["pt_kf"], s["obs_uv"], s["Xw"]), lines=kind(s["ls_lm"], s["ls_kf"], s["l_obs"], s["Lw"]))
    return m, s["T_kf_w"].reshape(n_kf, 16)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert a.reps >= 20
    import torch
    ctx = plslam_amd.Context(0)
    cam = plslam_amd.make_cam(**synth.EUROC)
    m, T = c3_image()
    n = m["n_map_kf"]
    ix = LM.DeviceMapIndex(m, ctx.device)
    lm = LM.LocalMap(ctx)
    lm.form(ix, n - 1, m["row"], 0, 0)
    c = lm.gather(ix)
    assert (c["nkf"], c["npt"], c["nls"], c["n_pt_obs"] + c["n_ls_obs"]) == (n - 1, 10_000, 2_000, 60_000), c
    b = lm.device_buffers()
    nkf, npt, nls = c["nkf"], c["npt"], c["nls"]

    def schur_lists(plan):
        z = (C.c_int32 * 11)()
        rc = plan._L.plslam_lba_plan_list_sizes(plan._h, 1, C.addressof(z))
        assert rc == 0
        return plan

    def plan_dev():
        return schur_lists(LbaPlan.from_device(ctx, cam, 1e-7, n + nkf, nkf, npt, nls, b["pt_lm_loc"], b["pt_pose_slot"], b["pt_kf_loc"],
                                               b["pt_obs_uv"], c["n_pt_obs"], b["ls_lm_loc"], b["ls_pose_slot"], b["ls_kf_loc"],
                                               b["ls_l_obs"], c["n_ls_obs"], b["X_aux"] + 48 * nkf, b["X_aux"] + 8 * (6 * nkf + 3 * npt), n))

    def plan_host():
        g = lm.download(*_COLS)
        slot = np.where(g["pt_kf_loc"] >= 0, n + g["pt_kf_loc"], g["pt_pose_slot"]).astype(np.int32)
        return schur_lists(LbaPlan(ctx, cam, 1e-7, n + nkf, nkf, npt, nls, g["pt_lm_loc"], slot, g["pt_kf_loc"], g["pt_obs_uv"],
                                   g["ls_lm_loc"], g["ls_pose_slot"], g["ls_kf_loc"], g["ls_l_obs"]))
    res = dict(what="device-built LBA plan and write-back against the host routes, C3 map, medians host to host through the Python binding",
               reps=a.reps, nkf=nkf, npt=npt, nls=nls, n_obs=c["n_pt_obs"] + c["n_ls_obs"])
    res["plan_dev_us"] = _median_us(plan_dev, a.reps, lambda p: p.close())
    res["plan_host_us"] = _median_us(plan_host, a.reps, lambda p: p.close())
    # the same lists on both sides, once
    pd, ph = plan_dev(), plan_host()
    ld, lh = pd.lists(), ph.lists()
    assert all(np.array_equal(ld[k], lh[k]) for k in lh), "the device-built lists differ from the host builder's"
    res["n_pairs"] = int(ld["pairs"].shape[0])
    ph.close()
    # ---- (b) the write-back: one LM step moves the landmarks; then the same state is written back reps times
    g = lm.download("kf_list", "pt_list", "ls_list")
    kf_list = g["kf_list"]
    Ts = np.concatenate([T, T[kf_list]])
    pd.set_poses(Ts)
    pd.iterate_resident()
    S, bb, _ = pd.schur(1e-5 * pd.diag_max())
    pd.backsub(np.linalg.solve(S, bb), apply=True, want=False)
    res["apply_dev_us"] = _median_us(lambda: lm.apply_lba(pd, ix, 0.01), a.reps)
    dev = torch.device("cuda", ctx.device)
    img = {k: ix._t[k][0] for k in ("points.X", "points.inlier", "lines.X", "lines.inlier")}
    hX, hI = {"points": m["points"]["X"].copy(), "lines": m["lines"]["X"].copy()}, {"points": m["points"]["inlier"].copy(), "lines": m["lines"]["inlier"].copy()}

    def apply_host():
        Xn, Ln = pd.get_landmarks()
        for kind, lst, new in (("points", g["pt_list"], Xn), ("lines", g["ls_list"], Ln)):
            d = new - hX[kind][lst]
            mv = np.sqrt((d * d).sum(axis=1)) > 0.01
            hI[kind][lst[mv]] = 0
            hX[kind][lst] = new
            img[kind + ".X"].copy_(torch.from_numpy(hX[kind].reshape(-1)))
            img[kind + ".inlier"].copy_(torch.from_numpy(hI[kind]))
        torch.cuda.synchronize(dev)
    res["apply_host_us"] = _median_us(apply_host, a.reps)
    pd.close()
    lm.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
