#!/usr/bin/env python3
"""tests/golden/make_lba_lm_golden.py -- writes tests/golden/lba_lm_golden.npz: one local bundle adjustment run by the
REFERENCE'S OWN Levenberg-Marquardt text (src/mapHandler.cpp:1334-1812 compiled where it lies: oracle/ref_wrap_lba_lm.cpp via
oracle.ref_lba_lm) on a seeded synthetic local map -- the inputs and, per solve, lambda and err; the final state; the loop's
last values.  Run in the container that holds /root/reference (python tests/golden/make_lba_lm_golden.py); the GPU box only
reads the fixture.  What the fixture pins for plslam_amd/host/lba_rows.hpp LbaPlanSolver::optimize: the first step applied
unconditionally, err / (Npt_obs + Nls_obs) in the first pass and err / (Npt + Nls) in the iterations, lambda GROWING on success,
the stop tests, the pose update through expmap / logmap."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from oracle import oracle as O  # noqa: E402
from plslam_amd import synth  # noqa: E402

CFG = dict(homog_th=1e-7, lambda_lm=0.00001, lambda_k=10.0, max_iters=15, min_err_change=1e-7, min_err=1e-7)   # config/config/config.yaml:28-30, 101-106


def _fixed_heavy(lm, n_kf, seed):
    """every landmark seen twice: once by key frame 0 and once by another one -- half the observations by the key frame that is
    not optimised.  The observations are drawn again as synth.local_map draws them (projection + N(0, 1 px))."""
    rng = np.random.Generator(np.random.PCG64(seed + 2000))
    K = synth.EUROC
    T = lm["T_kf_w"].reshape(-1, 4, 4)

    def project(k, X):
        Ti = np.linalg.inv(T[k])
        Xc = X @ Ti[:3, :3].T + Ti[:3, 3]
        return np.stack([K["cx"] + K["fx"] * Xc[:, 0] / Xc[:, 2], K["cy"] + K["fy"] * Xc[:, 1] / Xc[:, 2]], axis=1)
    for lmk, kfk in (("pt_lm", "pt_kf"), ("ls_lm", "ls_kf")):
        n = lm[lmk].size // 2
        lm[kfk] = np.stack([np.zeros(n, np.int32), 1 + rng.integers(0, n_kf - 1, n).astype(np.int32)], 1).reshape(-1)
    for k in range(n_kf):
        s = lm["pt_kf"] == k
        lm["obs_uv"][s] = project(k, lm["Xw"][lm["pt_lm"][s]]) + rng.standard_normal((int(s.sum()), 2))
        s = lm["ls_kf"] == k
        n = int(s.sum())
        p = project(k, lm["Lw"][lm["ls_lm"][s], :3]) + rng.standard_normal((n, 2))
        q = project(k, lm["Lw"][lm["ls_lm"][s], 3:]) + rng.standard_normal((n, 2))
        ln = np.cross(np.concatenate([p, np.ones((n, 1))], 1), np.concatenate([q, np.ones((n, 1))], 1))
        lm["l_obs"][s] = ln / np.sqrt(ln[:, 0:1] ** 2 + ln[:, 1:2] ** 2)
    return lm


def problem(n_kf_map, n_pt, n_ls, obs, seed, sigma_lm, sigma_pose, fixed_heavy=False):
    """Key frame 0 of the map is never optimised (src/mapHandler.cpp:1231); the others are the local ones, kf_loc = index - 1."""
    lm = synth.local_map(n_kf=n_kf_map, n_pt=n_pt, n_ls=n_ls, obs_per_lm=obs, seed=seed)
    if fixed_heavy:
        lm = _fixed_heavy(lm, n_kf_map, seed)
    rng = np.random.Generator(np.random.PCG64(seed + 1000))
    x = np.stack([O.logmap_se3(T) for T in lm["T_kf_w"].reshape(-1, 4, 4)])
    x[1:] += sigma_pose * rng.standard_normal((n_kf_map - 1, 6)) * np.array([1, 1, 1, 0.2, 0.2, 0.2])
    T_map = np.stack([O.expmap_se3(v) for v in x]).reshape(-1, 16)        # the stored T_kf_w of every key frame
    Xw = lm["Xw"] + sigma_lm * rng.standard_normal(lm["Xw"].shape)
    Lw = lm["Lw"] + sigma_lm * rng.standard_normal(lm["Lw"].shape)
    return dict(n_kf_map=n_kf_map, nkf=n_kf_map - 1, T_map=T_map, x_kf=x[1:].reshape(-1), Xw=Xw, Lw=Lw,
                pt_lm=lm["pt_lm"], pt_kf_map=lm["pt_kf"], pt_kf_loc=lm["pt_kf"] - 1, pt_uv=lm["obs_uv"],
                ls_lm=lm["ls_lm"], ls_kf_map=lm["ls_kf"], ls_kf_loc=lm["ls_kf"] - 1, ls_l=lm["l_obs"])


def run_ref(p, cfg=CFG):
    cam = O.make_cam(synth.EUROC["fx"], synth.EUROC["fy"], synth.EUROC["cx"], synth.EUROC["cy"])
    return O.ref_lba_lm(cam, cfg["homog_th"], cfg["lambda_lm"], cfg["lambda_k"], cfg["max_iters"], cfg["min_err_change"], cfg["min_err"],
                        p["nkf"], p["T_map"], p["x_kf"], p["Xw"], p["Lw"], p["pt_lm"], p["pt_kf_map"], p["pt_kf_loc"], p["pt_uv"],
                        p["ls_lm"], p["ls_kf_map"], p["ls_kf_loc"], p["ls_l"])


CASES = {      # name -> problem arguments
    "main": dict(n_kf_map=7, n_pt=400, n_ls=120, obs=4, seed=31, sigma_lm=0.05, sigma_pose=0.01),      # 6 optimised key frames
    # rough starts (found by a seed search): the second / third iteration's err is ABOVE the one before -- step not applied,
    # lambda /= lambda_k, and the iteration after recomputes the same err and stops at the first test
    "reject": dict(n_kf_map=5, n_pt=120, n_ls=40, obs=3, seed=61, sigma_lm=0.8, sigma_pose=0.3),
    "reject_later": dict(n_kf_map=5, n_pt=120, n_ls=40, obs=3, seed=74, sigma_lm=1.5, sigma_pose=0.15),
    "points_only": dict(n_kf_map=4, n_pt=90, n_ls=0, obs=3, seed=5, sigma_lm=0.05, sigma_pose=0.01),
    # landmark blocks without rank (two views: rank 2 of 3 and of 6), and half the observations by the key frame that is not optimised
    "two_views": dict(n_kf_map=5, n_pt=90, n_ls=30, obs=2, seed=1, sigma_lm=0.05, sigma_pose=0.01),
    "fixed_heavy": dict(n_kf_map=5, n_pt=90, n_ls=30, obs=2, seed=1, sigma_lm=0.05, sigma_pose=0.01, fixed_heavy=True),
}


def main():
    out = {}
    for name, args in CASES.items():
        p = problem(**args)
        r = run_ref(p)
        if r is None:
            raise SystemExit("oracle/_ref/libplslam_ref.so (ref_lba_lm) is not available: build it where /root/reference is")
        print(f"{name}: N = {r['X'].size}, solves {len(r['lam'])}, iters {r['iters']}, err {r['err']}, lambda {r['lam']}, "
              f"last err {r['err_last']:.6g} prev {r['err_prev']:.6g}")
        for k, v in p.items():
            out[f"{name}_{k}"] = np.asarray(v)
        for k, v in r.items():
            out[f"{name}_ref_{k}"] = np.asarray(v)
        if not all(np.isfinite(np.asarray(r[k], np.float64)).all() for k in ("X", "lam", "err_last")):
            raise SystemExit(f"{name}: the reference's run left a non-finite value")
    out["cfg"] = np.array([CFG[k] for k in ("homog_th", "lambda_lm", "lambda_k", "max_iters", "min_err_change", "min_err")], np.float64)
    path = os.path.join(ROOT, "tests", "golden", "lba_lm_golden.npz")
    if os.path.exists(path):                   # a regeneration leaves every array that was there byte for byte as it was
        old = np.load(path)
        for k in old.files:
            a, b = old[k], out[k]
            if a.dtype != b.dtype or a.shape != b.shape or a.tobytes() != b.tobytes():
                raise SystemExit(f"{k} would change: not written")
        print(f"{len(old.files)} arrays of the fixture as it was: byte-identical; {len(out) - len(old.files)} new")
    np.savez_compressed(path, **out)


if __name__ == "__main__":
    main()
