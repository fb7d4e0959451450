"""Seeded map generator for the global bundle adjustment (plslam_gba_*): a trajectory-shaped map.

synth.local_map gives every landmark random keyframes, so every keyframe pair is covisible and the reduced camera system is
dense.  Here the keyframes lie on a closed circular trajectory and each landmark is seen by a window of consecutive keyframes,
so covisibility is banded; with loop=True windows may wrap past the last keyframe to the first ones (the loop revisit that
links the two ends).  The lists are laid out as MapHandler::globalBundleAdjustment builds them (src/mapHandler.cpp:1995-2099):
keyframe 0 is not optimised (its observations carry keyframe local index -1), every landmark is an unknown with all its
observations, in landmark order."""
from __future__ import annotations

import numpy as np

from .synth import EUROC, se3_exp


def trajectory_map(n_kf=400, n_pt=40000, n_ls=6000, obs_per_lm=4, loop=True, seed=11, noise_px=1.0, pose_noise=0.002,
                   n_unobserved=0, cam=EUROC, step=0.3):
    """-> dict(n_map_kf, kf_list (nkf,), T_kf_w (n_kf, 16) stored poses, x_kf (nkf, 6) the optimised keyframes' x_kf_w,
    Xw (n_pt, 3), Lw (n_ls, 6), pt_obs / ls_obs (n, 6) int32 Vector6i rows, pt_uv (n, 2), ls_l (n, 3)).

    n_unobserved: that many points and lines in the middle of the lists get no observation (their blocks are singular)."""
    assert n_kf >= 2 and 1 <= obs_per_lm <= n_kf
    rng = np.random.Generator(np.random.PCG64(seed))
    fx, fy, cx, cy = cam["fx"], cam["fy"], cam["cx"], cam["cy"]
    W, H = cam["width"], cam["height"]
    # a full circle from 100 keyframes on (the last keyframe comes back next to the first), an arc of that circle below
    R = max(n_kf, 100) * step / (2 * np.pi)
    x_true = np.zeros((n_kf, 6))
    for k in range(n_kf):
        th = k * step / R
        # camera k on a circle in the x-z plane, optical axis (z) along the tangent (sin th, 0, cos th): a rotation by th about y
        x_true[k, 3:] = [0.0, th, 0.0]
        T = se3_exp(np.concatenate([[0.0, 0.0, 0.0], x_true[k, 3:]]))
        T[:3, 3] = [R * (1 - np.cos(th)), 0.0, R * np.sin(th)]
        x_true[k] = np.concatenate([np.linalg.solve(_V(x_true[k, 3:]), T[:3, 3]), x_true[k, 3:]])
    T_true = np.stack([se3_exp(x) for x in x_true])
    # stored poses and the estimates the optimisation starts from: both near the truth, not equal to each other
    x_est = x_true + pose_noise * rng.standard_normal(x_true.shape)
    T_kf_w = np.stack([se3_exp(x_true[k] + pose_noise * rng.standard_normal(6)) for k in range(n_kf)])

    def windows(n):
        last = n_kf if loop else n_kf - obs_per_lm + 1
        s = rng.integers(0, last, n)
        return (s[:, None] + np.arange(obs_per_lm)[None, :]) % n_kf

    def in_front(kfs, n):
        """points 4..12 m in front of the middle keyframe of each window, inside its image"""
        mid = kfs[:, obs_per_lm // 2]
        z = rng.uniform(4.0, 12.0, n)
        u = rng.uniform(0.2 * W, 0.8 * W, n)
        v = rng.uniform(0.2 * H, 0.8 * H, n)
        Pc = np.stack([(u - cx) / fx * z, (v - cy) / fy * z, z], axis=1)
        Tm = T_true[mid]
        return np.einsum("nab,nb->na", Tm[:, :3, :3], Pc) + Tm[:, :3, 3]

    def project(k, X):
        Ti = np.linalg.inv(T_true[k])
        Xc = X @ Ti[:3, :3].T + Ti[:3, 3]
        return np.stack([cx + fx * Xc[:, 0] / Xc[:, 2], cy + fy * Xc[:, 1] / Xc[:, 2]], axis=1)

    def unobserved(n):
        m = np.zeros(n, bool)
        if n_unobserved and n > 2:
            m[rng.choice(np.arange(1, n - 1), size=min(n_unobserved, n - 2), replace=False)] = True
        return m

    kf_pt = windows(n_pt)
    Xw_true = in_front(kf_pt, n_pt) if n_pt else np.zeros((0, 3))
    kf_ls = windows(n_ls)
    P = in_front(kf_ls, n_ls) if n_ls else np.zeros((0, 3))
    Q = P + rng.uniform(-1.0, 1.0, (n_ls, 3)) * np.array([1.0, 1.0, 0.3])
    skip_pt, skip_ls = unobserved(n_pt), unobserved(n_ls)

    def obs_rows(kfs, skip):
        rows = []
        for j in range(kfs.shape[0]):
            if skip[j]:
                continue
            for i, k in enumerate(kfs[j]):
                rows.append((j, j, i, int(k), int(k) - 1, 1))
        return np.array(rows, np.int32).reshape(-1, 6)

    pt_obs, ls_obs = obs_rows(kf_pt, skip_pt), obs_rows(kf_ls, skip_ls)
    uv = np.empty((pt_obs.shape[0], 2))
    l_obs = np.empty((ls_obs.shape[0], 3))
    for k in range(n_kf):
        sel = pt_obs[:, 3] == k
        uv[sel] = project(k, Xw_true[pt_obs[sel, 1]])
        sel = ls_obs[:, 3] == k
        p = project(k, P[ls_obs[sel, 1]])
        q = project(k, Q[ls_obs[sel, 1]])
        if sel.any():
            p = p + noise_px * rng.standard_normal(p.shape)
            q = q + noise_px * rng.standard_normal(q.shape)
            ln = np.cross(np.concatenate([p, np.ones((p.shape[0], 1))], 1), np.concatenate([q, np.ones((q.shape[0], 1))], 1))
            ln /= np.sqrt(ln[:, 0:1] ** 2 + ln[:, 1:2] ** 2)      # normalised 2D line equation (include/mapFeatures.h:93)
            l_obs[sel] = ln
    uv += noise_px * rng.standard_normal(uv.shape)
    Xw = Xw_true + 0.02 * rng.standard_normal(Xw_true.shape)
    Lw = np.concatenate([P, Q], axis=1) + 0.02 * rng.standard_normal((n_ls, 6))
    return dict(n_map_kf=n_kf, kf_list=np.arange(1, n_kf, dtype=np.int32), T_kf_w=T_kf_w.reshape(n_kf, 16),
                x_kf=x_est[1:].copy(), Xw=Xw, Lw=Lw, pt_obs=pt_obs, pt_uv=uv, ls_obs=ls_obs, ls_l=l_obs, npt=n_pt, nls=n_ls)


def covisible_blocks(m):
    """The set of lower covisible keyframe blocks (k1 >= k2, local indices) the map's observations produce."""
    out = set()
    for obs in (m["pt_obs"], m["ls_obs"]):
        if obs.shape[0] == 0:
            continue
        order = np.argsort(obs[:, 1], kind="stable")
        o = obs[order]
        starts = np.flatnonzero(np.r_[True, o[1:, 1] != o[:-1, 1]])
        for a, b in zip(starts, np.r_[starts[1:], o.shape[0]]):
            ks = [int(k) for k in o[a:b, 4] if k >= 0]
            for k1 in ks:
                for k2 in ks:
                    if k1 >= k2:
                        out.add((k1, k2))
    return out


def _V(w):
    th = np.linalg.norm(w)
    if th < 1e-6:
        return np.eye(3)
    s = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]]) / th
    return np.eye(3) + s * (1 - np.cos(th)) / th + s @ s * (th - np.sin(th)) / th
