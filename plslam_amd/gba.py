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


def map_image(m):
    """The arrays of a plslam_map_index (the dict plslam_amd.local_map.DeviceMapIndex takes) whose global-BA gather
    (LocalMap.form_all + .gather) gives back a trajectory_map-shaped dict m: kf_list, the six Vector6i columns, pt_uv, ls_l, Xw, Lw.

    Every landmark is valid and an inlier, landmark j of the image is local landmark j; kf_valid marks kf_list plus slot 0;
    obs_ptr counts column 1; x_kf_w holds x_kf at the optimised slots (NaN elsewhere: nothing reads it).  No features: the GBA
    gather reads none.  Precondition (asserted): the rows are grouped by ascending landmark local index, column 0 equals column 1,
    column 2 counts from 0 within the landmark and column 4 is the position of column 3 in kf_list, or -1."""
    n_map = int(m["n_map_kf"])
    kf_list = np.asarray(m["kf_list"], np.int32)
    assert kf_list.size and (np.diff(kf_list) > 0).all() and kf_list[0] >= 1 and kf_list[-1] < n_map, "kf_list: ascending slots above 0"
    kf_valid = np.zeros(n_map, np.uint8)
    kf_valid[0] = 1
    kf_valid[kf_list] = 1
    inv = np.full(n_map, -1, np.int32)
    inv[kf_list] = np.arange(kf_list.size, dtype=np.int32)
    x_kf_w = np.full((n_map, 6), np.nan)
    x_kf_w[kf_list] = np.asarray(m["x_kf"], np.float64).reshape(-1, 6)

    def kind(obs, val, X, dv):
        obs = np.asarray(obs, np.int32).reshape(-1, 6)
        n = X.shape[0]
        lm = obs[:, 1]
        assert ((lm >= 0) & (lm < n)).all() and (np.diff(lm) >= 0).all(), "rows grouped by ascending landmark local index"
        assert (obs[:, 0] == lm).all(), "landmark map index == local index"
        obs_ptr = np.zeros(n + 1, np.int32)
        obs_ptr[1:] = np.cumsum(np.bincount(lm, minlength=n))
        assert (obs[:, 2] == np.arange(obs.shape[0]) - obs_ptr[lm]).all(), "column 2 counts within the landmark"
        assert ((obs[:, 3] >= 0) & (obs[:, 3] < n_map)).all() and (obs[:, 4] == inv[obs[:, 3]]).all(), "column 4 is kf_list's position"
        assert (obs[:, 5] == 1).all()
        return dict(n=n, valid=np.ones(n, np.uint8), inlier=np.ones(n, np.uint8), X=np.asarray(X, np.float64).copy(), obs_ptr=obs_ptr,
                    obs_kf=obs[:, 3].copy(), obs_val=np.asarray(val, np.float64).reshape(-1, dv).copy(),
                    feat_ptr=np.zeros(n_map + 1, np.int32), feat_idx=np.zeros(0, np.int32))

    return dict(n_map_kf=n_map, kf_valid=kf_valid, x_kf_w=x_kf_w, points=kind(m["pt_obs"], m["pt_uv"], np.asarray(m["Xw"]).reshape(-1, 3), 2),
                lines=kind(m["ls_obs"], m["ls_l"], np.asarray(m["Lw"]).reshape(-1, 6), 3))


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
