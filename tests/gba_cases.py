"""Seeded global-bundle-adjustment inputs that leave the banded arc of fixed tracks of plslam_amd.gba.trajectory_map, for
tests/test_gba_cpu.py (which checks from the input and the restatement alone that each one reaches what it exists for) and
tests/test_gpu_gba.py (which runs the device on them).  numpy only.  Every function returns trajectory_map's dict.

  rotated        the arc seen from another world frame (T' = G T, X' = G X, observations untouched): general rotation axes
  QUARTER_TURN   the world transform of the frame-invariance test (with world_transform / moved / points_only)
  tumbling       attitude about a precessing axis, the angle from 0 to 2.7; optimised keyframes with w = 0, |w| = 5e-7, 2e-6
  ragged         ~60 keyframes on an inward-looking arc, track lengths from {1, 2, 3, 5, 9, 17, 40} over random keyframes in
                 random list order, landmarks seen by keyframe 0 only and by keyframe 0 plus one other: scattered blocks
  chunks         4 optimised keyframes, blocks of exactly 63 / 64 / 65 / 128 / 129 point pairs, one of 64 point + 65 line
                 pairs, one off-diagonal block of a single pair (CHUNK_BLOCKS)
  gaps           24 map slots, kf_list with gaps, two more fixed keyframes with observations, NaN in every unused slot; and
                 renumbered(), the same map with the slots packed
  nkf16 / nkf32  6 nkf is a multiple of the 32-wide tile: no padding
  degenerate     no_obs_keyframe (the last of 16 optimised keyframes sees nothing), no_point_obs (points, none observed),
                 nan_landmark (one point and one line with a NaN coordinate)

Observations are the projections of the true landmarks through the true poses plus pixel noise, as in trajectory_map, and
every landmark lies in front of every keyframe that sees it -- for the true, the stored and the estimated pose (asserted in
_assemble): these inputs stress the solver, not the rows' clamps.
"""
from __future__ import annotations

import numpy as np

from plslam_amd import gba
from plslam_amd.synth import EUROC

from gba_ref import expmap_se3, inverse_se3, logmap_se3

# the world rotations of the rotated arcs (axis * angle): about x, about z, a generic axis
FRAMES = {
    "about_x": np.array([1.2, 0.0, 0.0]),
    "about_z": np.array([0.0, 0.0, 1.4]),
    "generic": np.array([0.9, 0.3, -1.1]),
}
# the rigid transform of the frame-invariance test: a quarter turn about the world's x axis (y -> z, z -> -y: a signed
# permutation of the axes) and a translation.  Marquardt's damping lambda diag(H) of a landmark block is covariant under such
# a rotation only -- diag(R H R^T) = P diag(H) for a signed permutation R -- so only there do the damped landmark steps turn
# with the frame; under a general rotation (FRAMES) they do not.  The quarter turn keeps ragged's pose angles below 2.1
QUARTER_TURN = np.array([[1.0, 0.0, 0.0, 1.5], [0.0, 0.0, -1.0, -2.0], [0.0, 1.0, 0.0, 0.7], [0.0, 0.0, 0.0, 1.0]])
SMALL_W = (0.0, 5e-7, 2e-6)        # |w| of tumbling's optimised keyframes 0, 1, 2 (map 1, 2, 3)


def moved(G, x_kf, Xw, Lw):
    """The state (x_kf, Xw, Lw) in the world frame G: x' = logmap(G expmap(x)), X' = G X, both end points of a line."""
    G = np.asarray(G, np.float64).reshape(4, 4)
    L = np.asarray(Lw, np.float64).reshape(-1, 2, 3)
    return (np.stack([logmap_se3(G @ expmap_se3(x)) for x in np.asarray(x_kf, np.float64).reshape(-1, 6)]),
            np.asarray(Xw, np.float64).reshape(-1, 3) @ G[:3, :3].T + G[:3, 3], (L @ G[:3, :3].T + G[:3, 3]).reshape(-1, 6))


def world_transform(m, G):
    """The map m in the world frame G: every stored pose and estimate T' = G T, every landmark X' = G X.  What each camera
    sees is the same, so the undamped normal equations are the same up to the rotation of the landmark blocks
    (H_X' = R H_X R^T).  The damped steps are those of m, turned by G, only where R is a signed permutation (QUARTER_TURN)."""
    G = np.asarray(G, np.float64).reshape(4, 4)
    o = dict(m)
    o["T_kf_w"] = np.stack([G @ T.reshape(4, 4) for T in m["T_kf_w"]]).reshape(-1, 16)
    o["x_kf"], o["Xw"], o["Lw"] = moved(G, m["x_kf"], m["Xw"], m["Lw"])
    return o


def points_only(m):
    """m without its lines: the same keyframes, points and point observations"""
    o = dict(m)
    o["ls_obs"], o["ls_l"], o["Lw"], o["nls"] = m["ls_obs"][:0], m["ls_l"][:0], m["Lw"][:0], 0
    return o


def rotated(name, **kw):
    base = dict(n_kf=12, n_pt=300, n_ls=80, obs_per_lm=3, loop=False, seed=43)
    base.update(kw)
    return world_transform(gba.trajectory_map(**base), expmap_se3(np.concatenate([np.zeros(3), FRAMES[name]])))


# ---- from true poses, tracks and true landmarks to the plan's lists ---------------------------------------------------------
def _project(cam, T, X):
    Ti = inverse_se3(T)
    Xc = Ti[:3, :3] @ X + Ti[:3, 3]
    return np.array([cam["cx"] + cam["fx"] * Xc[0] / Xc[2], cam["cy"] + cam["fy"] * Xc[1] / Xc[2]]), Xc[2]


def _assemble(rng, x_true, kf_list, pt_tracks, ls_tracks, Xw_true, PQ_true, n_map=None, slots=None, noise_px=0.5,
              pose_noise=0.002, lm_noise=0.02, exact_w=(), cam=EUROC):
    """x_true (n, 6): the true poses of the n keyframes in use; slots[i]: the map slot of keyframe i (default i);
    kf_list: the map slots that are optimised; tracks: per landmark the keyframes (indices into x_true) that see it, in list
    order.  exact_w: keyframes whose estimate keeps the true rotation part to the bit."""
    n = x_true.shape[0]
    slots = np.arange(n) if slots is None else np.asarray(slots)
    n_map = int(slots.max()) + 1 if n_map is None else n_map
    kf_list = np.asarray(kf_list, np.int32)
    local = {int(s): k for k, s in enumerate(kf_list)}
    T_true = np.stack([expmap_se3(x) for x in x_true])
    x_est = x_true + pose_noise * rng.standard_normal(x_true.shape)
    for k in exact_w:
        x_est[k, 3:] = x_true[k, 3:]
    T_est = np.stack([expmap_se3(x) for x in x_est])
    T_stored = np.stack([expmap_se3(x_true[k] + pose_noise * rng.standard_normal(6)) for k in range(n)])
    T_kf_w = np.full((n_map, 16), np.nan)
    T_kf_w[slots] = T_stored.reshape(n, 16)

    def rows(tracks):
        out = []
        for j, tr in enumerate(tracks):
            for i, k in enumerate(tr):
                out.append((j, j, i, int(slots[k]), local.get(int(slots[k]), -1), 1))
        return np.array(out, np.int32).reshape(-1, 6)

    def seen_from(k, X):
        """pixel and the smallest depth over the three poses of keyframe k"""
        uv, z = _project(cam, T_true[k], X)
        return uv, min(z, _project(cam, T_stored[k], X)[1], _project(cam, T_est[k], X)[1])

    pt_obs, ls_obs = rows(pt_tracks), rows(ls_tracks)
    uv = np.zeros((pt_obs.shape[0], 2))
    l_obs = np.zeros((ls_obs.shape[0], 3))
    zmin, o = np.inf, 0
    for j, tr in enumerate(pt_tracks):
        for k in tr:
            p, z = seen_from(k, Xw_true[j])
            uv[o] = p + noise_px * rng.standard_normal(2)
            zmin, o = min(zmin, z), o + 1
    o = 0
    for j, tr in enumerate(ls_tracks):
        for k in tr:
            p, z1 = seen_from(k, PQ_true[j, :3])
            q, z2 = seen_from(k, PQ_true[j, 3:])
            p = p + noise_px * rng.standard_normal(2)
            q = q + noise_px * rng.standard_normal(2)
            ln = np.cross(np.r_[p, 1.0], np.r_[q, 1.0])
            l_obs[o] = ln / np.sqrt(ln[0] ** 2 + ln[1] ** 2)          # normalised 2D line equation
            zmin, o = min(zmin, z1, z2), o + 1
    assert zmin > 1.0, f"a landmark lies {zmin:.2f} m in front of a keyframe that sees it"
    Xw = Xw_true + lm_noise * rng.standard_normal(Xw_true.shape)
    Lw = PQ_true + lm_noise * rng.standard_normal(PQ_true.shape)
    sel = [int(np.flatnonzero(slots == s)[0]) for s in kf_list]
    return dict(n_map_kf=n_map, kf_list=kf_list, T_kf_w=T_kf_w, x_kf=x_est[sel].copy(), Xw=Xw, Lw=Lw, pt_obs=pt_obs, pt_uv=uv,
                ls_obs=ls_obs, ls_l=l_obs, npt=Xw.shape[0], nls=Lw.shape[0])


def ring_poses(rng, n, arc=2.4, radius=10.0):
    """n cameras on an arc around the origin, each looking at it, rolled about its optical axis by up to 0.4 rad and moved up
    and down: rotation axes in every direction, angles up to about 1.3.  -> x (n, 6)"""
    x = np.zeros((n, 6))
    for k in range(n):
        ph = -arc / 2 + arc * k / max(n - 1, 1)
        c = np.array([radius * np.sin(ph), np.sin(3 * ph), -radius * np.cos(ph)])
        z = -c / np.linalg.norm(c)
        ax = np.cross([0.0, 1.0, 0.0], z)
        ax /= np.linalg.norm(ax)
        R0 = np.stack([ax, np.cross(z, ax), z], 1)
        r = rng.uniform(-0.4, 0.4)
        T = np.eye(4)
        T[:3, :3] = R0 @ np.array([[np.cos(r), -np.sin(r), 0.0], [np.sin(r), np.cos(r), 0.0], [0.0, 0.0, 1.0]])
        T[:3, 3] = c
        x[k] = logmap_se3(T)
    return x


def _ball(rng, n, radius=2.5):
    v = rng.standard_normal((n, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True) * (radius * rng.uniform(0, 1, (n, 1)) ** (1 / 3))


def _segments(rng, n):
    P = _ball(rng, n)
    return np.concatenate([P, P + rng.uniform(-1.0, 1.0, (n, 3)) * np.array([1.0, 1.0, 0.3])], 1)


def _random_tracks(rng, n_lm, n_kf, lengths, window=None):
    """per landmark: a length from `lengths`, that many distinct keyframes (within `window` of a random first one, if given)
    in random list order"""
    out = []
    for _ in range(n_lm):
        L = int(rng.choice(lengths))
        if window is None:
            out.append(rng.choice(n_kf, min(L, n_kf), replace=False))
        else:
            s = int(rng.integers(0, n_kf))
            pool = np.arange(s, min(n_kf, s + window))
            if pool.size < L:
                pool = np.arange(max(0, n_kf - window), n_kf)
            out.append(rng.choice(pool, min(L, pool.size), replace=False))
    return out


def ring(n_kf, n_pt, n_ls, seed, lengths=(2, 3, 4, 6), window=8, **kw):
    """The inward-looking arc with keyframe 0 fixed and random tracks inside a window of keyframes."""
    rng = np.random.Generator(np.random.PCG64(seed))
    x = ring_poses(rng, n_kf)
    return _assemble(rng, x, np.arange(1, n_kf), _random_tracks(rng, n_pt, n_kf, lengths, window),
                     _random_tracks(rng, n_ls, n_kf, lengths, window), _ball(rng, n_pt), _segments(rng, n_ls), **kw)


def nkf16(seed=61):
    return ring(17, 340, 60, seed)


def nkf32(seed=62):
    return ring(33, 660, 120, seed)


RAGGED_LENGTHS = (1, 2, 3, 5, 9, 17, 40)
RAGGED_KF0_ONLY = dict(pt=(3, 100, 250), ls=(2, 40))         # landmarks that only the fixed keyframe 0 sees
RAGGED_KF0_PLUS_ONE = dict(pt=(4, 101, 251), ls=(3, 41))     # keyframe 0 and one optimised keyframe


def ragged(seed=71, n_kf=61, n_pt=420, n_ls=90):
    rng = np.random.Generator(np.random.PCG64(seed))
    x = ring_poses(rng, n_kf)
    tracks = {}
    for kind, n in (("pt", n_pt), ("ls", n_ls)):
        tr = _random_tracks(rng, n, n_kf, RAGGED_LENGTHS)
        for j in RAGGED_KF0_ONLY[kind]:
            tr[j % n] = np.array([0])
        for j in RAGGED_KF0_PLUS_ONE[kind]:
            tr[j % n] = np.array([int(rng.integers(1, n_kf)), 0])
        tracks[kind] = tr
    return _assemble(rng, x, np.arange(1, n_kf), tracks["pt"], tracks["ls"], _ball(rng, n_pt), _segments(rng, n_ls))


# lower block (k1, k2) of local keyframes -> (point pairs, line pairs) that `chunks` is built to give it
CHUNK_PAIRS = {(1, 0): (63, 0), (2, 0): (64, 65), (2, 1): (65, 0), (3, 0): (128, 0), (3, 1): (129, 0), (3, 2): (1, 0)}
CHUNK_BLOCKS = dict(CHUNK_PAIRS)
for _k in range(4):
    CHUNK_BLOCKS[(_k, _k)] = tuple(sum(v[i] for b, v in CHUNK_PAIRS.items() if _k in b) for i in (0, 1))


def chunks(seed=81):
    """Every landmark is seen by exactly two optimised keyframes (each seventh one by the fixed keyframe 0 as well, which
    adds no pair), so off-diagonal block (a, b) holds one pair per landmark of that pair of keyframes and diagonal block
    (a, a) one per landmark that a sees.  The two observations come in either list order."""
    rng = np.random.Generator(np.random.PCG64(seed))
    x = ring_poses(rng, 5, arc=1.2)
    pt, ls = [], []
    for (a, b), (n_p, n_l) in CHUNK_PAIRS.items():
        for out, n in ((pt, n_p), (ls, n_l)):
            for _ in range(n):
                tr = [a + 1, b + 1] if len(out) % 2 else [b + 1, a + 1]
                if len(out) % 7 == 0:
                    tr.insert(1, 0)
                out.append(np.array(tr))
    return _assemble(rng, x, np.arange(1, 5), pt, ls, _ball(rng, len(pt)), _segments(rng, len(ls)))


GAPS_KF_LIST = (1, 2, 4, 7, 8, 13, 14, 19, 21, 22)
GAPS_FIXED = (0, 5, 16)            # map keyframes that are not optimised and have observations (column 4 = -1)
GAPS_N_MAP = 24


def gaps(seed=91, n_pt=260, n_ls=50):
    rng = np.random.Generator(np.random.PCG64(seed))
    slots = np.array(sorted(GAPS_KF_LIST + GAPS_FIXED))
    x = ring_poses(rng, slots.size, arc=2.0)
    return _assemble(rng, x, GAPS_KF_LIST, _random_tracks(rng, n_pt, slots.size, (2, 3, 4, 6)),
                     _random_tracks(rng, n_ls, slots.size, (2, 3, 4)), _ball(rng, n_pt), _segments(rng, n_ls),
                     n_map=GAPS_N_MAP, slots=slots)


def renumbered(m):
    """m with its map slots packed: the slots that kf_list or an observation names, in order, become 0, 1, 2, ...  Only
    column 3 of the observation rows, kf_list and the rows of T_kf_w change: the arithmetic of the solve is the same."""
    used = np.unique(np.concatenate([m["kf_list"], m["pt_obs"][:, 3], m["ls_obs"][:, 3], [0]]))
    new = np.full(m["n_map_kf"], -1, np.int32)
    new[used] = np.arange(used.size, dtype=np.int32)
    o = dict(m)
    o["n_map_kf"] = int(used.size)
    o["kf_list"] = new[m["kf_list"]]
    o["T_kf_w"] = m["T_kf_w"][used].copy()
    for k in ("pt_obs", "ls_obs"):
        o[k] = m[k].copy()
        o[k][:, 3] = new[m[k][:, 3]]
    return o


def tumbling(seed=51, n_kf=26, n_pt=560, n_ls=110):
    """Keyframes 1, 2, 3 have |w| = SMALL_W about general axes (both sides of expmap_se3's 1e-6), to the bit in the estimate;
    from keyframe 4 on the angle grows to 2.7 about the unit axis n(phi) on a cone of half angle 0.9 around y, phi advancing
    0.25 per keyframe.  Whatever its attitude, each camera stands 10 m from the origin and looks at it, up to a metre aside:
    every landmark of the central ball is in front of every keyframe, also the foreign end points the iteration pass's
    stride-3 line block hands to a line.  Tracks of 2-4 keyframes inside a window of six."""
    rng = np.random.Generator(np.random.PCG64(seed))
    x = np.zeros((n_kf, 6))
    for k in range(n_kf):
        ph = 0.4 + 0.25 * k
        axis = np.array([np.sin(0.9) * np.cos(ph), np.cos(0.9), np.sin(0.9) * np.sin(ph)])
        ang = 0.01 if k == 0 else SMALL_W[k - 1] if k <= 3 else 2.7 * (k - 3) / (n_kf - 4)
        x[k, 3:] = ang * axis
        T = expmap_se3(x[k])
        T[:3, 3] = T[:3, :3] @ np.array([np.cos(2.1 * k), np.sin(1.3 * k), -10.0])
        x[k, :3] = logmap_se3(T)[:3]
    return _assemble(rng, x, np.arange(1, n_kf), _random_tracks(rng, n_pt, n_kf, (2, 3, 4), 6),
                     _random_tracks(rng, n_ls, n_kf, (2, 3, 4), 6), _ball(rng, n_pt), _segments(rng, n_ls), exact_w=(1, 2, 3))


# ---- the degenerate family: NaN arithmetic, never a bad address ----------------------------------------------------------------
def no_obs_keyframe(seed=63):
    """nkf16 whose last optimised keyframe sees nothing: its 6 x 6 block of S is zero, the last six pivots of an unpadded
    matrix.  Three points are seen by the fixed keyframe 0 only: they are the unknowns that stay finite."""
    rng = np.random.Generator(np.random.PCG64(seed))
    x = ring_poses(rng, 17)
    tp, tl = _random_tracks(rng, 340, 16, (2, 3, 4, 6), 8), _random_tracks(rng, 60, 16, (2, 3, 4, 6), 8)
    for j in (5, 77, 200):
        tp[j] = np.array([0])
    return _assemble(rng, x, np.arange(1, 17), tp, tl, _ball(rng, 340), _segments(rng, 60))


def no_point_obs(seed=64):
    """Lines only, and 30 points that nothing observes: npt > 0 with an empty point list."""
    m = ring(7, 0, 80, seed)
    rng = np.random.Generator(np.random.PCG64(seed + 1000))
    m["Xw"], m["npt"] = _ball(rng, 30), 30
    return m


NAN_POINT, NAN_LINE = 17, 9


def nan_landmark(seed=65):
    """One point and one line with a NaN coordinate in the initial estimate (nkf = 16: no padding)."""
    m = ring(17, 340, 60, seed)
    m["Xw"][NAN_POINT, 1] = np.nan
    m["Lw"][NAN_LINE, 4] = np.nan
    return m


# the runs that test_gba_cpu.py shows to reach what they are for and test_gpu_gba.py repeats on the device: the input and
# max_iters of the PLSLAM_GBA_STOP_DX exit, and max_iters and lambda_lm of the heavily damped run of tumbling
STOP_DX_CASE, STOP_DX_ITERS = "rotated_about_x", 40
DAMPED_ITERS, DAMPED_LAMBDA = 4, 1e3

# every non-degenerate input of the device tests beyond the arc, by name
INPUTS = {
    "rotated_about_x": lambda: rotated("about_x"),
    "rotated_about_z": lambda: rotated("about_z"),
    "rotated_generic": lambda: rotated("generic"),
    "tumbling": tumbling,
    "ragged": ragged,
    "chunks": chunks,
    "gaps": gaps,
    "nkf16": nkf16,
    "nkf32": nkf32,
}
DEGENERATE = {"no_obs_keyframe": no_obs_keyframe, "no_point_obs": no_point_obs, "nan_landmark": nan_landmark}
# inputs small enough (N < 1000 unknowns) for a dense long-double solve of the whole damped system
SMALL = {
    "rotated_generic": lambda: rotated("generic", n_pt=120, n_ls=24),
    "tumbling": lambda: tumbling(n_kf=12, n_pt=150, n_ls=30),
    "ragged": lambda: ragged(n_kf=21, n_pt=170, n_ls=30),
    "gaps": lambda: gaps(n_pt=160, n_ls=30),
    "nkf16": lambda: ring(17, 200, 30, 61),
}
