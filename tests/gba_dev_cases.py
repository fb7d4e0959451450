"""The inputs of the device-resident global bundle adjustment's tests (tests/test_gba_dev_cpu.py checks on the CPU what each one is,
tests/test_gpu_gba_dev.py runs the device on them).  numpy only.  Every function returns plslam_amd.gba.trajectory_map's dict.

  MAPS     inputs whose rows are a gather's (plslam_amd.gba.map_image's precondition holds): the tests/gba_cases.py inputs the issue
           names, a points-only and a lines-only map, nkf = 1, a landmark seen twice by one keyframe.  They go through the whole
           chain: image -> form_all -> gather -> create_dev -> optimize_dev -> apply_gba.
  COLUMNS  seeded random Vector6i columns whose rows are NOT grouped by landmark (a gather never makes them: map_image refuses
           them, and the CPU test says so); they are uploaded as columns and only the lists are compared.  Observation counts
           0, 1, T - 1, T, T + 1, 3 T + 37 per kind around the distribution's tile T."""
from __future__ import annotations

import numpy as np

from plslam_amd import gba

import gba_cases

T = 1024            # plslam_amd/csrc/distribute_dev.hpp: DIST_TILE
LOOKBACK = 256      # positions per workgroup of the pair enumeration and of the block compaction (gba_plan_dev.hip: GBP_NT)


def lines_only(m):
    """m without its points: the same keyframes, lines and line observations"""
    o = dict(m)
    o["pt_obs"], o["pt_uv"], o["Xw"], o["npt"] = m["pt_obs"][:0], m["pt_uv"][:0], m["Xw"][:0], 0
    return o


TWICE_POINTS, TWICE_LINES = (3, 40), (7,)


def twice(seed=66):
    """ring(7, 60, 20) whose points 3 and 40 and line 7 are seen a second time by the keyframe of their first observation: the
    pairs (a, b) and (b, a) both fall in the diagonal block of that keyframe."""
    m = gba_cases.ring(7, 60, 20, seed)
    rng = np.random.Generator(np.random.PCG64(seed + 1))
    for obs, val, which in (("pt_obs", "pt_uv", TWICE_POINTS), ("ls_obs", "ls_l", TWICE_LINES)):
        rows, vals = m[obs], m[val]
        for j in which:
            sel = np.flatnonzero(rows[:, 1] == j)
            opt = sel[rows[sel, 4] >= 0]
            assert opt.size, "the landmark is seen by an optimised keyframe"
            new = rows[opt[0]].copy()
            new[2] = sel.size
            at = sel[-1] + 1
            rows = np.insert(rows, at, new, axis=0)
            vals = np.insert(vals, at, vals[opt[0]] + 0.25 * rng.standard_normal(vals.shape[1]), axis=0)
        m[obs], m[val] = rows, vals
    return m


MAPS = {
    "chunks": gba_cases.chunks,
    "ragged": gba_cases.ragged,
    "gaps": gba_cases.gaps,
    "nkf16": gba_cases.nkf16,
    "no_obs_keyframe": gba_cases.no_obs_keyframe,
    "no_point_obs": gba_cases.no_point_obs,
    "nan_landmark": gba_cases.nan_landmark,
    "points_only": lambda: gba_cases.points_only(gba_cases.ring(9, 150, 30, 67)),
    "lines_only": lambda: lines_only(gba_cases.ring(9, 150, 30, 68)),
    "nkf1": lambda: gba.trajectory_map(n_kf=2, n_pt=60, n_ls=20, obs_per_lm=2, loop=False, seed=41),
    "twice": twice,
}
# the cases of "same plan, same bits" (max_iters 3)
OPTIMIZE = ("chunks", "ragged", "gaps", "nan_landmark")


def columns(n_pt_obs, n_ls_obs, nkf=5, n_map=9, npt=None, nls=None, seed=1):
    """random columns: unsorted landmark indices, keyframes over all n_map slots (those outside kf_list carry -1); the state
    arrays are there for the dict's shape only (these inputs are never optimised)"""
    rng = np.random.Generator(np.random.PCG64(seed))
    npt = max(1, n_pt_obs // 3) if npt is None else npt
    nls = max(1, n_ls_obs // 3) if nls is None else nls
    kf_list = np.sort(rng.choice(np.arange(1, n_map), nkf, replace=False)).astype(np.int32)
    inv = np.full(n_map, -1, np.int32)
    inv[kf_list] = np.arange(nkf, dtype=np.int32)

    def rows(n, nlm):
        lm = rng.integers(0, max(nlm, 1), n).astype(np.int32)
        kf = rng.integers(0, n_map, n).astype(np.int32)
        return np.stack([lm, lm, np.zeros(n, np.int32), kf, inv[kf], np.ones(n, np.int32)], 1).astype(np.int32).reshape(-1, 6)

    return dict(n_map_kf=n_map, kf_list=kf_list, T_kf_w=np.zeros((n_map, 16)), x_kf=np.zeros((nkf, 6)), Xw=np.zeros((npt, 3)),
                Lw=np.zeros((nls, 6)), pt_obs=rows(n_pt_obs, npt), pt_uv=rng.uniform(0, 700, (n_pt_obs, 2)), ls_obs=rows(n_ls_obs, nls),
                ls_l=rng.standard_normal((n_ls_obs, 3)), npt=npt, nls=nls)


COLUMNS = {f"both_{n}": (lambda n=n: columns(n, n, seed=20 + n % 97)) for n in (0, 1, T - 1, T, T + 1, 3 * T + 37)}
COLUMNS["nkf_70"] = lambda: columns(5000, 1200, nkf=70, n_map=90, seed=31)          # two digits of block keys, many blocks
COLUMNS["nkf_200"] = lambda: columns(6000, 1000, nkf=200, n_map=230, seed=32)       # three digits of block keys
