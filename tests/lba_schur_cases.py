"""Named inputs that take the local BA's Schur step (plslam_amd/csrc/lba_schur.hip K19-K24, schur_landmark in lba_blocks_dev.hpp,
plslam_lba_plan_iterate_schur / _apply_step) off the well-conditioned map of synth.local_map: landmark blocks that lack rank,
blocks with an exact zero on their diagonal, lists on the edges of their chunks and workgroups, depths over three decades -- for
tests/test_lba_schur_cases_cpu.py (what each case reaches, the bound, its cap) and tests/test_gpu_lba_schur_edges.py (the device
against the restatement of tests/lba_schur_ref.py, word for word).  numpy only.

A case is a dict of the arguments of LbaPlan (n_pose_slots, nkf, npt, nls and the eight observation columns) plus the state
T (n_pose_slots, 16), X (npt, 3), L (nls, 6).  Pose slot 0 is the keyframe that is never optimised: kf_loc = slot - 1
(wide_baseline fixes slots 0 and 1).  An observation is the exact projection of its landmark plus N(0, 1 px), as in
synth.local_map.

The cap leaves little of the small lambdas: a block of two views 0.25 m apart has a condition number of 1e6 to 1e7 at
lambda = 1e-3 already, and the bound's second term grows with it.  What DROPPED holds is what the restatement alone says on the
CPU; wide_baseline is the case on which 0, 1e-8 and 1e-5 stay."""
from __future__ import annotations

import functools

import numpy as np

from plslam_amd import synth

K = synth.EUROC
HOMOG_TH = 1e-7
SCH_CHUNK = POSE_CHUNK = 64            # lba_lists.hpp
BACK_PT, BACK_LS = 64, 32              # lba_schur.hip: BACK_WG / 3 points or BACK_WG / 6 lines per workgroup of K23

LAMBDAS = (1e-8, 1e-5, 1e-3, 10.0, 1e6)            # plain multipliers, as plslam_lba_plan_schur takes them
# lambda = 0 only where every landmark block has full rank (test_lba_schur_cases_cpu.py shows that these are all such cases): at 0
# a rank-deficient block's last pivot is rounding noise, and which side of zero it lands on is nobody's contract
FULL_RANK = ("wide_baseline", "points_only")


def _rng(seed):
    return np.random.Generator(np.random.PCG64(seed))


def _poses(rng, n_kf, step=0.25):
    """synth.local_map's trajectory: forward along z, small sideways motion and rotation"""
    T = np.empty((n_kf, 4, 4))
    for k in range(n_kf):
        T[k] = synth.se3_exp(np.concatenate([[0.02 * rng.standard_normal(), 0.02 * rng.standard_normal(), step * k],
                                             0.01 * rng.standard_normal(3)]))
    return T


def _frustum(rng, n, zmin=4.0, zmax=30.0, log=False):
    z = np.exp(rng.uniform(np.log(zmin), np.log(zmax), n)) if log else rng.uniform(zmin, zmax, n)
    u = rng.uniform(0.15 * K["width"], 0.85 * K["width"], n)
    v = rng.uniform(0.15 * K["height"], 0.85 * K["height"], n)
    return np.stack([(u - K["cx"]) / K["fx"] * z, (v - K["cy"]) / K["fy"] * z, z], axis=1)


def _project(T, X):
    Ti = np.linalg.inv(T)
    Xc = X @ Ti[:3, :3].T + Ti[:3, 3]
    return np.stack([K["cx"] + K["fx"] * Xc[:, 0] / Xc[:, 2], K["cy"] + K["fy"] * Xc[:, 1] / Xc[:, 2]], axis=1)


def _views(rng, n_lm, n_kf, obs):
    """synth.local_map's observations: every landmark by `obs` different keyframes -> (lm, kf slot), landmark-major"""
    kf = np.stack([rng.permutation(n_kf)[:obs] for _ in range(n_lm)]).reshape(-1) if n_lm else np.zeros(0, np.int64)
    return np.repeat(np.arange(n_lm), obs), kf


def build(T, X, L, pt_lm, pt_kf, ls_lm, ls_kf, seed, noise_px=1.0, n_fixed=1):
    """The case of the poses T (n_kf, 4, 4), the landmarks X / L and the observations (landmark, keyframe slot); the first n_fixed
    slots are not optimised."""
    rng = _rng(1000 + seed)
    i32 = lambda a: np.ascontiguousarray(a, np.int32).reshape(-1)                   # noqa: E731
    pt_lm, pt_kf, ls_lm, ls_kf = i32(pt_lm), i32(pt_kf), i32(ls_lm), i32(ls_kf)
    n_kf = T.shape[0]
    X, L = np.ascontiguousarray(X, np.float64).reshape(-1, 3), np.ascontiguousarray(L, np.float64).reshape(-1, 6)
    uv, lo = np.empty((pt_lm.size, 2)), np.empty((ls_lm.size, 3))
    for k in range(n_kf):
        s = pt_kf == k
        uv[s] = _project(T[k], X[pt_lm[s]]) + noise_px * rng.standard_normal((int(s.sum()), 2))
        s = ls_kf == k
        n = int(s.sum())
        p = _project(T[k], L[ls_lm[s], :3]) + noise_px * rng.standard_normal((n, 2))
        q = _project(T[k], L[ls_lm[s], 3:]) + noise_px * rng.standard_normal((n, 2))
        ln = np.cross(np.concatenate([p, np.ones((n, 1))], 1), np.concatenate([q, np.ones((n, 1))], 1))
        lo[s] = ln / np.sqrt(ln[:, 0:1] ** 2 + ln[:, 1:2] ** 2)
    loc = lambda kf: np.maximum(kf - n_fixed, -1).astype(np.int32)                  # noqa: E731
    return dict(n_pose_slots=n_kf, nkf=n_kf - n_fixed, npt=X.shape[0], nls=L.shape[0], pt_lm=pt_lm, pt_slot=pt_kf, pt_kf_loc=loc(pt_kf),
                pt_obs_uv=uv, ls_lm=ls_lm, ls_slot=ls_kf, ls_kf_loc=loc(ls_kf), ls_l_obs=lo,
                T=np.ascontiguousarray(T.reshape(n_kf, 16)), X=X, L=L)


def _lines(rng, n, **kw):
    P = _frustum(rng, n, **kw)
    return np.concatenate([P, P + rng.uniform(-1.0, 1.0, (n, 3)) * np.array([1.0, 1.0, 0.3]) * P[:, 2:3] / 10.0], axis=1)


def local(n_kf, n_pt, n_ls, obs, seed):
    """synth.local_map's family, through this file's builder"""
    rng = _rng(seed)
    T = _poses(rng, n_kf)
    X, L = _frustum(rng, n_pt), _lines(rng, n_ls)
    return build(T, X, L, *_views(rng, n_pt, n_kf, obs), *_views(rng, n_ls, n_kf, obs), seed)


def one_view():
    """one observation per landmark; landmarks 0, 3, 6, ... by the fixed keyframe (slot 0) only"""
    rng = _rng(12)
    T = _poses(rng, 4)
    X, L = _frustum(rng, 90), _lines(rng, 30)
    kf = lambda n: np.where(np.arange(n) % 3 == 0, 0, rng.integers(1, 4, n))           # noqa: E731
    return build(T, X, L, np.arange(90), kf(90), np.arange(30), kf(30), 12)


def on_the_axis():
    """R = I exactly and the translations along z; points 0, 1, 2 at (0, 0, z) and line 0 with both end points on the axis: the
    landmark's camera-frame x and y are exact zeros in every view, so the z column of its Jacobian rows is"""
    rng = _rng(13)
    T = np.tile(np.eye(4), (4, 1, 1))
    T[:, 2, 3] = 0.25 * np.arange(4)
    X, L = _frustum(rng, 40), _lines(rng, 12)
    X[:3] = [[0.0, 0.0, 6.0], [0.0, 0.0, 11.5], [0.0, 0.0, 23.0]]
    L[0] = [0.0, 0.0, 7.0, 0.0, 0.0, 9.5]
    return build(T, X, L, *_views(rng, 40, 4, 3), *_views(rng, 12, 4, 3), 13)


def twice_by_one_keyframe():
    """every landmark: two observations by keyframe a, one by keyframe b != a (a or b may be the fixed one)"""
    rng = _rng(14)
    T = _poses(rng, 4)
    X, L = _frustum(rng, 60), _lines(rng, 20)

    def views(n):
        ab = np.stack([rng.permutation(4)[:2] for _ in range(n)])
        return np.repeat(np.arange(n), 3), np.stack([ab[:, 0], ab[:, 1], ab[:, 0]], 1).reshape(-1)
    return build(T, X, L, *views(60), *views(20), 14)


def strangers():
    """optimised keyframes 0 and 1 (slots 1, 2) share no landmark: even landmarks by slots {0, 1, 3}, odd ones by {0, 2, 3}"""
    rng = _rng(15)
    T = _poses(rng, 4)
    X, L = _frustum(rng, 60), _lines(rng, 20)

    def views(n):
        kf = np.where((np.arange(n) % 2 == 0)[:, None], [0, 1, 3], [0, 2, 3])
        return np.repeat(np.arange(n), 3), kf.reshape(-1)
    return build(T, X, L, *views(60), *views(20), 15)


def block_63_64_65():
    """Six optimised keyframes.  0, 1, 2: blocks (0,1), (0,2), (1,2) hold 63, 64, 65 point pairs and 3 line pairs each, so 1, 0 and
    63 null pairs stand between a block's point pairs and its line chunk (the diagonal blocks: 127, 128, 129 point pairs).  3, 4, 5:
    seen with the fixed keyframe only, 63, 64 and 65 observations each (60, 61, 62 points and 3 lines)."""
    rng = _rng(16)
    T = _poses(rng, 7)
    pl, pk, ll, lk = [], [], [], []
    npt = nls = 0
    for (a, b), n in (((1, 2), 63), ((1, 3), 64), ((2, 3), 65)):
        pl += [np.repeat(npt + np.arange(n), 2)]; pk += [np.tile([a, b], n)]; npt += n
        ll += [np.repeat(nls + np.arange(3), 2)]; lk += [np.tile([a, b], 3)]; nls += 3
    for s, n in ((4, 60), (5, 61), (6, 62)):
        pl += [np.repeat(npt + np.arange(n), 2)]; pk += [np.tile([0, s], n)]; npt += n
        ll += [np.repeat(nls + np.arange(3), 2)]; lk += [np.tile([0, s], 3)]; nls += 3
    return build(T, _frustum(rng, npt), _lines(rng, nls), np.concatenate(pl), np.concatenate(pk), np.concatenate(ll),
                 np.concatenate(lk), 16)


def chunks_33():
    """two optimised keyframes, 2049 points seen by both: 33 chunks of pairs in block (0, 1); with its 5 lines (seen with the fixed
    keyframe) each keyframe has 2054 observations: 33 chunks.  The second round of 32 in k_schur_finish."""
    rng = _rng(17)
    T = _poses(rng, 3)
    n = 32 * SCH_CHUNK + 1
    return build(T, _frustum(rng, n), _lines(rng, 10), np.repeat(np.arange(n), 2), np.tile([1, 2], n), np.repeat(np.arange(10), 2),
                 np.stack([np.zeros(10, int), 1 + np.arange(10) % 2], 1).reshape(-1), 17)


def depths():
    """landmarks from 0.5 m to 500 m (log-uniform; the keyframes 5 cm apart, so the nearest stay in front of all of them): a
    landmark block scales with 1 / depth^2, a cross block with it"""
    rng = _rng(18)
    T = _poses(rng, 5, step=0.05)
    X, L = _frustum(rng, 120, 0.5, 500.0, log=True), _lines(rng, 40, zmin=0.5, zmax=500.0, log=True)
    X[:2, 2], X[2:4, 2] = [0.5, 0.55], [500.0, 480.0]
    X[:4, :2] = X[:4, 2:3] * [[0.1, -0.05]]
    return build(T, X, L, *_views(rng, 120, 5, 3), *_views(rng, 40, 5, 3), 18)


def wide_baseline():
    """points only, four views each from keyframes a metre apart sideways, depths 4 to 10 m: every block of full rank and well
    conditioned -- the case that keeps lambda = 0 and the small lambdas under the cap.  Slots 0 AND 1 are fixed (keyframes outside
    the local window): one fixed keyframe leaves the scale of a map of points free, and the undamped system singular."""
    rng = _rng(22)
    T = _poses(rng, 5)
    T[:, 0, 3] += 1.0 * np.arange(5)
    X = _frustum(rng, 120, 4.0, 10.0)
    X[:, 0] += 2.0
    return build(T, X, np.zeros((0, 6)), *_views(rng, 120, 5, 4), np.zeros(0, int), np.zeros(0, int), 22, n_fixed=2)


CASES = {
    "wide_baseline": wide_baseline,
    "two_views": lambda: local(4, 90, 40, 2, 11),
    "one_view": one_view,
    "on_the_axis": on_the_axis,
    "twice_by_one_keyframe": twice_by_one_keyframe,
    "strangers": strangers,
    "block_63_64_65": block_63_64_65,
    "chunks_33": chunks_33,
    **{f"backsub_{p}_{l}": (lambda p=p, l=l: local(3, p, l, 2, 100 + p + l)) for p in (63, 64, 65) for l in (31, 32, 33)},
    "depths": depths,
    # the sizes of test_gpu_lba.py::test_schur_step_edge_shapes
    "points_only": lambda: local(6, 300, 0, 4, 19),
    "lines_only": lambda: local(6, 0, 90, 4, 20),
    "one_optimised_keyframe": lambda: local(2, 200, 40, 2, 21),
}

# what each case exists for; test_lba_schur_cases_cpu.py::test_cases_reach_what_they_are_for asserts every entry
REACHES = {
    "wide_baseline": ("no_lines", "every_block_of_full_rank", "lambda_zero_under_the_cap"),
    "two_views": ("pt_rank_2", "ls_rank_2"),
    "one_view": ("pt_rank_1", "ls_rank_1", "a_third_by_the_fixed_keyframe_only"),
    "on_the_axis": ("rotations_are_identity", "zero_on_the_diagonal_of_a_nonzero_block_x4", "four_singular_at_every_lambda"),
    "twice_by_one_keyframe": ("both_orders_in_a_diagonal_block",),
    "strangers": ("a_block_without_pairs",),
    "block_63_64_65": ("point_pairs_63_64_65", "null_pairs_1_0_63", "keyframes_of_63_64_65"),
    "chunks_33": ("block_of_33_chunks", "keyframes_of_33_chunks"),
    **{f"backsub_{p}_{l}": (f"workgroups_{p}_{l}",) for p in (63, 64, 65) for l in (31, 32, 33)},
    "depths": ("depths_over_three_decades", "blocks_over_six_decades"),
    "points_only": ("no_lines", "every_block_of_full_rank"),
    "lines_only": ("no_points",),
    "one_optimised_keyframe": ("one_block",),
}

# The lambdas the cap takes out (test_lba_schur_cases_cpu.py::test_the_cap): bound_e <= 1e-5 max|S_ld| must hold for every entry of
# S of every case x lambda kept.  Measured on the restatement alone, on the CPU.
_SMALL, _SMALLER = (1e-8, 1e-5), (1e-8, 1e-5, 1e-3)
DROPPED = {
    "two_views": _SMALLER, "one_view": _SMALLER, "on_the_axis": _SMALL, "twice_by_one_keyframe": _SMALL, "strangers": _SMALL,
    "block_63_64_65": _SMALL, "chunks_33": _SMALL, "backsub_63_32": _SMALL,
    **{f"backsub_{p}_{l}": _SMALLER for p in (63, 64, 65) for l in (31, 32, 33) if (p, l) != (63, 32)},
    "depths": _SMALL, "points_only": (0.0,) + _SMALL, "lines_only": _SMALL, "one_optimised_keyframe": _SMALLER,
}


def lambdas(name):
    """the lambda table of a case: LAMBDAS (and 0 where every block has full rank) less what the cap drops"""
    table = ((0.0,) if name in FULL_RANK else ()) + LAMBDAS
    return tuple(x for x in table if x not in DROPPED.get(name, ()))


@functools.lru_cache(maxsize=None)
def case(name):
    return CASES[name]()


PLAN_COLUMNS = ("pt_lm", "pt_slot", "pt_kf_loc", "pt_obs_uv", "ls_lm", "ls_slot", "ls_kf_loc", "ls_l_obs")


def plan_args(c):
    return (c["n_pose_slots"], c["nkf"], c["npt"], c["nls"]) + tuple(c[k] for k in PLAN_COLUMNS)
