"""The inputs of tests/test_gpu_lba_plan_dev.py: observation columns for plslam_lba_plan_create / _create_dev.  A case is a dict of
the call's arguments (host arrays); T = the tile of the device-side list builder (distribute_dev.hpp: DIST_TILE), POSE_CHUNK and
SCH_CHUNK the chunk lengths of lba_lists.hpp."""
import numpy as np

from plslam_amd.capi import LbaPlan

T = LbaPlan.DIST_TILE
POSE_CHUNK = SCH_CHUNK = 64


def case(nkf, npt, nls, pt_lm, pt_kf, ls_lm, ls_kf, n_slots=None, seed=0):
    rng = np.random.Generator(np.random.PCG64(seed))
    n_slots = n_slots if n_slots is not None else nkf + 3
    i32 = lambda a: np.ascontiguousarray(a, np.int32).reshape(-1)                  # noqa: E731
    pt_lm, pt_kf, ls_lm, ls_kf = i32(pt_lm), i32(pt_kf), i32(ls_lm), i32(ls_kf)
    return dict(n_pose_slots=n_slots, nkf=nkf, npt=npt, nls=nls, pt_lm=pt_lm, pt_slot=rng.integers(0, n_slots, pt_lm.size).astype(np.int32),
                pt_kf_loc=pt_kf, pt_obs_uv=rng.uniform(0, 700, (pt_lm.size, 2)), ls_lm=ls_lm,
                ls_slot=rng.integers(0, n_slots, ls_lm.size).astype(np.int32), ls_kf_loc=ls_kf, ls_l_obs=rng.uniform(-1, 1, (ls_lm.size, 3)))


def random_case(n_pt_obs, n_ls_obs, nkf=5, npt=None, nls=None, seed=1, fixed_frac=0.25):
    """unsorted lm_loc, kf_loc in [-1, nkf): about fixed_frac of the observations by keyframes that are not optimised"""
    rng = np.random.Generator(np.random.PCG64(seed))
    npt = npt if npt is not None else max(1, n_pt_obs // 3)
    nls = nls if nls is not None else max(1, n_ls_obs // 3)

    def kf(n):
        k = rng.integers(0, max(nkf, 1), n)
        k[rng.random(n) < fixed_frac] = -1
        return k if nkf > 0 else np.full(n, -1)
    lm = lambda n_lm, n: rng.integers(0, n_lm, n) if n else np.zeros(0, np.int32)        # noqa: E731
    return case(nkf, npt, nls, lm(npt, n_pt_obs), kf(n_pt_obs), lm(nls, n_ls_obs), kf(n_ls_obs), seed=seed)


def pairs_in_block(n_point_lms, n_line_lms):
    """two keyframes; every landmark is seen once by each: block (0, 1) -- and (0, 0), (1, 1) -- holds n_point_lms point pairs and
    n_line_lms line pairs"""
    pl, ll = np.repeat(np.arange(n_point_lms), 2), np.repeat(np.arange(n_line_lms), 2)
    return case(2, n_point_lms, n_line_lms, pl, np.tile([0, 1], n_point_lms), ll, np.tile([0, 1], n_line_lms), seed=5)


def keyframe_lengths(lengths):
    """keyframe k is observed len[k] times (points, and a few lines among them), every landmark once"""
    kf = np.concatenate([np.full(n, k) for k, n in enumerate(lengths)])
    n_ls = 7
    return case(len(lengths), kf.size - n_ls, n_ls, np.arange(kf.size - n_ls), kf[:-n_ls], np.arange(n_ls), kf[-n_ls:], seed=6)


CASES = {
    **{f"both_{n}": (lambda n=n: random_case(n, n, seed=10 + n % 97)) for n in (0, 1, T - 1, T, T + 1, 3 * T + 37)},
    "points_only": lambda: random_case(300, 0, nls=0, seed=2),
    "lines_only": lambda: random_case(0, 300, npt=0, seed=3),
    "one_keyframe": lambda: random_case(400, 150, nkf=1, seed=4),
    "no_optimised_keyframe": lambda: random_case(400, 150, fixed_frac=1.1, seed=5),
    "all_on_one_keyframe": lambda: case(4, 60, 20, np.arange(300) % 60, np.full(300, 2), np.arange(90) % 20, np.full(90, 2), seed=6),
    # a landmark seen twice by the same keyframe: the pairs (a, b) and (b, a) both belong to block (k, k)
    "twice_by_one_keyframe": lambda: case(3, 2, 1, [1, 0, 1, 1, 0], [2, 0, 2, 1, -1], [0, 0, 0], [1, 1, 0], seed=7),
    "nkf_23": lambda: random_case(2500, 800, nkf=23, seed=8),
    # a third digit for lm_loc, one observation per landmark (shuffled)
    "npt_over_65536": lambda: (lambda r: case(6, 70001, 40, r.permutation(70001), r.integers(-1, 6, 70001), r.integers(0, 40, 120),
                                              r.integers(-1, 6, 120), seed=9))(np.random.Generator(np.random.PCG64(9))),
    "block_64_point_pairs": lambda: pairs_in_block(SCH_CHUNK, 5),
    "block_65_point_pairs": lambda: pairs_in_block(SCH_CHUNK + 1, 5),
    "keyframe_63_64_65": lambda: keyframe_lengths((POSE_CHUNK - 1, POSE_CHUNK, POSE_CHUNK + 1)),
}
