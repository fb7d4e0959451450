"""Seeded loop-closure inputs that leave the one forward-facing scene of plslam_amd.loop_closure.keyframe_pair (a EuRoC camera,
depths of 2-20 m, one small pose, equal feature counts), for tests/test_lc_cpu.py (which checks from the input and the
restatement alone that each one reaches what it exists for) and the device tests (tests/test_gpu_loop_closure.py,
tests/test_gpu_lc_batch.py).  numpy and the oracle only.  A case is (parameter overrides, camera dict, kf0, kf1): keyframe_pair's
output with post-edits -- kf0's P and sPeP scaled, a keyframe cut, an entry overwritten.  keyframe_pair itself is untouched.

Scaling works because P and sPeP times s with the same observations is the same problem with its translation times s: the
translation columns of H shrink by s against the rotation columns, which moves the QR's pivots and the LU's row swaps.

  near / far50 / far1000   the scene x 0.02 (translation columns pivot first, no LU swap), x 50, x 1000 (the norm downdate's
                           recompute branch)
  tele / tele_near         fx = fy = 20000 (other pivot lists), and that scene x 0.01
  lines_near / points_far  has_points = 0 at x 0.02; has_lines = 0 at x 1000
  th1                      homog_th = 1 at x 0.2: z^2 and ||err|| on both sides of std::max(homog_th, .)
  n255 ... n513            keep_frac = 1, flip_p = 0: every row matches, common == n at the gather's chunk of 256 and twice it
  cut_kf1 / cut_kf0        the 513 / 129 pair with one keyframe cut to its first 255 / 63 rows: the two ratios under std::max differ
  no_idx0 / no_idx         pt_idx / ls_idx = None in kf0, in both: the -1 rows of the gather
  still_p / still_pl       pose 0 without noise: e == 0 exactly (points), rounding noise (with lines); the err_small stop
  nan_landmark             one NaN coordinate in a matched P row of kf0
"""
from __future__ import annotations

import numpy as np

from plslam_amd import loop_closure as LC, synth
from oracle import oracle as O

import lc_ref

SEED, N_PT, N_LS = 11, 300, 60
TH1_SEED = 19          # of seeds 11-39 the one whose nearest residual lies farthest (0.84 px) from the outlier threshold
TELE = dict(synth.EUROC, fx=20000.0, fy=20000.0)
COUNTS = ((255, 63), (256, 64), (257, 65), (511, 127), (512, 128), (513, 129))
ALL_MATCH = dict(keep_frac=1.0, flip_p=0.0)
STILL = dict(pose=(0.0,) * 6, noise_px=0.0, outlier_frac=0.0, keep_frac=1.0, flip_p=0.0)
# points_far at seed 11 moves by 1.1e-10 (e, cov_eig) under a reordering of its rows, over a tenth of the suite's 1e-9: re-seeded
POINTS_FAR_SEED = 12
NAN_ROW = 3            # the NaN goes into the NAN_ROW-th matched point row of kf0, coordinate 1
KF1_POINT, KF1_LINE = ("pdesc", "P", "pl", "pt_idx"), ("ldesc", "sPeP", "le", "ls_idx")


def scaled(kf0, s):
    o = dict(kf0)
    o["P"], o["sPeP"] = kf0["P"] * s, kf0["sPeP"] * s
    return o


def cut(kf, n_pt, n_ls):
    o = dict(kf)
    for k in KF1_POINT:
        o[k] = np.ascontiguousarray(kf[k][:n_pt])
    for k in KF1_LINE:
        o[k] = np.ascontiguousarray(kf[k][:n_ls])
    return o


def _pair(seed=SEED, n_pt=N_PT, n_ls=N_LS, scale=1.0, cam=None, **kw):
    kf0, kf1, _ = LC.keyframe_pair(seed, n_pt, n_ls, cam=cam, **kw)
    return (scaled(kf0, scale) if scale != 1.0 else kf0), kf1


def _nan_landmark():
    kf0, kf1 = _pair()
    m12, _ = O.match(kf0["pdesc"], kf1["pdesc"], LC.DEFAULTS["min_ratio_12_p"], True)
    kf0 = dict(kf0, P=kf0["P"].copy())
    kf0["P"][np.flatnonzero(m12 >= 0)[NAN_ROW], 1] = np.nan
    return kf0, kf1


def _without_idx(kf):
    return dict(kf, pt_idx=None, ls_idx=None)


def _build(name):
    E = synth.EUROC
    if name == "near":
        return {}, E, *_pair(scale=0.02)
    if name == "far50":
        return {}, E, *_pair(scale=50.0)
    if name == "far1000":
        return {}, E, *_pair(scale=1000.0)
    if name == "tele":
        return {}, TELE, *_pair(cam=TELE)
    if name == "tele_near":
        return {}, TELE, *_pair(cam=TELE, scale=0.01)
    if name == "lines_near":
        return dict(has_points=0), E, *_pair(scale=0.02)
    if name == "points_far":
        return dict(has_lines=0), E, *_pair(seed=POINTS_FAR_SEED, scale=1000.0)
    if name == "th1":
        return dict(homog_th=1.0), E, *_pair(seed=TH1_SEED, scale=0.2)
    if name in COUNT_NAMES:
        return {}, E, *_pair(*((SEED,) + COUNT_NAMES[name]), **ALL_MATCH)
    if name in ("cut_kf1", "cut_kf0"):
        kf0, kf1 = _pair(SEED, 513, 129, **ALL_MATCH)
        return ({}, E, kf0, cut(kf1, 255, 63)) if name == "cut_kf1" else ({}, E, cut(kf0, 255, 63), kf1)
    if name in ("no_idx0", "no_idx"):
        kf0, kf1 = _pair()
        return {}, E, _without_idx(kf0), (kf1 if name == "no_idx0" else _without_idx(kf1))
    if name == "still_p":
        return dict(has_lines=0), E, *_pair(SEED, 257, 65, **STILL)
    if name == "still_pl":
        return {}, E, *_pair(SEED, 257, 65, **STILL)
    if name == "nan_landmark":
        return {}, E, *_nan_landmark()
    raise KeyError(name)


COUNT_NAMES = {f"n{n_pt}": (n_pt, n_ls) for n_pt, n_ls in COUNTS}
SCENES = ("near", "far50", "far1000", "tele", "tele_near", "lines_near", "points_far", "th1")
NAMES = SCENES + tuple(COUNT_NAMES) + ("cut_kf1", "cut_kf0", "no_idx0", "no_idx", "still_p", "still_pl", "nan_landmark")
# compared field by field at the suite's tolerance; still_pl and nan_landmark are compared as their tests state
VALUE_COMPARED = tuple(n for n in NAMES if n not in ("still_pl", "nan_landmark"))
_cases, _refs, _lds = {}, {}, {}


def case(name):
    """-> (parameter overrides, camera dict, kf0, kf1); built once"""
    if name not in _cases:
        _cases[name] = _build(name)
    return _cases[name]


def ocam(cam):
    return O.make_cam(**cam)


def reference(name):
    """lc_ref.is_loop_closure of the case -> (ref, params dict, log of the QR solves and the LU inverse); computed once"""
    if name not in _refs:
        over, cam, kf0, kf1 = case(name)
        prm = LC.params_dict(LC.params(cam, **over))
        log = {"qr": [], "lu": []}
        _refs[name] = (lc_ref.is_loop_closure(prm, ocam(cam), kf0, kf1, log=log), prm, log)
    return _refs[name]


def first_system(name):
    """-> (lc_ref.first_system_ld(..., with_scale=True) over the case's correspondences, the oracle's distance from it:
    lc_ref.system_distance of O.pose_gn_accumulate at T = I).  The distance is the size of fp64 rounding on this input."""
    if name not in _lds:
        over, cam, _, _ = case(name)
        ref, prm, _ = reference(name)
        P, pl, S, le = ref["corr_inputs"]
        ld = lc_ref.first_system_ld(ocam(cam), prm["homog_th"], P, pl, S, le, with_scale=True)
        H, g, e, (n_p, n_l) = O.pose_gn_accumulate(ocam(cam), prm["homog_th"], np.eye(4), P, pl, np.ones(len(P), np.uint8), S, le,
                                                   np.ones(len(S), np.uint8))
        _lds[name] = (ld, lc_ref.system_distance(H, g, e / (n_p + n_l), ld))
    return _lds[name]


# computeRelativePoseRobustGN on given correspondences (the device's identity path, which keeps no rows): the points of
# n255 / n256 / n257 without lines, and their lines without points
IDENTITY = {f"id_p{n_pt}": (f"n{n_pt}", "p") for n_pt, _ in COUNTS[:3]}
IDENTITY.update({f"id_l{n_ls}": (f"n{n_pt}", "l") for n_pt, n_ls in COUNTS[:3]})


def identity_problem(name):
    """-> (P, pl_obs, sPeP, le_obs) of IDENTITY[name]; its restatement is reference(name)"""
    src, kind = IDENTITY[name]
    P, pl, S, le = reference(src)[0]["corr_inputs"]
    assert len(P) == COUNT_NAMES[src][0] and len(S) == COUNT_NAMES[src][1]
    q = (P, pl, S[:0], le[:0]) if kind == "p" else (P[:0], pl[:0], S, le)
    if name not in _refs:
        prm = LC.params_dict(LC.params())
        log = {"qr": [], "lu": []}
        ref = lc_ref.relpose_robust_gn(prm, ocam(synth.EUROC), *q, log=log)
        ref.update(corr_inputs=q, common_pt=len(q[0]), common_ls=len(q[2]))
        _cases[name] = ({}, synth.EUROC, None, None)
        _refs[name] = (ref, prm, log)
    return q


# the parameter sets the cases run under: a batched call has one set for all its records
PARAM_SETS = {"default": ({}, synth.EUROC), "tele": ({}, TELE), "lines": (dict(has_points=0), synth.EUROC),
              "points": (dict(has_lines=0), synth.EUROC), "th1": (dict(homog_th=1.0), synth.EUROC)}


def param_set_of(name):
    over, cam, _, _ = case(name)
    return next(k for k, (o, c) in PARAM_SETS.items() if o == over and c == cam)
