"""The inputs the local-map tests share: test_local_map_cpu.py shows they reach the branches they are named for,
test_gpu_local_map.py runs the device entry points on them.  A case is (map, dict(anchor, min_cov, window, kf2, max_kf_idx,
min_lm_obs)).  T = the look-back tile's item count."""
import numpy as np

from plslam_amd import local_map as LM

T = LM.LOOKBACK_TILE
SIZES = (0, 1, T - 1, T, T + 1, 3 * T + 37)


def hand_map(kf_valid, row, points=(), lines=(), pt_feats=None, ls_feats=None):
    """A map written out by hand.  points / lines: a (valid, inlier, [observing keyframes]) per landmark; *_feats: {keyframe:
    [feature idx, ...]} in feature order."""
    n_kf = len(kf_valid)
    rng = np.random.Generator(np.random.PCG64(77))

    def kind(lms, feats, dl, dv):
        feats = feats or {}
        n = len(lms)
        obs_ptr = np.zeros(n + 1, np.int32)
        obs_ptr[1:] = np.cumsum([len(o) for _, _, o in lms]) if n else 0
        obs_kf = np.array([k for _, _, o in lms for k in o], np.int32)
        feat_ptr = np.zeros(n_kf + 1, np.int32)
        feat_ptr[1:] = np.cumsum([len(feats.get(k, ())) for k in range(n_kf)])
        feat_idx = np.array([i for k in range(n_kf) for i in feats.get(k, ())], np.int32)
        return dict(n=n, valid=np.array([v for v, _, _ in lms], np.uint8), inlier=np.array([i for _, i, _ in lms], np.uint8),
                    X=rng.uniform(-5, 5, (n, dl)), obs_ptr=obs_ptr, obs_kf=obs_kf, obs_val=rng.uniform(0, 500, (obs_kf.size, dv)),
                    feat_ptr=feat_ptr, feat_idx=feat_idx)

    return dict(n_map_kf=n_kf, kf_valid=np.array(kf_valid, np.uint8), x_kf_w=rng.standard_normal((n_kf, 6)),
                row=np.array(row, np.int32), points=kind(points, pt_feats, 3, 2), lines=kind(lines, ls_feats, 6, 3))


def exact(n):
    """n valid landmarks of each kind with exactly one observation each and everything local: n list entries, n observations"""
    m = LM.synthetic_map(n_kf=12, n_pt=n, n_ls=n, seed=100 + n, max_obs=1, null_lm_frac=0.0, no_obs_frac=0.0)
    return m, dict(anchor=11, min_cov=0, window=0, kf2=11, max_kf_idx=30, min_lm_obs=2)


def mixed(n, **kw):
    m = LM.synthetic_map(n_kf=kw.pop("n_kf", 30), n_pt=n, n_ls=max(n // 3, min(n, 1)), seed=200 + n, **kw)
    return m, dict(anchor=m["n_map_kf"] - 1, min_cov=75, window=3, kf2=m["n_map_kf"] - 1, max_kf_idx=m["n_map_kf"] + 4, min_lm_obs=3)


def cull_edges():
    """14 keyframes, slot 1 NULL.  Points: 0 an outlier first seen in keyframe 2, named TWICE there (the first goes, the duplicate
    stays); 1 an outlier whose first observer is the NULL slot 1; 2 first seen in keyframe 3 with max_kf_idx = 13: 13 - 3 == 10,
    kept; 3 first seen in keyframe 2: 11, removed for its single observation; 4 an outlier without observations: kept; 5 an
    outlier that no feature names: removed, nothing cleared; 6 an inlier with enough observations: kept.  One line like point 0."""
    kf_valid = [1, 0] + [1] * 12
    pts = [(1, 0, [2, 4]), (1, 0, [1, 5]), (1, 0, [3]), (1, 1, [2]), (1, 0, []), (1, 0, [2, 3]), (1, 1, [2, 3, 4])]
    m = hand_map(kf_valid, [0] * 14, points=pts, lines=[(1, 0, [2, 3])],
                 pt_feats={2: [3, LM.FEAT_NULL, 0, -1, 0, 6], 3: [2, 6], 4: [0, 6], 5: [1]}, ls_feats={2: [-1, 0, 0], 3: [0]})
    return m, dict(anchor=13, min_cov=1, window=0, kf2=13, max_kf_idx=13, min_lm_obs=2)


CASES = {
    **{f"exact_{n}": (lambda n=n: exact(n)) for n in SIZES},
    **{f"mixed_{n}": (lambda n=n: mixed(n)) for n in SIZES},
    "one_keyframe": lambda: (LM.synthetic_map(n_kf=1, n_pt=40, n_ls=10, seed=7),
                             dict(anchor=0, min_cov=75, window=3, kf2=0, max_kf_idx=20, min_lm_obs=3)),
    "all_local": lambda: (mixed(300)[0], dict(anchor=29, min_cov=10 ** 6, window=10 ** 6, kf2=5, max_kf_idx=40, min_lm_obs=3)),
    "anchor_only": lambda: (mixed(300)[0], dict(anchor=29, min_cov=10 ** 6, window=-1, kf2=29, max_kf_idx=40, min_lm_obs=3)),
    "null_slot_in_window": lambda: (mixed(300, null_kf=(27, 4))[0],
                                    dict(anchor=29, min_cov=10 ** 6, window=5, kf2=29, max_kf_idx=40, min_lm_obs=3)),
    "anchor_null_features": lambda: (mixed(300, null_feat_frac=0.5)[0],
                                     dict(anchor=29, min_cov=75, window=2, kf2=29, max_kf_idx=40, min_lm_obs=3)),
    "overload_kf": lambda: (mixed(300)[0], dict(anchor=12, min_cov=100, window=1, kf2=12, max_kf_idx=40, min_lm_obs=3)),
    "anchor_null": lambda: (mixed(300, null_kf=(12,))[0], dict(anchor=12, min_cov=100, window=1, kf2=12, max_kf_idx=40, min_lm_obs=3)),
    "points_only": lambda: (LM.synthetic_map(n_kf=20, n_pt=400, n_ls=0, seed=8),
                            dict(anchor=19, min_cov=75, window=3, kf2=19, max_kf_idx=25, min_lm_obs=3)),
    "lines_only": lambda: (LM.synthetic_map(n_kf=20, n_pt=0, n_ls=400, seed=9),
                           dict(anchor=19, min_cov=75, window=3, kf2=19, max_kf_idx=25, min_lm_obs=3)),
    "no_observations": lambda: (LM.synthetic_map(n_kf=20, n_pt=300, n_ls=80, seed=10, no_obs_frac=1.0),
                                dict(anchor=19, min_cov=75, window=3, kf2=19, max_kf_idx=25, min_lm_obs=3)),
    "cull_edges": cull_edges,
    # a local landmark whose observation list is empty (named by a feature all the same): no candidate, no observation rows
    "local_without_observations": lambda: (hand_map([1, 1, 1], [0, 0, 0], points=[(1, 1, []), (1, 1, [1, 2])], lines=[(1, 1, [])],
                                                    pt_feats={2: [0, 1]}, ls_feats={2: [0]}),
                                           dict(anchor=2, min_cov=1, window=0, kf2=1, max_kf_idx=20, min_lm_obs=1)),
}

# what each named case is there for (tests/local_map_ref.py: BRANCHES); every case must reach its own
REACHES = {
    "one_keyframe": ("form.feat_set",),
    "all_local": ("form.graph_window", "gather.obs_kf_local", "gather.kf_zero"),
    "anchor_only": ("form.graph_neither", "gather.obs_kf_not_local", "cull.removed_outlier"),
    "null_slot_in_window": ("form.graph_null_slot", "gather.kf_null"),
    "anchor_null_features": ("form.anchor_feat_null", "form.graph_feat_null"),
    "overload_kf": ("form.graph_cov", "form.graph_window", "form.graph_neither"),
    "anchor_null": ("form.anchor_null",),
    "no_observations": ("cull.empty", "cand.null"),
    "cull_edges": ("cull.feat_first", "cull.feat_duplicate_left", "cull.observer_null", "cull.recent", "cull.removed_few_obs",
                   "cull.removed_outlier", "cull.empty", "cull.kept"),
    "local_without_observations": ("cand.empty", "gather.lm_no_obs"),
    "mixed_805": ("form.feat_unmatched", "form.feat_lm_null", "cand.not_local", "cand.same_kf", "cand.yes",
                  "gather.lm_null", "gather.lm_not_local", "gather.lm_listed", "gather.obs_kf_local", "gather.obs_kf_not_local",
                  "cull.null", "cull.local", "cull.kept", "cull.removed_few_obs"),
}


def run_ref(m, p, hits=None):
    """The restatement's four loops on a COPY of the map -> dict of every output, and the map after the cull"""
    import copy

    import local_map_ref as R
    m = copy.deepcopy(m)
    kf_l, pt_l, ls_l = R.form(m, p["anchor"], p["min_cov"], p["window"], hits)
    out = dict(kf_local=kf_l, pt_local=pt_l, ls_local=ls_l, pt_candidate=R.candidates(m, "points", pt_l, p["kf2"], hits),
               ls_candidate=R.candidates(m, "lines", ls_l, p["kf2"], hits))
    g = R.gather(m, kf_l, pt_l, ls_l, hits)
    out.update(g)
    for t in ("pt", "ls"):
        o = g[t + "_obs"]
        out[t + "_lm_loc"], out[t + "_pose_slot"], out[t + "_kf_loc"] = o[:, 1].copy(), o[:, 3].copy(), o[:, 4].copy()
    out["pt_removed"], out["ls_removed"] = R.cull(m, pt_l, ls_l, p["max_kf_idx"], p["min_lm_obs"], hits)
    return out, m
