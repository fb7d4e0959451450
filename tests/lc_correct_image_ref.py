"""The loop-closure map correction on the map image (plslam_lc_correct_image) restated in numpy, and the replay of the reference's
map_points_kf_idx / map_lines_kf_idx from the event records of the image calls.

The image rule: landmark j is corrected when it is valid, [obs_ptr[j], obs_ptr[j + 1]) is a non-empty list inside obs_kf, its first
observer k = obs_kf[obs_ptr[j]] is a slot of the map and corrected[k]; X[j], med_dir[j] and the rows of its list in dir then take
T_corr[k] (pgo_ref._rt: ((r0 p0 + r1 p1) + r2 p2) + t).  No anchor lists."""
from __future__ import annotations

import numpy as np

from pgo_ref import _rt

KINDS = ("points", "lines")


def anchor_slots(K, n_map_kf, corrected):
    """per landmark the slot whose T_corr it takes, -1 where it is not corrected"""
    valid, ptr = np.asarray(K["valid"]).reshape(-1), np.asarray(K["obs_ptr"], np.int64).reshape(-1)
    obs_kf, corrected = np.asarray(K["obs_kf"], np.int64).reshape(-1), np.asarray(corrected).astype(bool)
    slot = np.full(valid.size, -1, np.int64)
    for j in range(valid.size):
        b, e = ptr[j], ptr[j + 1]
        if not valid[j] or not (b >= 0 and e > b and e <= obs_kf.size):
            continue
        k = obs_kf[b]
        if 0 <= k < n_map_kf and corrected[k]:
            slot[j] = k
    return slot


def correct_kind(K, n_map_kf, T_corr, corrected, dirs=None, med_dir=None):
    """-> dict(X, dirs, med_dir (None where not given), n, n_dirs): new arrays and the counts of one kind"""
    T_corr = np.asarray(T_corr, np.float64).reshape(-1, 4, 4)
    ptr = np.asarray(K["obs_ptr"], np.int64).reshape(-1)
    X = np.array(K["X"], np.float64)
    dirs = None if dirs is None else np.array(dirs, np.float64).reshape(-1, 3)
    med = None if med_dir is None else np.array(med_dir, np.float64).reshape(-1, 3)
    slot = anchor_slots(K, n_map_kf, corrected)
    n_dirs = 0
    for j in np.flatnonzero(slot >= 0):
        T = T_corr[slot[j]]
        for h in range(0, X.shape[1], 3):
            X[j, h:h + 3] = _rt(T, X[j, h:h + 3])
        if med is not None:
            med[j] = _rt(T, med[j])
        if dirs is not None:
            dirs[ptr[j]:ptr[j + 1]] = _rt(T, dirs[ptr[j]:ptr[j + 1]])
            n_dirs += int(ptr[j + 1] - ptr[j])
    return dict(X=X, dirs=dirs, med_dir=med, n=int((slot >= 0).sum()), n_dirs=n_dirs)


def correct_image(m, T_corr, corrected, x_kf_w_new=None, lists=None, med_dir=None, kind_fn=correct_kind):
    """the whole call on an image dict -> dict(points, lines: correct_kind's dict, x_kf_w, counts)"""
    nk = int(m["n_map_kf"])
    out = {}
    for kind in KINDS:
        d = None if lists is None else lists[kind]["dir"]
        out[kind] = kind_fn(m[kind], nk, T_corr, corrected, d, None if med_dir is None else med_dir.get(kind))
    x = np.array(m["x_kf_w"], np.float64).reshape(nk, 6)
    if x_kf_w_new is not None:
        co = np.asarray(corrected).astype(bool)
        x[co] = np.asarray(x_kf_w_new, np.float64).reshape(nk, 6)[co]
    out["x_kf_w"] = x
    out["counts"] = dict(n_pt=out["points"]["n"], n_ls=out["lines"]["n"], n_pt_dirs=out["points"]["n_dirs"], n_ls_dirs=out["lines"]["n_dirs"])
    return out


# ---- the same in array operations: trusted only because test_lc_correct_image_cpu.py finds it equal to the loop, bit for bit -----
def _rt_rows(T, p):
    """_rt with one transform per row: T (m, 4, 4), p (m, 3) -> ((r0 p0 + r1 p1) + r2 p2) + t"""
    R, t = T[:, :3, :3], T[:, :3, 3]
    return ((R[:, :, 0] * p[:, 0:1] + R[:, :, 1] * p[:, 1:2]) + R[:, :, 2] * p[:, 2:3]) + t


def correct_kind_fast(K, n_map_kf, T_corr, corrected, dirs=None, med_dir=None):
    """correct_kind without a Python loop, for an obs_ptr that starts at 0 and never descends (anything else is refused: lists
    that overlap are transformed twice by the loop, and a row then has no one landmark)"""
    T_corr = np.asarray(T_corr, np.float64).reshape(-1, 4, 4)
    valid, ptr = np.asarray(K["valid"]).reshape(-1), np.asarray(K["obs_ptr"], np.int64).reshape(-1)
    obs_kf, corrected = np.asarray(K["obs_kf"], np.int64).reshape(-1), np.asarray(corrected).astype(bool)
    n, lens = valid.size, np.diff(ptr)
    assert ptr.size == n + 1 and ptr[0] == 0 and (lens >= 0).all(), "correct_kind_fast: obs_ptr must start at 0 and never descend"
    X = np.array(K["X"], np.float64)
    dirs = None if dirs is None else np.array(dirs, np.float64).reshape(-1, 3)
    med = None if med_dir is None else np.array(med_dir, np.float64).reshape(-1, 3)
    b, e = ptr[:n], ptr[1:]
    ok = (valid != 0) & (e > b) & (e <= obs_kf.size)
    slot = np.full(n, -1, np.int64)
    first = obs_kf[b[ok]]
    slot[ok] = np.where((first >= 0) & (first < n_map_kf) & corrected[np.clip(first, 0, corrected.size - 1)], first, -1)
    j = np.flatnonzero(slot >= 0)
    for h in range(0, X.shape[1], 3):
        X[j, h:h + 3] = _rt_rows(T_corr[slot[j]], X[j, h:h + 3])
    if med is not None:
        med[j] = _rt_rows(T_corr[slot[j]], med[j])
    n_dirs = 0
    if dirs is not None:
        row_slot = slot[np.repeat(np.arange(n), lens)]            # per row of [0, obs_ptr[n]) the slot of its landmark
        o = np.flatnonzero(row_slot >= 0)
        dirs[o] = _rt_rows(T_corr[row_slot[o]], dirs[o])
        n_dirs = int(o.size)
    return dict(X=X, dirs=dirs, med_dir=med, n=int(j.size), n_dirs=n_dirs)


def correct_image_fast(m, T_corr, corrected, x_kf_w_new=None, lists=None, med_dir=None):
    """correct_image through correct_kind_fast: the same signature, the same dict"""
    return correct_image(m, T_corr, corrected, x_kf_w_new, lists, med_dir, kind_fn=correct_kind_fast)


# ---- the reference's containers, replayed from the records -----------------------------------------------------------------------
def lists_of(anchor_ptr, anchor_idx):
    """a CSR -> per-slot Python lists"""
    return [list(map(int, anchor_idx[anchor_ptr[k]:anchor_ptr[k + 1]])) for k in range(len(anchor_ptr) - 1)]


def csr_of(lists):
    ptr = np.zeros(len(lists) + 1, np.int32)
    ptr[1:] = np.cumsum([len(x) for x in lists])
    return ptr, np.array([j for x in lists for j in x], np.int32)


def _erase_first(lst, j):
    """the reference's erase loop: the FIRST entry that equals j goes (:2727-2737, :4521-4529)"""
    for i, v in enumerate(lst):
        if v == j:
            del lst[i]
            return
    raise AssertionError(f"landmark {j} is not in its first observer's list")


def replay_insert(lists, kf, out_kind):
    """kf2kf: a new landmark is pushed to kf1's list (:299-311 / :461); map2kf creates none"""
    for lm, _i1, _i2, is_new in np.asarray(out_kind["ev"]).reshape(-1, 4).tolist():
        if is_new:
            lists[int(kf["kf1"])].append(int(lm))


def replay_cull(lists, K_before, removed):
    """a culled landmark is erased from its first observer's list (:2717-2737 / :2756-2777)"""
    ptr, okf = np.asarray(K_before["obs_ptr"]), np.asarray(K_before["obs_kf"])
    for j in np.flatnonzero(removed).tolist():
        _erase_first(lists[int(okf[ptr[j]])], j)


def replay_fuse(lists, out_kind):
    """C: the new landmark is pushed to kf_prev's list (:4472-4477 / :4619); D: the dead landmark is erased from its first
    observer's (:4521-4529 / :4669-4676).  ev rows: code, kept, dead, anchor keyframe, position, count."""
    for code, keep, dead, anchor, _pos, _cnt in np.asarray(out_kind["ev"]).reshape(-1, 6).tolist():
        if code == 3:
            lists[anchor].append(int(keep))
        elif code == 4:
            _erase_first(lists[anchor], int(dead))
