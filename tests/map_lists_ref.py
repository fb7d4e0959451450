"""A sequential restatement of what the map's side lists (desc_list / dir_list / pts_list of MapPoint / MapLine) and the
representative descriptor do across an insert (MapHandler::addKeyFrame) and a loop-closure fusion
(MapHandler::loopClosureFuseLandmarks): the EVENT RECORDS of the existing restatements (tests/map_insert_ref.py,
tests/lc_fuse_ref.py, imported unchanged) are replayed, in event order, into per-landmark Python lists of tags:
  insert   a new landmark: [kf1 row, kf2 row]; an existing one: append the kf2 row
  fusion   A / B: append; C: a new pair; D: extend a by b's list, then clear b
A tag is a source observation's index, or -1 - (2 e + w) for the observation event / tuple e made (w = 0 the first keyframe's
row, 1 the second's): the obs_src encoding of include/plslam_hip.h.  The lists are flattened by landmark; rows are gathered by
tag; the representative of every landmark an event touched comes from oracle.median_desc_batched (pinned to the reference's
updateAverageDescDir), every other landmark keeps what the source lists store.  Nothing here uses CSR arithmetic of the device.

The replay proves its own ordering: obs_kf replayed the same way must equal the restatement's image (and, for the fusion, the
tags the restatement's own obs_src)."""
from __future__ import annotations

import functools

import numpy as np

from oracle import oracle as O
from plslam_amd import map_lists as ML

KINDS = ("points", "lines")


def _unpack(A):
    ptr = np.asarray(A["obs_ptr"]).tolist()
    return [list(range(ptr[x], ptr[x + 1])) for x in range(len(ptr) - 1)]


def replay_insert_kind(A, ev):
    """-> (lists of tags per landmark after the events, the landmarks an event touched)"""
    lists, touched = _unpack(A), set()
    for e, (lm, _, _, is_new) in enumerate(np.asarray(ev).reshape(-1, 4).tolist()):
        if is_new:
            assert lm == len(lists)
            lists.append([-1 - 2 * e, -1 - (2 * e + 1)])
        else:
            lists[lm].append(-1 - (2 * e + 1))
        touched.add(lm)
    return lists, touched


def replay_fuse_kind(A, ev):
    lists, touched = _unpack(A), set()
    for t, (code, keep, dead, _, _, _) in enumerate(np.asarray(ev).reshape(-1, 6).tolist()):
        if code == 1:
            lists[keep].append(-1 - 2 * t)
        elif code == 2:
            lists[keep].append(-1 - (2 * t + 1))
        elif code == 3:
            assert keep == len(lists)
            lists.append([-1 - 2 * t, -1 - (2 * t + 1)])
        elif code == 4:
            lists[keep].extend(lists[dead])
            lists[dead] = []
            touched.add(dead)
        if code:
            touched.add(keep)
    return lists, touched


def _gather_kind(kind, src, lists, touched, row_of, rows, names, dirs, kf_of, A_src, B_dst):
    """src: the kind's source lists; row_of(e, w) -> the row of rows[names[w]] event e's side w names; dirs: (n_ev, 6); kf_of(e,
    w): the keyframe of that observation -> the kind's destination lists with obs_src and refreshed"""
    tags = [tg for lst in lists for tg in lst]
    ptr = np.zeros(len(lists) + 1, np.int64)
    ptr[1:] = np.cumsum([len(lst) for lst in lists])
    n_obs = len(tags)
    assert np.array_equal(ptr, B_dst["obs_ptr"]), "the replay's list lengths are not the restatement's"
    desc, dir_ = np.zeros((n_obs, 32), np.uint8), np.zeros((n_obs, 3), np.float64)
    pts = np.zeros((n_obs, 4), np.float64) if kind == "lines" else None
    kf = np.zeros(n_obs, np.int32)
    tg_all = np.array(tags, np.int64).reshape(-1)
    old = tg_all >= 0                                             # (the copied rows at once; the events' rows one by one)
    desc[old], dir_[old], kf[old] = np.asarray(src["desc"])[tg_all[old]], np.asarray(src["dir"])[tg_all[old]], np.asarray(A_src["obs_kf"])[tg_all[old]]
    if pts is not None:
        pts[old] = np.asarray(src["pts"])[tg_all[old]]
    for j in np.flatnonzero(~old).tolist():
        e, w = (-1 - tags[j]) >> 1, (-1 - tags[j]) & 1
        r = row_of(e, w)
        desc[j], dir_[j], kf[j] = rows[names[w]][r], dirs[e, 3 * w:3 * w + 3], kf_of(e, w)
        if pts is not None:
            pts[j] = rows[names[2 + w]][r]
    assert np.array_equal(kf, B_dst["obs_kf"]), "the replayed obs_kf is not the restatement's: the replay's order is wrong"
    n, n_src = len(lists), int(np.asarray(src["med_idx"]).size)
    idx, med = O.median_desc_batched(desc, ptr.astype(np.int32)) if n else (np.zeros(0, np.int32), np.zeros((0, 32), np.uint8))
    refreshed = np.zeros(n, np.uint8)
    refreshed[sorted(touched)] = 1
    keep = np.flatnonzero(refreshed[:n_src] == 0)
    idx[keep], med[keep] = np.asarray(src["med_idx"])[keep], np.asarray(src["med_desc"]).reshape(-1, 32)[keep]
    empty = (np.diff(ptr) == 0) & (refreshed == 1)
    idx[empty], med[empty] = -1, 0                                # (an empty list: -1 and zero bytes, whatever the checker returns)
    out = dict(desc=desc, dir=dir_, med_idx=idx.astype(np.int32), med_desc=med, refreshed=refreshed, obs_src=np.array(tags, np.int32).reshape(-1))
    if pts is not None:
        out["pts"] = pts
    return out


def carry_insert(m_src, m_dst, kf, out, lists_src, rows):
    """the lists after the insert `out` = map_insert_ref.insert_*(m_src, kf)[1] took m_src to m_dst; rows: keyframe_rows"""
    res = {}
    for kind in KINDS:
        ev, dirs = out[kind]["ev"], out[kind]["dir"]
        lists, touched = replay_insert_kind(m_src[kind], ev)
        res[kind] = _gather_kind(kind, lists_src[kind], lists, touched, lambda e, w: int(ev[e, 1 + w]), rows.get(kind) or {},
                                 ("desc1", "desc2", "pts1", "pts2"), dirs, lambda e, w: kf["kf2"] if w else kf["kf1"], m_src[kind], m_dst[kind])
    return res


def carry_fuse(m_src, m_dst, lc, out, lists_src, rows):
    """the lists after the fusion `out` = lc_fuse_ref.fuse(m_src, lc)[1]; rows: tuple_rows"""
    res = {}
    lc_idx = np.asarray(lc["lc_idx"]).reshape(-1, 3)
    for kind in KINDS:
        ev, dirs = out[kind]["ev"], out[kind]["dir"]
        lists, touched = replay_fuse_kind(m_src[kind], ev)
        ent = np.repeat(np.arange(lc_idx.shape[0]), np.diff(lc[kind]["entry_ptr"])) if lc.get(kind) is not None else np.zeros(0, np.int64)
        res[kind] = _gather_kind(kind, lists_src[kind], lists, touched, lambda e, w: e, rows.get(kind) or {},
                                 ("desc0", "desc1", "pts0", "pts1"), dirs, lambda e, w: int(lc_idx[ent[e], w]), m_src[kind], m_dst[kind])
        assert np.array_equal(res[kind]["obs_src"], out[kind]["obs_src"]), "the replayed tags are not the restatement's obs_src"
    return res


def with_last_row_as_representative(lists, m):
    """the lists with med_idx / med_desc deliberately set to each list's LAST row: what an untouched landmark must keep"""
    out = {}
    for kind in KINDS:
        L, ptr = dict(lists[kind]), np.asarray(m[kind]["obs_ptr"], np.int64)
        lens = np.diff(ptr)
        idx = (lens - 1).astype(np.int32)
        med = np.zeros((lens.size, 32), np.uint8)
        med[lens > 0] = L["desc"][ptr[1:][lens > 0] - 1]
        L["med_idx"], L["med_desc"] = idx, med
        out[kind] = L
    return out


def tied_landmarks(desc, ptr, which):
    """how many of the landmarks `which` have a winning value that two rows share (the 'first row wins' rule decides them)"""
    n = 0
    for lm in which:
        d = desc[ptr[lm]:ptr[lm + 1]]
        if d.shape[0] < 2:
            continue
        D = np.sort(O.np_dist_matrix(d, d), axis=1)[:, int(1 + 0.5 * (d.shape[0] - 1))]
        n += int((D == D.min()).sum() >= 2)
    return n


@functools.lru_cache(maxsize=None)
def run_insert(name, clustered=True, last_row=False):
    """a case of map_insert_cases with lists -> dict(m, kf, kf_b, m_a, m_b, lists0, rows_a, rows_b, want_a, want_b); computed once
    and shared: nobody writes to it"""
    import map_insert_cases as CS
    m, kf, (m_a, out_a), kf_b, (m_b, out_b), _ = CS.run_ref(name)
    lists0 = ML.synthetic_lists(m, seed=5, clustered=clustered)
    if last_row:
        lists0 = with_last_row_as_representative(lists0, m)
    rows_a = ML.keyframe_rows(kf, seed=6, clustered=clustered)
    rows_b = {k: (None if kf_b.get(k) is None or rows_a.get(k) is None else {f: v for f, v in rows_a[k].items() if f.endswith("2")}) for k in KINDS}
    want_a = carry_insert(m, m_a, kf, out_a, lists0, rows_a)
    want_b = carry_insert(m_a, m_b, dict(kf_b, kf1=-1), out_b, want_a, rows_b)
    return dict(m=m, kf=kf, kf_b=kf_b, m_a=m_a, m_b=m_b, lists0=lists0, rows_a=rows_a, rows_b=rows_b, want_a=want_a, want_b=want_b,
                out_a=out_a, out_b=out_b)


@functools.lru_cache(maxsize=None)
def run_fuse(name, clustered=True, last_row=False):
    """a case of lc_fuse_cases with lists -> dict(m, lc, m_a, lists0, rows, want, out), or None where the restatement refuses"""
    import lc_fuse_cases as CS
    m, lc, after, _ = CS.run_ref(name)
    if after is None:
        return None
    lists0 = ML.synthetic_lists(m, seed=7, clustered=clustered)
    if last_row:
        lists0 = with_last_row_as_representative(lists0, m)
    rows = ML.tuple_rows(lc, seed=8, clustered=clustered)
    return dict(m=m, lc=lc, m_a=after[0], lists0=lists0, rows=rows, want=carry_fuse(m, after[0], lc, after[1], lists0, rows), out=after[1])
