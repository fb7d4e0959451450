"""A literal, sequential restatement of MapHandler::loopClosureFuseLandmarks (src/mapHandler.cpp:4412-4687) on Python lists of
lists: per landmark its kf_obs_list / obs_list as one list of (keyframe, observation, tag), per keyframe the list of its
features' idx, and a dense full_graph increment.  Nothing here works on CSR offsets: the image is unpacked first and packed again
at the end, so the checker shares no layout arithmetic with the device (plslam_amd/csrc/lc_fuse.hip).  The line numbers cited
are the reference's.  `hits` (a collections.Counter, optional) counts every branch taken.

An EVENT is a tuple (lm_idx0, lm_ldx0, lm_idx1, lm_ldx1) of an entry of lc_idx_list whose (2) == 1, in entry order then tuple
order; its number t is its position in the kind's concatenated array.  tag: a source observation's index, or -1 - (2 t + w) for
the observation tuple t made (w = 0 kf_prev's, 1 kf_curr's).

Where the reference has undefined behaviour the restatement does what include/plslam_hip.h documents: it SKIPS the event and
counts it (the order of the checks below is the header's).  The LEVEL of an event is 1 + the largest level among the latest
earlier events that name one of its landmarks (an index in [0, n); every event of a flagged entry names, acted or not); one above
max_level raises LevelExceeded, as the call refuses.  Arithmetic as tests/map_insert_ref.py: Python floats in the order stated."""
from __future__ import annotations

import numpy as np

from map_insert_ref import over_norm, xform

FEAT_NULL = -2
MAX_LEVEL = 64                                                    # include/plslam_hip.h: PLSLAM_LC_FUSE_MAX_LEVEL
BRANCHES = ("flag_zero", "skip.null_slot", "skip.lm_range", "skip.ldx_range", "skip.self_fuse", "skip.empty_b", "skip.graph_kf_range",
            "a.act", "a.feat_null", "a.lm_null", "a.lm_dead", "a.diagonal", "b.act", "b.feat_null", "b.lm_null", "b.lm_dead",
            "b.diagonal", "c.act", "c.feat_null0", "c.feat_null1", "d.act", "d.feat_null", "d.lm_null", "d.lm_dead", "d.on_grown_a",
            "d.copies_appended", "same_feature", "level.2", "level.max")


class LevelExceeded(Exception):
    pass


def _hit(hits, k):
    if hits is not None:
        hits[k] += 1


def _fuse_kind(m, kind, lc, G, hits, max_level):
    """the loop over one kind's entries -> (the kind's new image, dict(ev, dir, obs_src, counts))"""
    A, lines = m[kind], kind == "lines"
    n, nk, dl, dv = int(A["n"]), int(m["n_map_kf"]), A["X"].shape[1], A["obs_val"].shape[1]
    K = lc.get(kind)
    lc_idx = np.asarray(lc["lc_idx"]).reshape(-1, 3).tolist()
    T = np.asarray(lc["T_kf_w"], np.float64).reshape(nk, 4, 4).tolist()
    if K is None:
        tuples, eptr, P0, o0, P1, o1 = [], [0] * (len(lc_idx) + 1), [], [], [], []
    else:
        tuples, eptr = np.asarray(K["tuples"]).reshape(-1, 4).tolist(), np.asarray(K["entry_ptr"]).tolist()
        P0, o0, P1, o1 = (np.asarray(K[k], np.float64).tolist() for k in ("P0", "obs0", "P1", "obs1"))
    # ---- unpack the image into the reference's containers ----
    optr, okf, oval = A["obs_ptr"].tolist(), A["obs_kf"].tolist(), A["obs_val"].tolist()
    lists = [[(okf[j], oval[j], j) for j in range(optr[x], optr[x + 1])] for x in range(n)]
    valid, dead = A["valid"].tolist(), set()
    fp, fi = A["feat_ptr"].tolist(), A["feat_idx"].tolist()
    feat = [fi[fp[k]:fp[k + 1]] for k in range(nk)]
    kfv = m["kf_valid"].tolist()
    new, ev, dirs, first_tag, level, written = [], [], [], {}, {}, set()
    c = dict(n_a=0, n_b=0, n_c=0, n_d=0, n_new=0, n_dead=0, n_skipped=0)

    def skip(why):
        c["n_skipped"] += 1
        _hit(hits, why)

    def inc(i, j):
        if 0 <= i < nk and 0 <= j < nk:
            G[i][j] += 1
            G[j][i] += 1
        else:
            skip("skip.graph_kf_range")

    def write_feat(kf, ldx, lm):
        if (kf, ldx) in written:
            _hit(hits, "same_feature")
        written.add((kf, ldx))
        feat[kf][ldx] = lm

    def cam_dir(P):                                               # :4436 / :4560-4561: P / P.norm(), (sP + eP) / (sP + eP).norm()
        return over_norm([P[a] + P[3 + a] for a in range(3)] if lines else P)

    def world_dir(Tk, P):                                         # :4473-4474 / :4608-4611
        if lines:
            s, e = xform(Tk, P[:3]), xform(Tk, P[3:])
            return over_norm([0.5 * (s[a] + e[a]) for a in range(3)])
        return over_norm(xform(Tk, P))

    for ei, (kp, kc, flag) in enumerate(lc_idx):
        for t in range(eptr[ei], eptr[ei + 1]):
            a, l0, b, l1 = tuples[t]
            row, d = [0, -1, -1, -1, -1, 0], [0.0] * 6
            ev.append(row)
            dirs.append(d)
            if flag != 1:                                         # :4419 / :4543
                _hit(hits, "flag_zero")
                continue
            named = sorted({x for x in (a, b) if 0 <= x < n})
            lv = 1 + max([level.get(x, 0) for x in named], default=0)
            for x in named:
                level[x] = lv
            if lv > max_level:
                raise LevelExceeded(f"{kind}: event {t} has level {lv}")
            if lv == 2:
                _hit(hits, "level.2")
            if lv == max_level:
                _hit(hits, "level.max")
            if not kfv[kp] or not kfv[kc]:                        # (the reference dereferences map_keyframes[.])
                skip("skip.null_slot")
                continue
            if (a != -1 and not 0 <= a < n) or (b != -1 and not 0 <= b < n):
                skip("skip.lm_range")
                continue
            need0, need1 = a == -1, not (a == -1 and b != -1)     # which stereo_pt[.] / stereo_ls[.] the branch reads
            if (need0 and not 0 <= l0 < len(feat[kp])) or (need1 and not 0 <= l1 < len(feat[kc])):
                skip("skip.ldx_range")
                continue
            if a == -1 and b != -1:                               # :4431 / :4555
                if feat[kp][l0] == FEAT_NULL:
                    _hit(hits, "a.feat_null")
                    continue
                if not valid[b]:                                  # :4433 / :4557
                    _hit(hits, "a.lm_dead" if b in dead else "a.lm_null")
                    continue
                write_feat(kp, l0, b)                             # :4435
                d[0:3] = cam_dir(P0[t])                           # :4436
                tag = -1 - 2 * t
                lists[b].append((kp, o0[t], tag))                 # :4437
                for k, _, _ in lists[b]:                          # :4439-4443: against kf_curr, the new entry included
                    if k == kc:
                        _hit(hits, "a.diagonal")
                    inc(k, kc)
                row[:] = [1, b, -1, -1, -1, 1]
                first_tag[t] = tag
                c["n_a"] += 1
                _hit(hits, "a.act")
            elif a != -1 and b == -1:                             # :4446 / :4577
                if feat[kc][l1] == FEAT_NULL:
                    _hit(hits, "b.feat_null")
                    continue
                if not valid[a]:                                  # :4448 / :4579
                    _hit(hits, "b.lm_dead" if a in dead else "b.lm_null")
                    continue
                write_feat(kc, l1, a)                             # :4450
                d[3:6] = cam_dir(P1[t])                           # :4451
                tag = -1 - (2 * t + 1)
                lists[a].append((kc, o1[t], tag))                 # :4452
                for k, _, _ in lists[a]:                          # :4456-4460: against kf_prev
                    if k == kp:
                        _hit(hits, "b.diagonal")
                    inc(k, kp)
                row[:] = [2, a, -1, -1, -1, 1]
                first_tag[t] = tag
                c["n_b"] += 1
                _hit(hits, "b.act")
            elif a == -1 and b == -1:                             # :4464 / :4599
                if feat[kp][l0] == FEAT_NULL:
                    _hit(hits, "c.feat_null0")
                    continue
                if feat[kc][l1] == FEAT_NULL:
                    _hit(hits, "c.feat_null1")
                    continue
                lm = n + len(new)                                 # max_pt_idx / max_ls_idx
                write_feat(kp, l0, lm)                            # :4469-4470
                write_feat(kc, l1, lm)
                X = xform(T[kp], P0[t][:3]) + (xform(T[kp], P0[t][3:]) if lines else [])      # :4473 / :4608-4609
                d[0:3] = world_dir(T[kp], P0[t])
                d[3:6] = world_dir(T[kc], P1[t])                  # :4479-4480 / :4621-4624
                new.append((X, [(kp, o0[t], -1 - 2 * t), (kc, o1[t], -1 - (2 * t + 1))]))
                inc(kp, kc)                                       # :4486-4487
                row[:] = [3, lm, -1, kp, -1, 2]
                first_tag[t] = -1 - 2 * t
                c["n_c"] += 1
                c["n_new"] += 1
                _hit(hits, "c.act")
            else:                                                 # :4491 / :4638
                if feat[kc][l1] == FEAT_NULL:
                    _hit(hits, "d.feat_null")
                    continue
                if not valid[a] or not valid[b]:                  # :4493
                    _hit(hits, "d.lm_dead" if (a in dead or b in dead) else "d.lm_null")
                    continue
                if a == b:                                        # (the reference pushes onto the vector it iterates)
                    skip("skip.self_fuse")
                    continue
                if not lists[b]:                                  # (kf_obs_list[0] of an empty vector, :4521)
                    skip("skip.empty_b")
                    continue
                n_prev = len(lists[a])                            # :4496
                if n_prev > optr[a + 1] - optr[a]:
                    _hit(hits, "d.on_grown_a")
                if any(tg < 0 or not optr[b] <= tg < optr[b + 1] for _, _, tg in lists[b]):
                    _hit(hits, "d.copies_appended")
                row[:] = [4, a, b, lists[b][0][0], -1, len(lists[b])]              # the anchor: :4521
                first_tag[t] = lists[b][0][2]
                for ob in list(lists[b]):                         # :4499-4518
                    lists[a].append(ob)
                    for i in range(n_prev):
                        inc(lists[a][i][0], ob[0])
                write_feat(kc, l1, a)                             # :4517
                valid[b] = 0                                      # :4531-4532
                lists[b] = []
                dead.add(b)
                c["n_d"] += 1
                c["n_dead"] += 1
                _hit(hits, "d.act")
    # ---- pack the containers into the new image ----
    lists += [o for _, o in new]
    flat = [ob for lst in lists for ob in lst]
    ptr = np.zeros(len(lists) + 1, np.int64)
    ptr[1:] = np.cumsum([len(lst) for lst in lists])
    pos_of = {tg: j for j, (_, _, tg) in enumerate(flat)}
    for t, tg in first_tag.items():
        ev[t][4] = pos_of[tg]
    B = dict(n=len(lists), valid=np.array(valid + [1] * len(new), np.uint8),
             inlier=np.concatenate([A["inlier"], np.ones(len(new), np.uint8)]),
             X=np.concatenate([A["X"], np.array([x for x, _ in new], np.float64).reshape(-1, dl)]), obs_ptr=ptr.astype(np.int32),
             obs_kf=np.array([k for k, _, _ in flat], np.int32), obs_val=np.array([v for _, v, _ in flat], np.float64).reshape(-1, dv),
             feat_ptr=A["feat_ptr"].copy(), feat_idx=np.array([v for f in feat for v in f], np.int32))
    out = dict(ev=np.array(ev, np.int32).reshape(-1, 6), dir=np.array(dirs, np.float64).reshape(-1, 6),
               obs_src=np.array([tg for _, _, tg in flat], np.int32), counts=c)
    return B, out


def fuse(m, lc, hits=None, max_level=MAX_LEVEL):
    """loopClosureFuseLandmarks: the points' loop :4415-4537, then the lines' :4539-4685 -> (the map after, dict(points, lines:
    dict(ev (m, 6), dir (m, 6), obs_src, counts), graph_delta (n_map_kf, n_map_kf) int32)).  Raises LevelExceeded."""
    nk = int(m["n_map_kf"])
    G = [[0] * nk for _ in range(nk)]
    m2 = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in m.items() if k not in ("points", "lines")}
    out = {}
    for kind in ("points", "lines"):
        m2[kind], out[kind] = _fuse_kind(m, kind, lc, G, hits, max_level)
    out["graph_delta"] = np.array(G, np.int32).reshape(nk, nk)
    return m2, out
