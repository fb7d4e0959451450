"""The tracker's rows restated (include/plslam_track.h): rows_seq is the literal sequential text -- a loop per pair, per i1,
every operation on fp64 scalars in the order the header writes it -- and rows_vec the same arithmetic on whole arrays, which
tests/test_track_cpu.py pins to it bit for bit.  numpy evaluates one operation per call and rounds each to fp64: no contraction.

A pair is a dict of host arrays named as plslam_track_pair's fields: m_pt, st_pt_prev, disp_pt_prev (n), kp_prev (n x 2 f32),
st_pt_curr, kp_curr; m_ls, st_ls_prev, disp_ls_prev (n x 2), seg_prev (n x 4 f32), st_ls_curr, seg_curr.  The counts are the
arrays' lengths (prev: of the match table; curr: of the key points / segments).  cam: a dict with fx, cx, cy, b."""
import numpy as np

F = np.float64


def back_projection(cam, u, v, d):
    """PinholeStereoCamera::backProjection as the header states it"""
    bd = F(cam["b"]) / d
    return bd * (u - F(cam["cx"])), bd * (v - F(cam["cy"])), bd * F(cam["fx"])


def line_through(sx, sy, ex, ey):
    le0, le1, le2 = sy - ey, ex - sx, sx * ey - sy * ex
    n = np.sqrt(le0 * le0 + le1 * le1)
    return le0 / n, le1 / n, le2 / n


def _correspondence(m, st_prev, st_curr, n_curr, i1):
    i2 = int(m[i1])
    if not 0 <= i2 < n_curr:
        return -1
    if st_prev[i1] < 0 or st_curr[i2] < 0:
        return -1
    return i2


def rows_seq(cam, pair):
    out = {k: [] for k in ("pt_rows", "P", "pl_obs", "ls_rows", "sPeP", "le_obs")}
    with np.errstate(all="ignore"):
        kp0, kp1 = np.asarray(pair["kp_prev"], np.float32).reshape(-1, 2), np.asarray(pair["kp_curr"], np.float32).reshape(-1, 2)
        for i1 in range(len(pair["m_pt"])):
            i2 = _correspondence(pair["m_pt"], pair["st_pt_prev"], pair["st_pt_curr"], kp1.shape[0], i1)
            if i2 < 0:
                continue
            u, v, d = F(kp0[i1, 0]), F(kp0[i1, 1]), F(pair["disp_pt_prev"][i1])
            out["pt_rows"].append((i1, i2))
            out["P"].append(back_projection(cam, u, v, d))
            out["pl_obs"].append((F(kp1[i2, 0]), F(kp1[i2, 1])))
        sg0, sg1 = np.asarray(pair["seg_prev"], np.float32).reshape(-1, 4), np.asarray(pair["seg_curr"], np.float32).reshape(-1, 4)
        disp = np.asarray(pair["disp_ls_prev"], F).reshape(-1, 2)
        for i1 in range(len(pair["m_ls"])):
            i2 = _correspondence(pair["m_ls"], pair["st_ls_prev"], pair["st_ls_curr"], sg1.shape[0], i1)
            if i2 < 0:
                continue
            sP = back_projection(cam, F(sg0[i1, 0]), F(sg0[i1, 1]), disp[i1, 0])
            eP = back_projection(cam, F(sg0[i1, 2]), F(sg0[i1, 3]), disp[i1, 1])
            out["ls_rows"].append((i1, i2))
            out["sPeP"].append(sP + eP)
            out["le_obs"].append(line_through(F(sg1[i2, 0]), F(sg1[i2, 1]), F(sg1[i2, 2]), F(sg1[i2, 3])))
    return _typed(out)


def _typed(out):
    w = dict(pt_rows=2, P=3, pl_obs=2, ls_rows=2, sPeP=6, le_obs=3)
    return {k: np.asarray(v, np.int32 if k.endswith("rows") else F).reshape(-1, w[k]) for k, v in out.items()}


def _kept(m, st_prev, st_curr, n_curr):
    m = np.asarray(m, np.int64)
    ok = (m >= 0) & (m < n_curr)
    i1 = np.flatnonzero(ok)
    i2 = m[i1]
    keep = (np.asarray(st_prev)[i1] >= 0) & (np.asarray(st_curr)[i2] >= 0) if i1.size else np.zeros(0, bool)
    return i1[keep], i2[keep]


def rows_vec(cam, pair):
    with np.errstate(all="ignore"):
        kp0, kp1 = np.asarray(pair["kp_prev"], np.float32).reshape(-1, 2).astype(F), np.asarray(pair["kp_curr"], np.float32).reshape(-1, 2).astype(F)
        i1, i2 = _kept(pair["m_pt"], pair["st_pt_prev"], pair["st_pt_curr"], kp1.shape[0])
        d = np.asarray(pair["disp_pt_prev"], F).reshape(-1)[i1]
        P = np.stack(back_projection(cam, kp0[i1, 0], kp0[i1, 1], d), axis=1) if i1.size else np.zeros((0, 3))
        out = dict(pt_rows=np.stack([i1, i2], axis=1), P=P, pl_obs=kp1[i2])
        sg0, sg1 = np.asarray(pair["seg_prev"], np.float32).reshape(-1, 4).astype(F), np.asarray(pair["seg_curr"], np.float32).reshape(-1, 4).astype(F)
        j1, j2 = _kept(pair["m_ls"], pair["st_ls_prev"], pair["st_ls_curr"], sg1.shape[0])
        disp = np.asarray(pair["disp_ls_prev"], F).reshape(-1, 2)[j1]
        if j1.size:
            a, b = sg0[j1], sg1[j2]
            sPeP = np.stack(back_projection(cam, a[:, 0], a[:, 1], disp[:, 0]) + back_projection(cam, a[:, 2], a[:, 3], disp[:, 1]), axis=1)
            le = np.stack(line_through(b[:, 0], b[:, 1], b[:, 2], b[:, 3]), axis=1)
        else:
            sPeP, le = np.zeros((0, 6)), np.zeros((0, 3))
        out.update(ls_rows=np.stack([j1, j2], axis=1), sPeP=sPeP, le_obs=le)
    return _typed(out)


def batch(cam, pairs, rows=rows_vec):
    """The packed form of B pairs: pt_off, ls_off (B + 1) and the six row arrays concatenated"""
    per = [rows(cam, p) for p in pairs]
    out = {k: np.concatenate([r[k] for r in per]) if per else _typed({k: []})[k] for k in ("pt_rows", "P", "pl_obs", "ls_rows", "sPeP", "le_obs")}
    out["pt_off"] = np.concatenate([[0], np.cumsum([r["pt_rows"].shape[0] for r in per])]).astype(np.int32)
    out["ls_off"] = np.concatenate([[0], np.cumsum([r["ls_rows"].shape[0] for r in per])]).astype(np.int32)
    out["per_pair"] = per
    return out


def frame(cam, st, disp, f, lines):
    """plslam_stereo_backproject_dev: one frame by left row, zeros where st < 0"""
    n = len(st)
    pair = dict(m_pt=np.zeros(0, np.int32), st_pt_prev=np.zeros(0, np.int32), disp_pt_prev=np.zeros(0), kp_prev=np.zeros((0, 2), np.float32),
                st_pt_curr=np.zeros(0, np.int32), kp_curr=np.zeros((0, 2), np.float32), m_ls=np.zeros(0, np.int32),
                st_ls_prev=np.zeros(0, np.int32), disp_ls_prev=np.zeros((0, 2)), seg_prev=np.zeros((0, 4), np.float32),
                st_ls_curr=np.zeros(0, np.int32), seg_curr=np.zeros((0, 4), np.float32))
    ident = np.arange(n, dtype=np.int32)
    if lines:
        pair.update(m_ls=ident, st_ls_prev=st, st_ls_curr=st, disp_ls_prev=disp, seg_prev=f, seg_curr=f)
        r = rows_vec(cam, pair)
        a, o = np.zeros((n, 6)), np.zeros((n, 3))
        a[r["ls_rows"][:, 0]], o[r["ls_rows"][:, 0]] = r["sPeP"], r["le_obs"]
    else:
        pair.update(m_pt=ident, st_pt_prev=st, st_pt_curr=st, disp_pt_prev=disp, kp_prev=f, kp_curr=f)
        r = rows_vec(cam, pair)
        a, o = np.zeros((n, 3)), np.zeros((n, 2))
        a[r["pt_rows"][:, 0]], o[r["pt_rows"][:, 0]] = r["P"], r["pl_obs"]
    return a, o
