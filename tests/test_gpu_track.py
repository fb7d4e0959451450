"""The tracker on the device (include/plslam_track.h; K108-K110 in front of K54): its rows bit for bit against tests/track_ref.py
on hand-made tables and across pair boundaries, its poses against the single call and against tests/lc_ref.py, the chain
from descriptors through a match plan with gates into the tracker on one stream, the one-frame back-projection, the refusals,
and the C++ client."""
import ctypes as C_
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

import plslam_amd
from plslam_amd import _lib, loop_closure as LC, track as TR
from plslam_amd.capi import EINVAL, ERANGE, PlslamError

import lc_batch_cases
import track_cases as TC
import track_ref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REL = 1e-9                                   # tests/test_gpu_loop_closure.py
ROW_KEYS = (("pt_rows", "pt_off"), ("P", "pt_off"), ("pl_obs", "pt_off"), ("pt_inlier", "pt_off"),
            ("ls_rows", "ls_off"), ("sPeP", "ls_off"), ("le_obs", "ls_off"), ("ls_inlier", "ls_off"))
FIELDS = (("m_pt", np.int32), ("st_pt_prev", np.int32), ("disp_pt_prev", np.float64), ("kp_prev", np.float32), ("st_pt_curr", np.int32),
          ("kp_curr", np.float32), ("m_ls", np.int32), ("st_ls_prev", np.int32), ("disp_ls_prev", np.float64), ("seg_prev", np.float32),
          ("st_ls_curr", np.int32), ("seg_curr", np.float32))


def _dev(ctx):
    import torch
    return torch.device("cuda", ctx.device)


def _counts(p):
    return dict(n_pt_prev=len(p["m_pt"]), n_pt_curr=np.asarray(p["kp_curr"]).reshape(-1, 2).shape[0],
                n_ls_prev=len(p["m_ls"]), n_ls_curr=np.asarray(p["seg_curr"]).reshape(-1, 4).shape[0])


class _Arena:
    """Every array of a list of host pairs in ONE device block (16-byte aligned slices): one upload.  records(): the
    plslam_track_pair of every pair, an empty array as NULL."""

    def __init__(self, ctx, pairs):
        import torch
        at, size = [], 0
        for p in pairs:
            o = {}
            for k, dt in FIELDS:
                a = np.ascontiguousarray(p[k], dt).reshape(-1)
                o[k] = (size, a) if a.size else None
                size += (a.nbytes + 15) // 16 * 16
            at.append(o)
        buf = np.zeros(size + 16, np.uint8)
        for o in at:
            for v in o.values():
                if v is not None:
                    buf[v[0]:v[0] + v[1].nbytes] = v[1].view(np.uint8)
        self.t = torch.from_numpy(buf).to(_dev(ctx))
        base = self.t.data_ptr()
        self.recs = [TR.track_pair(**{k: base + v[0] for k, v in o.items() if v is not None}, **_counts(p)) for o, p in zip(at, pairs)]


def _prefill(batch, value=0x5A):
    """every output array of the object, to its capacity, set to `value` bytes"""
    import torch
    b = batch.device_buffers()
    B, np_, nl = batch.B, int(b.pt_capacity), int(b.ls_capacity)
    sizes = dict(pt_off=4 * (B + 1), ls_off=4 * (B + 1), pt_rows=8 * np_, ls_rows=8 * nl, P=24 * np_, pl_obs=16 * np_, sPeP=48 * nl,
                 le_obs=24 * nl, pt_inlier=np_, ls_inlier=nl, results=C_.sizeof(LC.LcResult) * B)
    src = torch.full((max(sizes.values()) + 1,), value, dtype=torch.uint8, device=torch.device("cuda", batch._ctx.device))
    torch.cuda.synchronize()
    for k, n in sizes.items():
        if n:
            assert _lib._hip_memcpy_dtod(getattr(b, k), src.data_ptr(), n) == 0


def _bits(a):
    return np.ascontiguousarray(a, np.float64).reshape(-1).view(np.uint64)


def _same_rows(dl, ref, names=None):
    """offsets, row tables and row arrays equal the restatement bit for bit; rows past off[B] still hold the 0x5A prefill"""
    assert np.array_equal(dl["pt_off"], ref["pt_off"]), (dl["pt_off"][:8], ref["pt_off"][:8])
    assert np.array_equal(dl["ls_off"], ref["ls_off"]), (dl["ls_off"][:8], ref["ls_off"][:8])
    for k, off in ROW_KEYS:
        n = int(ref[off][-1])
        got = dl[k]
        assert (got[n:].view(np.uint8) == 0x5A).all(), f"{k}: rows past off[B] were written"
        if k.endswith("inlier"):
            continue
        want = ref[k]
        assert got[:n].shape == want.shape, k
        if want.dtype == np.int32:
            assert np.array_equal(got[:n], want), k
        elif not np.array_equal(_bits(got[:n]), _bits(want)):
            bad = np.flatnonzero((_bits(got[:n]) != _bits(want)).reshape(n, -1).any(axis=1))
            b = np.searchsorted(ref[off], bad[0], side="right") - 1
            raise AssertionError(f"{k}: {bad.size} rows differ, first row {bad[0]} of pair {b} ({names[b] if names else ''}): "
                                 f"{got[bad[0]]} != {want[bad[0]]}")


def _run(ctx, prm, pairs, stream=None):
    import torch
    arena = _Arena(ctx, pairs)
    batch = TR.TrackBatch(ctx, prm, arena.recs)
    _prefill(batch)
    batch.run(stream.cuda_stream if stream is not None else 0)
    if stream is not None:
        stream.synchronize()
    dl = batch.download()
    torch.cuda.synchronize()
    return batch, arena, dl


# ---- rows ---------------------------------------------------------------------------------------------------------------------
def test_rows_on_the_hand_made_tables(ctx):
    """n_prev in {0, 1, 63, 64, 65, 255, 256, 257, 513} x {all, none, every other, the edge entries} and points-only / lines-only
    pairs in one batch: NaN and inf rows among them, so only bit patterns are compared (K54 runs on them and must come back)"""
    names, pairs = TC.edge_pairs()
    prm = LC.params(cam=TC.CAM)
    batch, _, dl = _run(ctx, prm, pairs)
    ref = track_ref.batch(TC.CAM, pairs, rows=track_ref.rows_seq)
    _same_rows(dl, ref, names)
    assert np.isnan(ref["le_obs"]).any() and np.isinf(ref["P"]).any() and np.isinf(ref["sPeP"]).any()
    for b, r in enumerate(dl["results"]):                              # K54 saw exactly these rows
        assert (r["common_pt"], r["common_ls"]) == (ref["pt_off"][b + 1] - ref["pt_off"][b], ref["ls_off"][b + 1] - ref["ls_off"][b]), names[b]
    batch.close()


@pytest.mark.parametrize("kind", ["points", "lines"])
def test_rows_of_a_batch_with_one_kind_only(ctx, kind):
    """no pair of the batch has a row of the other kind: that kind's capacity is 0 and its arrays are never written"""
    pairs = [TC.pair(300 + k, n if kind == "points" else 0, 0 if kind == "points" else n, mode, n_pt_curr=None if kind == "points" else 0,
                     n_ls_curr=0 if kind == "points" else None)
             for k, (n, mode) in enumerate([(257, "edges"), (0, "all"), (64, "alt"), (513, "all"), (1, "all")])]
    batch, _, dl = _run(ctx, LC.params(cam=TC.CAM), pairs)
    b = batch.device_buffers()
    assert (int(b.pt_capacity) == 0) == (kind == "lines") and (int(b.ls_capacity) == 0) == (kind == "points")
    _same_rows(dl, track_ref.batch(TC.CAM, pairs))
    batch.close()


@pytest.mark.parametrize("B", [1, 2, 255, 256, 257, 600])
def test_offsets_across_pairs(ctx, B):
    """n_prev <= 8 per kind, empty pairs at the start, in the middle and at the end: the scan across the lanes of K109 and
    across its chunks (B = 257, 600: more than one pair per lane)"""
    pairs = TC.small_pairs(B)
    batch, _, dl = _run(ctx, LC.params(cam=TC.CAM), pairs)
    ref = track_ref.batch(TC.CAM, pairs)
    _same_rows(dl, ref)
    if B > 2:
        assert ref["pt_off"][-1] > B and ref["ls_off"][-1] > B // 2
    batch.close()


# ---- the pose -----------------------------------------------------------------------------------------------------------------
def _pair_rows(dl, b):
    p0, p1, l0, l1 = dl["pt_off"][b], dl["pt_off"][b + 1], dl["ls_off"][b], dl["ls_off"][b + 1]
    return dl["P"][p0:p1], dl["pl_obs"][p0:p1], dl["sPeP"][l0:l1], dl["le_obs"][l0:l1], dl["pt_inlier"][p0:p1].astype(bool), dl["ls_inlier"][l0:l1].astype(bool)


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.max(np.abs(a - b)) / max(1e-300, float(np.max(np.abs(b))))) if a.size else 0.0


def _check_gn(d, pi, li, ref):
    """the tolerances of tests/test_gpu_loop_closure.py::_check, for computeRelativePoseRobustGN alone"""
    assert d["gn_ran"] == 1 and d["is_lc"] == ref["is_lc"]
    assert np.array_equal(pi, ref["pt_inlier"]) and np.array_equal(li, ref["ls_inlier"])
    for k in ("ok_res", "ok_unc", "ok_inl", "ok_trs", "ok_rot", "n_pt_inliers", "n_ls_inliers"):
        assert d[k] == ref[k], (k, d[k], ref[k])
    if ref["stops"][0] != "err_change" and ref["stops"][1] != "err_change":
        assert (d["iters_1"], d["iters_2"]) == (ref["iters_1"], ref["iters_2"])
    for k in ("e", "t", "r", "cov_eig"):
        assert (math.isnan(d[k]) and math.isnan(ref[k])) or abs(d[k] - ref[k]) <= REL * abs(ref[k]) + 1e-300, (k, d[k], ref[k])
    assert _rel(d["T_inc"], ref["T_inc"]) <= REL
    assert _rel(d["pose_inc"], ref["pose_inc"]) <= REL or not ref["is_lc"]


def _check_poses(ctx, prm, dl, refs):
    for b, (rows, ref, _) in enumerate(refs):
        P, pl, S, le, pi, li = _pair_rows(dl, b)
        assert np.array_equal(_bits(P), _bits(rows["P"])) and np.array_equal(_bits(le), _bits(rows["le_obs"])), b
        single, spi, sli = ctx.relpose_robust_gn(prm, P, pl, S, le)
        assert lc_batch_cases.same_result(single, dl["results"][b]), b
        assert np.array_equal(pi, spi) and np.array_equal(li, sli), b
        _check_gn(dl["results"][b], pi, li, ref)


def test_the_pose_of_every_pair(ctx):
    """six scene pairs, one without lines and one without points: results[b] and the masks are the single call's on pair b's
    downloaded rows bit for bit, and the restatement's within the loop-closure check's tolerances"""
    prm = LC.params(cam=TC.scene_cam())
    pairs = TC.pose_pairs()
    batch, _, dl = _run(ctx, prm, pairs)
    _same_rows(dl, track_ref.batch(TC.scene_cam(), pairs))
    assert dl["ls_off"][3] == dl["ls_off"][2] and dl["pt_off"][5] == dl["pt_off"][4]           # the pairs without a kind
    _check_poses(ctx, prm, dl, TC.gn_references("pose"))
    batch.close()


def test_placement_independence(ctx):
    """the same pair first and last of two batches: identical rows, an identical result"""
    prm = LC.params(cam=TC.scene_cam())
    pose = TC.pose_pairs()
    me, others = pose[0], [TC.pair(40, 65, 9, "edges"), pose[2], TC.pair(41, 0, 0, "all"), pose[4]]
    out = []
    for pairs, b in (([me] + others, 0), (others + [me], len(others))):
        batch, _, dl = _run(ctx, prm, pairs)
        out.append((_pair_rows(dl, b), dl["pt_rows"][dl["pt_off"][b]:dl["pt_off"][b + 1]], dl["ls_rows"][dl["ls_off"][b]:dl["ls_off"][b + 1]],
                    dl["results"][b]))
        batch.close()
    (ra, pa, la, resa), (rb, pb, lb, resb) = out
    for x, y in zip(ra, rb):
        assert x.shape == y.shape and x.tobytes() == y.tobytes()
    assert np.array_equal(pa, pb) and np.array_equal(la, lb) and pa.shape[0] > 100
    assert lc_batch_cases.same_result(resa, resb)


# ---- the whole chain ----------------------------------------------------------------------------------------------------------
def test_descriptors_to_poses_on_one_stream(ctx):
    """MatchPlan (prev L<->R, curr L<->R, prev<->curr, both kinds) with the stereo gates, then TrackBatch.run, on one stream,
    one synchronisation at the end; against oracle tables -> oracle gates -> track_ref -> lc_ref.  Twice: identical outputs."""
    import torch
    dev = _dev(ctx)
    scene, (pairs, tables), g = TC.chain_scene(), TC.chain_pairs(), TC.gates()
    prm = LC.params(cam=TC.scene_cam())
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)                 # noqa: E731
    keep, probs, gate_list, recs, tabs = [], [], [], [], []
    for p in scene:
        n_pt, n_ls = p["kp_pl"].shape[0], p["seg_pl"].shape[0]
        d = {k: t(p[k]) for k in ("pdesc_pl", "pdesc_pr", "pdesc_cl", "pdesc_cr", "ldesc_pl", "ldesc_pr", "ldesc_cl", "ldesc_cr",
                                   "kp_pl", "kp_pr", "kp_cl", "kp_cr", "seg_pl", "seg_pr", "seg_cl", "seg_cr")}
        i32 = lambda n: torch.full((n,), -2, dtype=torch.int32, device=dev)           # noqa: E731
        f64 = lambda n: torch.full((n,), -7.0, dtype=torch.float64, device=dev)       # noqa: E731
        o = dict(m_pp=i32(n_pt), m_cc=i32(n_pt), m_pc=i32(n_pt), l_pp=i32(n_ls), l_cc=i32(n_ls), l_pc=i32(n_ls),
                 st_pp=i32(n_pt), st_cc=i32(n_pt), sl_pp=i32(n_ls), sl_cc=i32(n_ls),
                 dp_pp=f64(n_pt), dp_cc=f64(n_pt), dl_pp=f64(2 * n_ls), dl_cc=f64(2 * n_ls))
        keep += [d, o]
        tabs.append(o)
        for a, b, mp, ml in (("pl", "pr", "m_pp", "l_pp"), ("cl", "cr", "m_cc", "l_cc"), ("pl", "cl", "m_pc", "l_pc")):
            probs.append((d[f"pdesc_{a}"].data_ptr(), n_pt, d[f"pdesc_{b}"].data_ptr(), n_pt, TC.NNR, TC.MUTUAL, o[mp].data_ptr(), 0))
            probs.append((d[f"ldesc_{a}"].data_ptr(), n_ls, d[f"ldesc_{b}"].data_ptr(), n_ls, TC.NNR, TC.MUTUAL, o[ml].data_ptr(), 0))
        for f, m, st, dp in (("p", "m_pp", "st_pp", "dp_pp"), ("c", "m_cc", "st_cc", "dp_cc")):
            gate_list.append(dict(matches_12=o[m].data_ptr(), f_l=d[f"kp_{f}l"].data_ptr(), f_r=d[f"kp_{f}r"].data_ptr(), n_l=n_pt, n_r=n_pt,
                                  lines=0, stereo_12=o[st].data_ptr(), disp=o[dp].data_ptr(), n_stereo=0, **g))
        for f, m, st, dp in (("p", "l_pp", "sl_pp", "dl_pp"), ("c", "l_cc", "sl_cc", "dl_cc")):
            gate_list.append(dict(matches_12=o[m].data_ptr(), f_l=d[f"seg_{f}l"].data_ptr(), f_r=d[f"seg_{f}r"].data_ptr(), n_l=n_ls, n_r=n_ls,
                                  lines=1, stereo_12=o[st].data_ptr(), disp=o[dp].data_ptr(), n_stereo=0, **g))
        recs.append(TR.track_pair(m_pt=o["m_pc"].data_ptr(), st_pt_prev=o["st_pp"].data_ptr(), disp_pt_prev=o["dp_pp"].data_ptr(),
                                  kp_prev=d["kp_pl"].data_ptr(), st_pt_curr=o["st_cc"].data_ptr(), kp_curr=d["kp_cl"].data_ptr(),
                                  n_pt_prev=n_pt, n_pt_curr=n_pt, m_ls=o["l_pc"].data_ptr(), st_ls_prev=o["sl_pp"].data_ptr(),
                                  disp_ls_prev=o["dl_pp"].data_ptr(), seg_prev=d["seg_pl"].data_ptr(), st_ls_curr=o["sl_cc"].data_ptr(),
                                  seg_curr=d["seg_cl"].data_ptr(), n_ls_prev=n_ls, n_ls_curr=n_ls))
    plan = ctx.plan(probs)
    plan.add_stereo_gates(gate_list)
    batch = TR.TrackBatch(ctx, prm, recs)
    st = torch.cuda.Stream(device=dev)
    ref = track_ref.batch(TC.scene_cam(), pairs)
    runs = []
    for _ in range(2):
        _prefill(batch)
        plan.run(st.cuda_stream)
        batch.run(st.cuda_stream)
        st.synchronize()                                                            # the one synchronisation
        dl = batch.download()
        _same_rows(dl, ref)
        runs.append(dl)
    for b, (o, m, p) in enumerate(zip(tabs, tables, pairs)):                        # the plan's tables are the oracle's
        assert np.array_equal(o["m_pc"].cpu().numpy(), m["pc"][0]) and np.array_equal(o["l_pc"].cpu().numpy(), m["pc"][1]), b
        assert np.array_equal(o["st_pp"].cpu().numpy(), p["st_pt_prev"]) and np.array_equal(o["sl_cc"].cpu().numpy(), p["st_ls_curr"]), b
    _check_poses(ctx, prm, runs[0], TC.gn_references("chain"))
    for k, v in runs[0].items():
        if k == "results":
            assert all(lc_batch_cases.same_result(x, y) for x, y in zip(v, runs[1][k]))
        else:
            assert v.tobytes() == runs[1][k].tobytes(), k
    batch.close()
    plan.close()


# ---- the one-frame form -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lines", [False, True])
def test_backproject_dev_is_the_trackers_rows_and_zero_elsewhere(ctx, lines):
    """prev against itself (m = identity, both stereo tables prev's): the tracker's row for left row i is backproject_dev's
    row i; rows that are not stereo are zeros.  257 rows: two workgroups, the second ragged"""
    import torch
    dev = _dev(ctx)
    n = 257
    p = TC.pair(77, 0 if lines else n, n if lines else 0, "edges", n_pt_curr=n, n_ls_curr=n)
    st = np.asarray(p["st_ls_prev" if lines else "st_pt_prev"])
    disp, f = p["disp_ls_prev" if lines else "disp_pt_prev"], p["seg_prev" if lines else "kp_prev"]
    ident = np.arange(n, dtype=np.int32)
    z = dict(m_pt=np.zeros(0, np.int32), st_pt_prev=np.zeros(0, np.int32), disp_pt_prev=np.zeros(0), kp_prev=np.zeros((0, 2), np.float32),
             st_pt_curr=np.zeros(0, np.int32), kp_curr=np.zeros((0, 2), np.float32), m_ls=np.zeros(0, np.int32), st_ls_prev=np.zeros(0, np.int32),
             disp_ls_prev=np.zeros((0, 2)), seg_prev=np.zeros((0, 4), np.float32), st_ls_curr=np.zeros(0, np.int32), seg_curr=np.zeros((0, 4), np.float32))
    if lines:
        z.update(m_ls=ident, st_ls_prev=st, st_ls_curr=st, disp_ls_prev=disp, seg_prev=f, seg_curr=f)
    else:
        z.update(m_pt=ident, st_pt_prev=st, st_pt_curr=st, disp_pt_prev=disp, kp_prev=f, kp_curr=f)
    batch, arena, dl = _run(ctx, LC.params(cam=TC.CAM), [z])
    rec = arena.recs[0]
    wa, wo = (6, 3) if lines else (3, 2)
    a = torch.full((n, wa), 9.0, dtype=torch.float64, device=dev)
    o = torch.full((n, wo), 9.0, dtype=torch.float64, device=dev)
    s = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()
    TR.backproject_dev(ctx, LC.params(cam=TC.CAM).cam, rec.st_ls_prev if lines else rec.st_pt_prev, rec.disp_ls_prev if lines else rec.disp_pt_prev,
                       rec.seg_prev if lines else rec.kp_prev, n, lines, a.data_ptr(), o.data_ptr(), s.cuda_stream)
    s.synchronize()
    a, o = a.cpu().numpy(), o.cpu().numpy()
    ra, ro = track_ref.frame(TC.CAM, st, disp, f, lines)
    assert np.array_equal(_bits(a), _bits(ra)) and np.array_equal(_bits(o), _bits(ro))
    rows = dl["ls_rows" if lines else "pt_rows"][:dl["ls_off" if lines else "pt_off"][1]]
    k = rows.shape[0]
    assert 0 < k < n and np.array_equal(rows[:, 0], np.flatnonzero(st >= 0))
    assert np.array_equal(_bits(a[rows[:, 0]]), _bits(dl["sPeP" if lines else "P"][:k]))
    assert np.array_equal(_bits(o[rows[:, 0]]), _bits(dl["le_obs" if lines else "pl_obs"][:k]))
    assert not a[st < 0].any() and not o[st < 0].any()
    batch.close()


# ---- refusals -----------------------------------------------------------------------------------------------------------------
def test_validation_and_that_everything_still_works_afterwards(ctx):
    L = ctx._L
    prm = LC.params(cam=TC.CAM)
    pairs = [TC.pair(1, 65, 9, "alt")]
    arena = _Arena(ctx, pairs)
    good = arena.recs[0]
    h = C_.c_void_p(123)

    def create(p=prm, recs=(good,), B=None, ctxh=None, out=h):
        arr = (TR.TrackPair * max(len(recs), 1))(*recs)
        return L.plslam_track_batch_create(ctx.handle if ctxh is None else ctxh, C_.byref(p) if p is not None else None, arr if recs else None,
                                           len(recs) if B is None else B, C_.byref(out) if out is not None else None)

    def changed(**kw):
        q = TR.TrackPair.from_buffer_copy(good)
        for k, v in kw.items():
            setattr(q, k, v)
        return q

    assert create(p=None) == EINVAL and h.value is None                                    # (*out is NULL after a failed create)
    assert create(out=None) == EINVAL and create(B=-1) == EINVAL and create(recs=(), B=1) == EINVAL
    for k in ("m_pt", "st_pt_prev", "disp_pt_prev", "kp_prev", "st_pt_curr", "kp_curr", "m_ls", "st_ls_prev", "disp_ls_prev", "seg_prev",
              "st_ls_curr", "seg_curr"):
        assert create(recs=(changed(**{k: None}),)) == EINVAL, k
    for k in ("n_pt_prev", "n_pt_curr", "n_ls_prev", "n_ls_curr"):
        assert create(recs=(changed(**{k: -1}),)) == EINVAL, k
        assert create(recs=(changed(**{k: LC.LC_MAX_FEATURES + 1}),)) == ERANGE, k
    assert create(B=LC.LC_MAX_BATCH + 1) == ERANGE
    assert create(p=LC.params(cam=TC.CAM, max_iters=-1)) == EINVAL
    assert h.value is None
    assert L.plslam_track_batch_run(None, None) == EINVAL
    assert L.plslam_track_batch_device_buffers(None, None) == EINVAL
    cam = prm.cam
    assert L.plslam_stereo_backproject_dev(ctx.handle, C_.byref(cam), None, None, None, 5, 0, None, None, None) == EINVAL
    assert L.plslam_stereo_backproject_dev(ctx.handle, C_.byref(cam), None, None, None, -1, 0, None, None, None) == EINVAL
    assert L.plslam_stereo_backproject_dev(ctx.handle, C_.byref(cam), None, None, None, 0, 0, None, None, None) == 0
    with pytest.raises(PlslamError) as e:
        TR.TrackBatch(ctx, prm, [changed(kp_prev=None)])
    assert e.value.code == EINVAL
    # B = 0: an object that launches nothing
    empty = TR.TrackBatch(ctx, prm, [])
    empty.run()
    b = empty.device_buffers()
    assert b.B == 0 and not b.pt_off and not b.results and empty.download()["results"] == []
    empty.close()
    # the context and a new object work
    batch = TR.TrackBatch(ctx, prm, arena.recs)
    _prefill(batch)
    batch.run()
    _same_rows(batch.download(), track_ref.batch(TC.CAM, pairs))
    batch.run()                                                                            # and the object runs again
    _same_rows(batch.download(), track_ref.batch(TC.CAM, pairs))
    batch.close()


# ---- the C++ client -----------------------------------------------------------------------------------------------------------
def test_cpp_client_tracks_two_pairs(tmp_path):
    """tests/cpp/test_track_shim.cpp uploads two pairs' tables, runs PLSLAM::TrackBatch and prints offsets, rows and T_inc with
    %.17g: the rows are the restatement's bit for bit, the poses its solve's within REL"""
    lib = os.path.dirname(plslam_amd.LIB_PATH)
    exe = str(tmp_path / "test_track_shim")
    subprocess.run([shutil.which("g++") or "g++", "-O2", "-std=c++17", os.path.join(ROOT, "tests", "cpp", "test_track_shim.cpp"),
                    "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "plslam_amd", "host"), "-I/opt/rocm/include",
                    "-D__HIP_PLATFORM_AMD__", "-L" + lib, "-lplslam_hip", "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib",
                    "-lamdhip64", "-o", exe], check=True)
    pairs, refs = TC.pose_pairs()[:2], TC.gn_references("pose")[:2]
    cam = TC.scene_cam()
    for b, p in enumerate(pairs):
        for k, dt in FIELDS:
            np.ascontiguousarray(p[k], dt).tofile(str(tmp_path / f"p{b}_{k}.bin"))
    c = _counts(pairs[0]), _counts(pairs[1])
    (tmp_path / "meta.txt").write_text("2\n" + "".join(f"{x['n_pt_prev']} {x['n_pt_curr']} {x['n_ls_prev']} {x['n_ls_curr']}\n" for x in c))
    prm = dict(LC.DEFAULTS)
    vals = [cam["fx"], cam["fy"], cam["cx"], cam["cy"], cam["b"]] + [prm[k] for k in ("homog_th", "max_iters", "max_iters_ref", "lc_res", "lc_unc",
                                                                                       "lc_inl", "lc_trs", "lc_rot")]
    (tmp_path / "params.txt").write_text(" ".join(repr(v) for v in vals) + "\n")
    r = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.strip().split("\n")
    at = 0
    for b in range(2):
        tag, bb, npt, nls = lines[at].split()
        assert tag == "pair" and int(bb) == b
        npt, nls = int(npt), int(nls)
        rows = np.array([[int(v) for v in ln.split()] for ln in lines[at + 1:at + 1 + npt]], np.int32).reshape(-1, 2)
        P0 = np.array([float(v) for v in lines[at + 1 + npt].split()[1:]])
        lrows = np.array([[int(v) for v in ln.split()] for ln in lines[at + 2 + npt:at + 2 + npt + nls]], np.int32).reshape(-1, 2)
        T = np.array([float(v) for v in lines[at + 2 + npt + nls].split()[1:]]).reshape(4, 4)
        at += 3 + npt + nls
        ref_rows, ref, _ = refs[b]
        assert np.array_equal(rows, ref_rows["pt_rows"]) and np.array_equal(lrows, ref_rows["ls_rows"])
        assert np.array_equal(_bits(P0), _bits(ref_rows["P"][0]))                          # %.17g: every bit
        assert _rel(T, ref["T_inc"]) <= REL
