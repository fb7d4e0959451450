"""plslam_lc_correct_image (K105-K107) on the device: the loop-closure map correction on the map image, without anchor lists,
against the numpy restatement (tests/lc_correct_image_ref.py), against plslam_lc_correct_map_dev given the lists derived from the
image, and inside the whole resident loop-closure chain.  Every comparison is bitwise."""
import ctypes as C

import numpy as np
import pytest

import lc_correct_image_ref as R
import lc_fuse_ref as FR
import map_lists_ref as LR
from lc_correct_image_cases import decision_map as _decision_map
from lc_correct_image_cases import length_map as _length_map
from plslam_amd import capi
from plslam_amd import lc_fuse as LF
from plslam_amd import local_map as LM
from plslam_amd import map_insert as MI
from plslam_amd import map_lists as ML
from plslam_amd import pgo as PG

pytestmark = pytest.mark.gpu
T = LM.LOOKBACK_TILE
BLANK = 90


def _bits(a):
    return np.ascontiguousarray(a, np.float64).reshape(-1).view(np.uint64)


def _inputs(m, seed, corrected=None):
    rng = np.random.Generator(np.random.PCG64(seed))
    nk = m["n_map_kf"]
    T_corr = np.stack([MI._pose(rng) for _ in range(nk)])
    co = (rng.random(nk) < 0.6) if corrected is None else np.asarray(corrected, bool)
    lists = {kind: dict(dir=rng.standard_normal((m[kind]["obs_kf"].size, 3)), desc=np.zeros((m[kind]["obs_kf"].size, 32), np.uint8),
                        med_idx=np.zeros(m[kind]["n"], np.int32)) for kind in R.KINDS}
    med = {kind: rng.standard_normal((m[kind]["n"], 3)) for kind in R.KINDS}
    return T_corr, co, lists, med, rng.standard_normal((nk, 6))


class _Device:
    """the image, its dir lists and two med_dir arrays on the device"""

    def __init__(self, ctx, m, lists=None, med=None):
        import torch
        self.ctx, self.m = ctx, m
        self.index = LM.DeviceMapIndex(m, ctx.device)
        self.lists = None if lists is None else ML.DeviceMapLists(lists, device=ctx.device)
        dev = torch.device("cuda", ctx.device)
        self.med = None if med is None else {k: torch.from_numpy(np.ascontiguousarray(med[k]) if med[k].size else np.zeros((1, 3))).to(dev)
                                             for k in R.KINDS}

    def correct(self, T_corr, co, x_new=None):
        med = None if self.med is None else {k: t.data_ptr() for k, t in self.med.items()}
        return PG.correct_image(self.ctx, self.index, T_corr, co, x_new, self.lists, med)

    def state(self):
        out = dict(x_kf_w=self.index.host("x_kf_w"))
        for kind in R.KINDS:
            n = self.m[kind]["n"]
            out[kind] = dict(X=self.index.host(f"{kind}.X"), dirs=None if self.lists is None else self.lists.host(f"{kind}.dir"),
                             med_dir=None if self.med is None else self.med[kind].cpu().numpy()[:n])
        return out


def _same(got, want, what=""):
    assert np.array_equal(_bits(got["x_kf_w"]), _bits(want["x_kf_w"])), (what, "x_kf_w")
    for kind in R.KINDS:
        for f in ("X", "dirs", "med_dir"):
            g, w = got[kind][f], want[kind][f]
            assert (g is None) == (w is None), (what, kind, f)
            if g is not None:
                assert np.array_equal(_bits(g), _bits(w)), (what, kind, f, np.flatnonzero(_bits(g) != _bits(w))[:8])


def _against_the_restatement(ctx, m, seed, corrected=None, with_dir=True, with_med=True, with_x=True):
    T_corr, co, lists, med, x_new = _inputs(m, seed, corrected)
    d = _Device(ctx, m, lists if with_dir else None, med if with_med else None)
    counts = d.correct(T_corr, co, x_new if with_x else None)
    want = R.correct_image(m, T_corr, co, x_new if with_x else None, lists if with_dir else None, med if with_med else None)
    _same(d.state(), want, seed)
    assert counts == want["counts"], (counts, want["counts"])
    return counts, want, co


# ---- the shapes at the kernels' edges -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, T - 1, T, T + 1])
def test_landmark_counts_at_the_tile_edges(ctx, n):
    m = LM.synthetic_map(n_kf=6, n_pt=n, n_ls=n, seed=300 + n, no_obs_frac=0.1)
    counts, _, _ = _against_the_restatement(ctx, m, 10 + n, corrected=[1, 0, 1, 1, 0, 1])
    if n >= T - 1:
        assert counts["n_pt"] > T // 4 and counts["n_ls"] > T // 4 and counts["n_pt_dirs"] > counts["n_pt"]


@pytest.mark.parametrize("nk", [1, 2])
@pytest.mark.parametrize("lines_too", [True, False])
def test_list_lengths_and_a_list_across_a_workgroup_boundary(ctx, nk, lines_too):
    m = _length_map(nk, lines_too)
    assert m["points"]["obs_ptr"][5] < T < m["points"]["obs_ptr"][6] and m["lines"]["n"] == (13 if lines_too else 0)
    for corrected in ([1] * nk, [1] + [0] * (nk - 1), [0] * (nk - 1) + [1]):
        counts, _, _ = _against_the_restatement(ctx, m, 7, corrected)
        assert counts["n_pt"] > 0 and (counts["n_ls"] > 0) == lines_too


@pytest.mark.parametrize("with_dir", [True, False])
@pytest.mark.parametrize("with_med", [True, False])
def test_arrays_that_are_not_carried(ctx, with_dir, with_med):
    m = LM.synthetic_map(n_kf=9, n_pt=T + 40, n_ls=70, seed=12)
    counts, want, _ = _against_the_restatement(ctx, m, 13, corrected=[1, 0, 1, 1, 0, 1, 1, 0, 1], with_dir=with_dir, with_med=with_med,
                                               with_x=with_med)
    assert (counts["n_pt_dirs"] > 0) == with_dir and (counts["n_ls_dirs"] > 0) == with_dir and counts["n_pt"] > 0


# ---- the decisions ----------------------------------------------------------------------------------------------------------------------
def test_nothing_corrected_changes_nothing(ctx):
    m = _decision_map()
    T_corr, _, lists, med, x_new = _inputs(m, 3)
    d = _Device(ctx, m, lists, med)
    before = d.state()
    assert d.correct(T_corr, np.zeros(4, bool), x_new) == dict(n_pt=0, n_ls=0, n_pt_dirs=0, n_ls_dirs=0)
    _same(d.state(), before, "no slot corrected")
    # only the slot that anchors nothing: its x_kf_w row is written, no landmark moves
    assert d.correct(T_corr, np.array([0, 0, 0, 1], bool), x_new) == dict(n_pt=0, n_ls=0, n_pt_dirs=0, n_ls_dirs=0)
    after = d.state()
    assert np.array_equal(_bits(after["x_kf_w"][:18]), _bits(before["x_kf_w"][:18])) and np.array_equal(_bits(after["x_kf_w"][18:]), _bits(x_new[3]))
    after["x_kf_w"] = before["x_kf_w"]
    _same(after, before, "the slot that anchors nothing")


def test_every_slot_corrected_and_who_is_left_alone(ctx):
    m = _decision_map()
    counts, want, _ = _against_the_restatement(ctx, m, 5, corrected=[1, 1, 1, 1])
    assert counts == dict(n_pt=3, n_ls=3, n_pt_dirs=6, n_ls_dirs=6)
    for kind in R.KINDS:                                          # (the restatement itself: who moved)
        moved = (want[kind]["X"] != m[kind]["X"]).any(axis=1)
        assert moved.tolist() == [True, False, True, False, False, False, True], kind
    assert np.array_equal(_bits(want["x_kf_w"]), _bits(_inputs(m, 5, [1, 1, 1, 1])[4]))
    # slot 0 alone: the invalid landmark it first observed stays, so does the valid landmark of slot 1; x_kf_w row 0 only
    counts, want, _ = _against_the_restatement(ctx, m, 6, corrected=[1, 0, 0, 0])
    assert counts == dict(n_pt=1, n_ls=1, n_pt_dirs=2, n_ls_dirs=2)
    assert np.array_equal(_bits(want["x_kf_w"][1:]), _bits(m["x_kf_w"][1:])) and not np.array_equal(want["x_kf_w"][0], m["x_kf_w"][0])


# ---- against the parent's route -----------------------------------------------------------------------------------------------------
def test_equals_correct_map_dev_given_the_lists_of_the_image(ctx):
    import torch
    m = LM.synthetic_map()
    lists = ML.synthetic_lists(m)
    T_corr, co, _, med, x_new = _inputs(m, 21)
    nk = m["n_map_kf"]
    new = _Device(ctx, m, lists, med)
    counts = new.correct(T_corr, co, x_new)
    old = _Device(ctx, m, lists, med)
    dev = torch.device("cuda", ctx.device)
    keep = [torch.from_numpy(np.ascontiguousarray(T_corr.reshape(-1, 16))).to(dev), torch.from_numpy(co.astype(np.uint8)).to(dev)]
    args = []
    for kind in R.KINDS:
        ptr, idx = LM.anchor_lists(m, kind)
        keep += [torch.from_numpy(ptr).to(dev), torch.from_numpy(idx if idx.size else np.zeros(1, np.int32)).to(dev)]
        args.append(dict(n=m[kind]["n"], n_anchor=int(idx.size), n_dir=int(m[kind]["obs_kf"].size), anchor_ptr=keep[-2].data_ptr(),
                         anchor_idx=keep[-1].data_ptr(), valid=old.index.ptr(f"{kind}.valid"), X=old.index.ptr(f"{kind}.X"),
                         med_dir=old.med[kind].data_ptr(), dir_ptr=old.index.ptr(f"{kind}.obs_ptr"), dirs=old.lists.ptr(f"{kind}.dir")))
    capi.correct_map_dev(ctx, nk, keep[0].data_ptr(), keep[1].data_ptr(), args[0], args[1])
    got, par = new.state(), old.state()
    par["x_kf_w"] = got["x_kf_w"]                                 # (the parent's route does not write x_kf_w)
    _same(got, par, "plslam_lc_correct_map_dev")
    want = R.correct_image(m, T_corr, co, x_new, lists, med)
    _same(got, want, "the restatement")
    assert counts == want["counts"] and counts["n_pt"] > 150 and counts["n_ls"] > 30


# ---- the chain ------------------------------------------------------------------------------------------------------------------------
def _same_image(img, want, what):
    for kind in R.KINDS:
        for f in ("valid", "inlier", "X", "obs_ptr", "obs_kf", "obs_val", "feat_idx"):
            g, w = img.host(f"{kind}.{f}"), np.asarray(want[kind][f])
            assert g.shape == w.shape, (what, kind, f, g.shape, w.shape)
            same = np.array_equal(_bits(g), _bits(w)) if w.dtype == np.float64 else np.array_equal(g, w)
            assert same, (what, kind, f)


def test_the_resident_loop_closure_chain_equals_the_host_route(ctx):
    """insert -> carry -> cull -> pose graph -> correct_image -> fusion -> carry on the resident image, against: the download, the
    containers replayed from the records, plslam_lc_correct_map, the fusion's restatement"""
    with_obs = lambda m: {k: ((m[k]["valid"] == 1) & (np.diff(m[k]["obs_ptr"]) > 0)).astype(np.uint8) for k in R.KINDS}  # noqa: E731
    m0, kf = MI.synthetic_keyframe(LM.synthetic_map(), 96, 32, seed=3, points=dict(n_new=18, n_exist=18, n_invalid=4, n_same_lm=2),
                                   lines=dict(n_new=6, n_exist=6, n_invalid=2))
    nk = m0["n_map_kf"]
    lists0 = ML.synthetic_lists(m0)
    mi, ml, lm, lf = MI.MapInsert(ctx), ML.MapLists(ctx), LM.LocalMap(ctx), LF.LcFuse(ctx)
    src, sl = LM.DeviceMapIndex(m0, ctx.device), ML.DeviceMapLists(lists0, device=ctx.device)
    cap = MI.insert_bounds(m0, kf, "kf2kf")
    img, dl = MI.DeviceMapImage(m0, **cap, device=ctx.device, blank=BLANK), ML.DeviceMapLists(None, **cap, device=ctx.device, blank=BLANK)
    mi.kf2kf(src, img, kf)
    ml.insert_carry(mi, src, sl, img, dl, ML.keyframe_rows(kf, seed=4))
    lm.form(img, nk - 1, m0["row"], 75, 3)
    culled = lm.cull(img, nk + 4, 3)
    removed = lm.download("pt_removed", "ls_removed")
    assert culled["n_pt_removed"] >= 5 and culled["n_ls_removed"] >= 1
    # the host route's containers: the lists of the first image, the insert's records, the cull's masks
    mA, listsA = img.host_map(m0), dl.host_lists()
    rec = mi.download()
    kf_idx = {}
    for kind, rem in zip(R.KINDS, (removed["pt_removed"], removed["ls_removed"])):
        kf_idx[kind] = R.lists_of(*LM.anchor_lists(m0, kind))
        R.replay_insert(kf_idx[kind], kf, rec[kind])
        R.replay_cull(kf_idx[kind], mA[kind], rem)
        assert kf_idx[kind] == R.lists_of(*LM.anchor_lists(mA, kind)), kind
    # the pose graph
    g = PG.pose_graph(n_kf=nk, seed=8)
    plan = capi.PgoPlan(ctx, g["kf_valid"], g["full_graph"], g["lc_idx"])
    res = plan.optimize(g["T_kf_w"], g["x_kf_w"], g["lc_pose"])
    plan.close()
    assert res["corrected"].sum() >= nk - 1
    # the correction: resident, and from host arrays with the replayed containers
    counts = PG.correct_image(ctx, img, res["T_corr"], res["corrected"], res["x"], dl)
    host = {}
    for kind in R.KINDS:
        ptr, idx = R.csr_of(kf_idx[kind])
        host[kind] = dict(anchor_ptr=ptr, anchor_idx=idx, valid=mA[kind]["valid"], X=mA[kind]["X"], med_dir=np.zeros((mA[kind]["n"], 3)),
                          dir_ptr=mA[kind]["obs_ptr"], dirs=listsA[kind]["dir"])
    hp, hl = capi.correct_map(ctx, res["T_corr"], res["corrected"], host["points"], host["lines"])
    mC, listsC = dict(mA), {k: dict(v) for k, v in listsA.items()}
    for kind, h in zip(R.KINDS, (hp, hl)):
        assert np.array_equal(_bits(img.host(f"{kind}.X")), _bits(h["X"])) and not np.array_equal(h["X"], mA[kind]["X"]), kind
        assert np.array_equal(_bits(dl.host(f"{kind}.dir")), _bits(h["dirs"])) and not np.array_equal(h["dirs"], listsA[kind]["dir"]), kind
        mC[kind] = dict(mA[kind], X=h["X"])
        listsC[kind]["dir"] = h["dirs"]
    co = res["corrected"]
    x_want = np.where(co[:, None], res["x"], mA["x_kf_w"].reshape(nk, 6))
    assert np.array_equal(_bits(img.host("x_kf_w")), _bits(x_want))
    mC["x_kf_w"] = x_want
    assert counts["n_pt"] == sum(len(x) for k, x in enumerate(kf_idx["points"]) if co[k]) and counts["n_pt"] > 300
    assert counts["n_ls"] == sum(len(x) for k, x in enumerate(kf_idx["lines"]) if co[k])
    # the fusion on the corrected image, and its carry
    lc = LF.synthetic_loop_closure(mC, entries=[tuple(int(v) for v in e) for e in g["lc_idx"]], points=dict(n_a=10, n_b=10, n_c=8, n_d=8),
                                   lines=dict(n_a=3, n_b=3, n_c=3, n_d=3), seed=6)
    lc["T_kf_w"] = res["T"]
    rows = ML.tuple_rows(lc, seed=7)
    capf = LF.fuse_bounds(mC, lc)
    img2 = MI.DeviceMapImage(mC, **capf, device=ctx.device, blank=BLANK)
    dl2 = ML.DeviceMapLists(None, **capf, device=ctx.device, blank=BLANK)
    lf.run(img, img2, lc)
    ml.fuse_carry(lf, img, dl, img2, dl2, rows)
    mF, out = FR.fuse(mC, lc)
    want = LR.carry_fuse(mC, mF, lc, out, listsC, rows)
    _same_image(img2, mF, "after the fusion")
    assert np.array_equal(_bits(img2.host("x_kf_w")), _bits(x_want))
    for kind in R.KINDS:
        for f in ML._fields_of(kind):
            got, w = dl2.host(f"{kind}.{f}"), np.asarray(want[kind][f])
            same = np.array_equal(_bits(got), _bits(w)) if w.dtype == np.float64 else np.array_equal(got, w)
            assert got.shape == w.shape and same, ("lists after the fusion", kind, f)
    for h in (mi, lm, lf):
        h.close()


# ---- the refusals --------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_every_array_as_it_was(ctx):
    m = LM.synthetic_map(n_kf=8, n_pt=120, n_ls=40, seed=17)
    T_corr, _, lists, med, x_new = _inputs(m, 18)
    co = np.ones(8, np.uint8)
    d = _Device(ctx, m, lists, med)
    before = d.state()
    fn = ctx._L.plslam_lc_correct_image
    Tc, xn = np.ascontiguousarray(T_corr.reshape(-1, 16)), np.ascontiguousarray(x_new)

    def dst(**kw):
        a = dict(pt_X=d.index.ptr("points.X"), pt_dir=d.lists.ptr("points.dir"), pt_med_dir=d.med["points"].data_ptr(),
                 ls_X=d.index.ptr("lines.X"), ls_dir=d.lists.ptr("lines.dir"), ls_med_dir=d.med["lines"].data_ptr(), x_kf_w=d.index.ptr("x_kf_w"))
        a.update(kw)
        return capi.LcImageDst(**a)

    def call(ctx_h=ctx.handle, index=None, T_=Tc, co_=co, dst_=None, null_map=False, null_dst=False):
        c = capi.LcImageCounts(-7, -7, -7, -7)
        s = dst() if dst_ is None else dst_
        rc = fn(ctx_h, None if null_map else C.addressof((index or d.index.struct)), capi._p(T_), capi._p(co_), capi._p(xn),
                None if null_dst else C.byref(s), C.byref(c))
        assert (c.n_pt, c.n_ls, c.n_pt_dirs, c.n_ls_dirs) == (-7, -7, -7, -7)
        return rc

    assert call(ctx_h=None) == -1 and call(null_map=True) == -1 and call(T_=None) == -1 and call(co_=None) == -1 and call(null_dst=True) == -1
    assert call(dst_=dst(pt_X=None)) == -1 and call(dst_=dst(ls_X=None)) == -1            # a kind with landmarks and no X
    assert call(dst_=dst(ls_dir=d.lists.ptr("lines.dir") + 4)) == -1                      # a misaligned destination
    for field, value in (("n_map_kf", 0), ("points.n", -1), ("lines.n_obs", -3), ("points.obs_ptr", None), ("lines.obs_kf", None),
                         ("points.valid", None)):
        bad = LM.MapIndex.from_buffer_copy(d.index.struct)                             # an image that fails map_src_kind_ok
        tgt, name = (bad, field) if "." not in field else (getattr(bad, field.split(".")[0]), field.split(".")[1])
        setattr(tgt, name, value)
        assert call(index=bad) == -1, field
    _same(d.state(), before, "after the refusals")
    c = d.correct(T_corr, co, x_new)                              # ... and the same arguments, whole, are taken
    assert c["n_pt"] > 80 and c["n_pt_dirs"] > c["n_pt"]
