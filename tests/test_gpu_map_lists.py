"""GPU tests of the map's side lists on the device (plslam_map_lists_refresh, plslam_map_insert_carry, plslam_lc_fuse_carry): desc /
dir / pts rows, med_idx / med_desc, the refreshed flags and the insert's new obs_src records BIT-EXACT against the replay of the
restatements' event records (tests/map_lists_ref.py) on every case of both case tables; untouched landmarks copied; the row
cache's split; one map of 200 000 landmarks; the chain into the map <-> keyframe matcher and the map correction; every refusal.
Everything is bytes, integers and verbatim doubles: no tolerance anywhere."""
import ctypes as C

import numpy as np
import pytest

import lc_fuse_cases as FC
import lc_fuse_ref as FR
import map_insert_cases as IC
import map_insert_ref as IR
import map_lists_ref as R
import pgo_ref
from oracle import oracle as O
from plslam_amd import lc_fuse as LF
from plslam_amd import local_map as LM
from plslam_amd import map_insert as MI
from plslam_amd import map_lists as ML
from plslam_amd.capi import PlslamError

pytestmark = pytest.mark.gpu
BLANK = 90                                                       # what a destination holds before the call writes it
T = MI.LOOKBACK_TILE


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


def _same_lists(dl, want, what=""):
    """the live part equals the replay, and everything beyond it still holds the blank byte"""
    for kind in R.KINDS:
        W = want[kind]
        for f in ML._fields_of(kind):
            got = dl.host(f"{kind}.{f}")
            w = np.asarray(W[f])
            assert got.shape == w.shape and got.dtype == w.dtype, (what, kind, f, got.shape, w.shape, got.dtype, w.dtype)
            assert np.array_equal(_bits(got), _bits(w)), (what, kind, f, np.flatnonzero((_bits(got) != _bits(w)).reshape(got.shape[0], -1).any(axis=1))[:8])
            rest = dl.raw(f"{kind}.{f}")[got.shape[0]:]
            assert (np.ascontiguousarray(rest).view(np.uint8) == BLANK).all(), (what, kind, f, "rows beyond the live part were written")


def _unchanged(sl, lists, what=""):
    for kind in R.KINDS:
        for f in ML._fields_of(kind):
            if f in lists[kind] and f != "refreshed":
                assert np.array_equal(_bits(sl.host(f"{kind}.{f}")), _bits(np.asarray(lists[kind][f]))), (what, kind, f, "the source lists changed")


def _insert_passes(ctx, r):
    """the two inserts of a case on the device with their carries, the second pair on what the first left there"""
    m, kf, kf_b = r["m"], r["kf"], r["kf_b"]
    mi, ml = MI.MapInsert(ctx), ML.MapLists(ctx)
    src = LM.DeviceMapIndex(m, ctx.device)
    cap = MI.insert_bounds(m, kf, "kf2kf")
    dst = MI.DeviceMapImage(m, **cap, device=ctx.device, blank=BLANK)
    sl = ML.DeviceMapLists(r["lists0"], device=ctx.device)
    dl = ML.DeviceMapLists(None, **cap, device=ctx.device, blank=BLANK)
    mi.kf2kf(src, dst, kf)
    ml.insert_carry(mi, src, sl, dst, dl, r["rows_a"])
    rec = mi.download()
    for kind in R.KINDS:
        assert np.array_equal(rec[kind]["obs_src"], r["want_a"][kind]["obs_src"]), ("kf2kf", kind, "obs_src")
    _same_lists(dl, r["want_a"], "kf2kf")
    _unchanged(sl, r["lists0"], "kf2kf")
    cap_b = MI.insert_bounds(r["m_a"], kf_b, "map2kf")
    dst2 = MI.DeviceMapImage(m, **cap_b, device=ctx.device, blank=BLANK)
    dl2 = ML.DeviceMapLists(None, **cap_b, device=ctx.device, blank=BLANK)
    mi.map2kf(dst, dst2, kf_b)
    ml.insert_carry(mi, dst, dl, dst2, dl2, r["rows_b"])
    rec = mi.download()
    for kind in R.KINDS:
        assert np.array_equal(rec[kind]["obs_src"], r["want_b"][kind]["obs_src"]), ("map2kf", kind, "obs_src")
    _same_lists(dl2, r["want_b"], "map2kf")
    _same_lists(dl, r["want_a"], "the source of the second carry")
    mi.close()
    return dl, dl2


def _fuse_pass(ctx, r):
    m, lc = r["m"], r["lc"]
    lf, ml = LF.LcFuse(ctx), ML.MapLists(ctx)
    src = LM.DeviceMapIndex(m, ctx.device)
    cap = LF.fuse_bounds(m, lc)
    dst = MI.DeviceMapImage(m, **cap, device=ctx.device, blank=BLANK)
    sl = ML.DeviceMapLists(r["lists0"], device=ctx.device)
    dl = ML.DeviceMapLists(None, **cap, device=ctx.device, blank=BLANK)
    lf.run(src, dst, lc)
    ml.fuse_carry(lf, src, sl, dst, dl, r["rows"])
    _same_lists(dl, r["want"], "fuse")
    _unchanged(sl, r["lists0"], "fuse")
    lf.close()
    return dl


# ---- 1, 5: every case of the insert's table (no_events among them) ------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(IC.CASES))
def test_insert_cases_equal_the_replay(ctx, name):
    r = R.run_insert(name)
    _insert_passes(ctx, r)
    if name.startswith("tile_events"):                            # the touched count at the tile's edge, both kinds, both passes
        n = T + int(name.rsplit("_", 1)[1])
        assert r["want_a"]["points"]["refreshed"].sum() == r["want_a"]["lines"]["refreshed"].sum() == r["want_b"]["points"]["refreshed"].sum() == n
    if name.startswith("tile_landmarks"):
        assert r["want_a"]["points"]["med_idx"].size == r["want_a"]["lines"]["med_idx"].size == T + int(name.rsplit("_", 1)[1])
    if name == "no_events":                                       # a pure copy
        for want, lists in ((r["want_a"], r["lists0"]), (r["want_b"], r["want_a"])):
            for kind in R.KINDS:
                assert not want[kind]["refreshed"].any()
                assert all(np.array_equal(_bits(want[kind][f]), _bits(lists[kind][f])) for f in lists[kind] if f not in ("refreshed", "obs_src"))


# ---- 2: every case of the fusion's table -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(n for n in FC.CASES if n != "level_over"))
def test_fuse_cases_equal_the_replay(ctx, name):
    r = R.run_fuse(name)
    _fuse_pass(ctx, r)
    if name == "only_d":                                          # dead landmarks: -1, zero bytes, refreshed
        for kind in R.KINDS:
            dead = r["out"][kind]["ev"][r["out"][kind]["ev"][:, 0] == 4][:, 2]
            W = r["want"][kind]
            assert dead.size >= 30 and (W["med_idx"][dead] == -1).all() and not W["med_desc"][dead].any() and W["refreshed"][dead].all()
    if name.startswith("tile_events"):
        n = T + int(name.rsplit("_", 1)[1])
        assert r["want"]["points"]["refreshed"].sum() == r["want"]["lines"]["refreshed"].sum() == n


# ---- 3: untouched means copied ---------------------------------------------------------------------------------------------------
def test_untouched_landmarks_are_copied_not_recomputed(ctx):
    """the source med_idx / med_desc are each list's LAST row: untouched landmarks still hold that, touched ones the representative"""
    r = R.run_insert("mixed", True, True)
    dl, _ = _insert_passes(ctx, r)
    f = R.run_fuse("three_entries", True, True)
    dlf = _fuse_pass(ctx, f)
    for got, want, lens, m_after in ((dl, r["want_a"], r["m"], r["m_a"]), (dlf, f["want"], f["m"], f["m_a"])):
        for kind in R.KINDS:
            n_src = lens[kind]["n"]
            ln = np.diff(lens[kind]["obs_ptr"])
            idx, ref = got.host(f"{kind}.med_idx"), got.host(f"{kind}.refreshed")
            same = np.flatnonzero(ref[:n_src] == 0)
            assert same.size > 20 and np.array_equal(idx[same], ln[same] - 1)
            true_idx, true_med = O.median_desc_batched(got.host(f"{kind}.desc"), m_after[kind]["obs_ptr"].astype(np.int32))
            t = np.flatnonzero(ref & (np.diff(m_after[kind]["obs_ptr"]) > 0))
            assert t.size >= 5 and np.array_equal(idx[t], true_idx[t]) and np.array_equal(got.host(f"{kind}.med_desc")[t], true_med[t])
            assert (true_idx[same] != ln[same] - 1).any()


# ---- 4: the row-cache split -------------------------------------------------------------------------------------------------------
def _map_with_long_lists(seed):
    """the base map with the points' lists redrawn: landmarks 0, 1, 2 have 15, 16, 17 observations, 3 and 4 have 9 each"""
    rng = np.random.Generator(np.random.PCG64(seed))
    m = dict(IC.base_map())
    P = dict(m["points"])
    lens = rng.integers(1, 5, P["n"])
    lens[:5] = (15, 16, 17, 9, 9)
    ptr = np.zeros(P["n"] + 1, np.int32)
    ptr[1:] = np.cumsum(lens)
    valid = P["valid"].copy()
    valid[:5] = 1
    P.update(obs_ptr=ptr, obs_kf=rng.integers(0, m["n_map_kf"], ptr[-1]).astype(np.int32), obs_val=rng.uniform(0.0, 700.0, (ptr[-1], 2)), valid=valid)
    m["points"] = P
    return m


@pytest.mark.parametrize("clustered", [True, False])
def test_row_cache_split(ctx, clustered):
    """lists that go 15 -> 16, 16 -> 17 and 17 -> 18 by an append (the row of conf in LDS up to 16, recomputed beyond) and a D
    fusion of 9 + 9; the result equals oracle.median_desc_batched"""
    m0 = _map_with_long_lists(21)
    m, kf = MI.synthetic_keyframe(m0, 96, 32, 4, {}, {})
    tab = np.full(m["points"]["n"], -1, np.int32)
    tab[:3] = (5, 6, 7)
    kf_b = dict(kf2=kf["kf2"], T2=kf["T2"], points=dict(table=tab, P2=kf["points"]["P2"], obs2=kf["points"]["obs2"]), lines=None)
    m_b, out_b = IR.insert_map2kf(m, kf_b)
    lists0 = ML.synthetic_lists(m, seed=31, clustered=clustered)
    rows = dict(points={k: v for k, v in ML.keyframe_rows(kf, seed=32, clustered=clustered)["points"].items() if k == "desc2"}, lines=None)
    want = R.carry_insert(m, m_b, dict(kf_b, kf1=-1), out_b, lists0, rows)
    assert np.diff(m_b["points"]["obs_ptr"])[:3].tolist() == [16, 17, 18] and want["points"]["refreshed"][:3].all()
    mi, ml = MI.MapInsert(ctx), ML.MapLists(ctx)
    src = LM.DeviceMapIndex(m, ctx.device)
    cap = MI.insert_bounds(m, kf_b, "map2kf")
    dst = MI.DeviceMapImage(m, **cap, device=ctx.device, blank=BLANK)
    sl, dl = ML.DeviceMapLists(lists0, device=ctx.device), ML.DeviceMapLists(None, **cap, device=ctx.device, blank=BLANK)
    mi.map2kf(src, dst, kf_b)
    ml.insert_carry(mi, src, sl, dst, dl, rows)
    _same_lists(dl, want, "appends")
    oi, om = O.median_desc_batched(dl.host("points.desc"), m_b["points"]["obs_ptr"].astype(np.int32))
    assert np.array_equal(dl.host("points.med_idx")[:3], oi[:3]) and np.array_equal(dl.host("points.med_desc")[:3], om[:3])
    mi.close()
    # the D fusion of 9 + 9 (18 rows: beyond the cache) on the same map without the keyframe
    f = LF.pack_loop_closure(m0, [(3, 30, 1)], points=[[(3, 0, 4, _feature(m0, 30))]], lines=None, seed=5)
    m_f, out_f = FR.fuse(m0, f)
    assert out_f["points"]["counts"]["n_d"] == 1 and np.diff(m_f["points"]["obs_ptr"])[3:5].tolist() == [18, 0]
    lists_f = ML.synthetic_lists(m0, seed=33, clustered=clustered)
    rows_f = ML.tuple_rows(f, seed=34, clustered=clustered)
    want_f = R.carry_fuse(m0, m_f, f, out_f, lists_f, rows_f)
    dlf = _fuse_pass(ctx, dict(m=m0, lc=f, lists0=lists_f, rows=rows_f, want=want_f))
    oi, om = O.median_desc_batched(dlf.host("points.desc"), m_f["points"]["obs_ptr"].astype(np.int32))
    assert dlf.host("points.med_idx")[3] == oi[3] and np.array_equal(dlf.host("points.med_desc")[3], om[3]) and dlf.host("points.med_idx")[4] == -1


def _feature(m, kf):
    f = m["points"]["feat_idx"][m["points"]["feat_ptr"][kf]:m["points"]["feat_ptr"][kf + 1]]
    return int(np.flatnonzero(f != LM.FEAT_NULL)[0])


# ---- 6: the full refresh ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("long_lists", [False, True])
def test_refresh_equals_the_oracle_over_the_whole_map(ctx, long_lists):
    m = _map_with_long_lists(22) if long_lists else IC.base_map()
    lists = ML.synthetic_lists(m, seed=41, clustered=True)
    lens = np.diff(m["points"]["obs_ptr"])
    assert (lens == 0).any() or long_lists
    assert (lens == 1).any() and (np.diff(m["lines"]["obs_ptr"]) == 0).any()
    planted = {k: dict(v, med_idx=np.full_like(v["med_idx"], 77), med_desc=np.full_like(v["med_desc"], 7)) for k, v in lists.items()}
    dl = ML.DeviceMapLists(planted, device=ctx.device)
    ml = ML.MapLists(ctx)
    ml.refresh(LM.DeviceMapIndex(m, ctx.device), dl)
    for kind in R.KINDS:
        oi, om = O.median_desc_batched(lists[kind]["desc"], m[kind]["obs_ptr"].astype(np.int32))
        e = np.diff(m[kind]["obs_ptr"]) == 0
        assert np.array_equal(dl.host(f"{kind}.med_idx"), oi) and (oi[e] == -1).all()
        assert np.array_equal(dl.host(f"{kind}.med_desc")[~e], om[~e]) and not dl.host(f"{kind}.med_desc")[e].any()
        assert (dl.host(f"{kind}.refreshed") == 1).all()
        assert np.array_equal(dl.host(f"{kind}.desc"), lists[kind]["desc"])


# ---- 7: the chain the feature exists for ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["points", "lines"])
def test_carried_representatives_feed_the_map2kf_matcher(ctx, kind):
    """insert -> carry -> plslam_map2kf_match_*_dev with dst_lists.med_desc where it lies: the table the same call gives when fed a
    med_desc computed on the host from the replayed lists"""
    import torch
    import plslam_amd
    from plslam_amd import synth
    from test_map2kf import fast_cfg, scene
    lines = kind == "lines"
    n_map, n_kf = (600, 150) if lines else (1500, 400)
    s = scene(n_map, n_kf, lines=lines, seed=5)
    m0 = LM.synthetic_map(n_kf=25, n_pt=10 if lines else n_map, n_ls=n_map if lines else 10, seed=41)
    m0[kind]["X"] = np.ascontiguousarray(s["LM"], np.float64)
    mix = dict(n_new=10, n_exist=40, n_same_lm=3)
    m, kf = MI.synthetic_keyframe(m0, 96, 96, 3, None if lines else mix, mix if lines else None)
    lists0 = ML.synthetic_lists(m, seed=51, clustered=True)
    ptr = np.asarray(m[kind]["obs_ptr"], np.int64)
    rng = np.random.Generator(np.random.PCG64(52))                # the landmark's lists are noisy copies of the scene's descriptor
    lists0[kind]["desc"] = np.ascontiguousarray(np.repeat(s["med"], np.diff(ptr), axis=0) ^ np.packbits(rng.random((int(ptr[-1]), 256)) < 0.02, axis=1))
    lists0[kind]["med_idx"], lists0[kind]["med_desc"] = ML.representative(lists0[kind]["desc"], ptr)
    rows = ML.keyframe_rows(kf, seed=53)
    m_a, out_a = IR.insert_kf2kf(m, kf)
    want = R.carry_insert(m, m_a, kf, out_a, lists0, rows)
    mi, ml = MI.MapInsert(ctx), ML.MapLists(ctx)
    src = LM.DeviceMapIndex(m, ctx.device)
    cap = MI.insert_bounds(m, kf, "kf2kf")
    dst = MI.DeviceMapImage(m, **cap, device=ctx.device, blank=BLANK)
    sl, dl = ML.DeviceMapLists(lists0, device=ctx.device), ML.DeviceMapLists(None, **cap, device=ctx.device, blank=BLANK)
    mi.kf2kf(src, dst, kf)
    ml.insert_carry(mi, src, sl, dst, dl, rows)
    n_dst = m_a[kind]["n"]
    assert n_dst == n_map + 10 and want[kind]["refreshed"].sum() >= 50
    dev = torch.device("cuda", ctx.device)
    d_cand = torch.ones(n_dst, dtype=torch.uint8, device=dev)
    d_host_med = torch.from_numpy(want[kind]["med_desc"]).to(dev)
    cam = plslam_amd.make_cam(**synth.EUROC)
    tail = (n_dst, s["kf_desc"], s["kf_feat"], s["kf_idx"], 0.9, True, 1.5, 10, fast_cfg())
    got = ctx.map2kf_match_dev(kind, cam, s["Twf"], dst.ptr(f"{kind}.X"), dl.ptr(f"{kind}.med_desc"), d_cand.data_ptr(), *tail, kf_seg=s.get("kf_seg"))
    ref = ctx.map2kf_match_dev(kind, cam, s["Twf"], dst.ptr(f"{kind}.X"), d_host_med.data_ptr(), d_cand.data_ptr(), *tail, kf_seg=s.get("kf_seg"))
    assert ref[1] > 20 and got[1] == ref[1] and got[2] == ref[2]
    np.testing.assert_array_equal(got[0], ref[0])
    _same_lists(dl, want, "chain")
    mi.close()


def test_carried_directions_feed_the_map_correction(ctx):
    """plslam_lc_correct_map_dev with dir_ptr = the image's obs_ptr and dirs = the carried dir list, in place: the restatement on the
    replayed directions"""
    import torch
    from plslam_amd import capi
    r = R.run_fuse("three_entries")
    m, lc, m_a = r["m"], r["lc"], r["m_a"]
    lf, ml = LF.LcFuse(ctx), ML.MapLists(ctx)
    src = LM.DeviceMapIndex(m, ctx.device)
    cap = LF.fuse_bounds(m, lc)
    dst = MI.DeviceMapImage(m, **cap, device=ctx.device, blank=BLANK)
    sl, dl = ML.DeviceMapLists(r["lists0"], device=ctx.device), ML.DeviceMapLists(None, **cap, device=ctx.device, blank=BLANK)
    lf.run(src, dst, lc)
    ml.fuse_carry(lf, src, sl, dst, dl, r["rows"])
    P, nk = m_a["points"], m_a["n_map_kf"]
    n = P["n"]
    rng = np.random.Generator(np.random.PCG64(61))
    home = rng.integers(0, nk, n)                                 # every landmark anchored at one slot
    order = np.argsort(home, kind="stable").astype(np.int32)
    anchor_ptr = np.zeros(nk + 1, np.int32)
    anchor_ptr[1:] = np.cumsum(np.bincount(home, minlength=nk))
    med_dir = rng.standard_normal((n, 3))
    T_corr = np.stack([MI._pose(rng) for _ in range(nk)])
    corrected = (rng.random(nk) < 0.6).astype(np.uint8)
    dev = torch.device("cuda", ctx.device)
    keep = {k: torch.from_numpy(np.ascontiguousarray(a)).to(dev) for k, a in dict(anchor_ptr=anchor_ptr, anchor_idx=order, med_dir=med_dir,
                                                                                  T=T_corr.reshape(-1, 16), co=corrected).items()}
    pp = dict(n=n, n_anchor=n, n_dir=P["obs_kf"].size, anchor_ptr=keep["anchor_ptr"].data_ptr(), anchor_idx=keep["anchor_idx"].data_ptr(),
              valid=dst.ptr("points.valid"), X=dst.ptr("points.X"), med_dir=keep["med_dir"].data_ptr(), dir_ptr=dst.ptr("points.obs_ptr"),
              dirs=dl.ptr("points.dir"))
    capi.correct_map_dev(ctx, nk, keep["T"].data_ptr(), keep["co"].data_ptr(), pp, None)
    X, med, dirs = pgo_ref.correct_landmarks(T_corr, corrected, anchor_ptr, order, P["valid"], P["X"], med_dir, P["obs_ptr"], r["want"]["points"]["dir"])
    assert np.array_equal(_bits(dl.host("points.dir")), _bits(dirs)) and not np.array_equal(dirs, r["want"]["points"]["dir"])
    assert np.array_equal(_bits(dst.host("points.X")), _bits(X)) and np.array_equal(_bits(keep["med_dir"].cpu().numpy()), _bits(med))
    lf.close()


# ---- 8: one large map -------------------------------------------------------------------------------------------------------------------
def test_two_hundred_thousand_landmarks(ctx):
    r = R.run_insert("big")
    _insert_passes(ctx, r)
    assert r["m"]["points"]["n"] == 200_000 and r["want_a"]["points"]["refreshed"].sum() == 1950 and r["want_a"]["points"]["desc"].shape[0] > 480_000


# ---- 9: the refusals ------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_destination_untouched(ctx):
    r = R.run_insert("mixed")
    m, kf = r["m"], r["kf"]
    L = ctx._L
    mi, ml = MI.MapInsert(ctx), ML.MapLists(ctx)
    src = LM.DeviceMapIndex(m, ctx.device)
    cap = MI.insert_bounds(m, kf, "kf2kf")
    dst = MI.DeviceMapImage(m, **cap, device=ctx.device, blank=BLANK)
    sl = ML.DeviceMapLists(r["lists0"], device=ctx.device)
    dl = ML.DeviceMapLists(None, **cap, device=ctx.device, blank=BLANK)
    rows = ML.insert_rows(r["rows_a"], ctx.device)
    fn = L.plslam_map_insert_carry

    def call(h=None, s=None, sL=None, d=None, dL=None, pt=0, ls=0):
        a = rows.addresses()
        return fn(mi._h if h is None else h, C.addressof((s or src).struct), C.addressof((sL or sl).struct), C.addressof((d or dst).struct),
                  C.addressof((dL or dl).struct), a[0] if pt == 0 else pt, a[1] if ls == 0 else ls)

    def blank():
        for kind in R.KINDS:
            for f in ML._fields_of(kind):
                assert (np.ascontiguousarray(dl.raw(f"{kind}.{f}")).view(np.uint8) == BLANK).all(), (kind, f)

    assert call() == -1                                           # no insert on the handle yet
    mi.kf2kf(src, dst, kf)
    a = rows.addresses()
    for args in ((None, C.addressof(src.struct), C.addressof(sl.struct), C.addressof(dst.struct), C.addressof(dl.struct), a[0], a[1]),
                 (mi._h, None, C.addressof(sl.struct), C.addressof(dst.struct), C.addressof(dl.struct), a[0], a[1]),
                 (mi._h, C.addressof(src.struct), None, C.addressof(dst.struct), C.addressof(dl.struct), a[0], a[1]),
                 (mi._h, C.addressof(src.struct), C.addressof(sl.struct), None, C.addressof(dl.struct), a[0], a[1]),
                 (mi._h, C.addressof(src.struct), C.addressof(sl.struct), C.addressof(dst.struct), None, a[0], a[1])):
        assert fn(*args) == -1                                    # NULL arguments
    assert call(s=dst) == -1 and call(d=src) == -1                # counts that are not the call's
    assert call(pt=None) == -1 and call(ls=None) == -1            # a kind with events without its rows
    one_side = ML.insert_rows(dict(points=r["rows_a"]["points"], lines=dict(r["rows_a"]["lines"], pts1=None)), ctx.device)
    assert call(ls=one_side.addresses()[1]) == -1                 # pts on one side only
    no_pts = ML.MapListsStruct.from_buffer_copy(dl.struct)
    no_pts.lines.pts = None
    assert fn(mi._h, C.addressof(src.struct), C.addressof(sl.struct), C.addressof(dst.struct), C.addressof(no_pts), a[0], a[1]) == -1
    for f in ("desc", "med_idx", "med_desc"):                     # a destination list that is a source list
        alias = ML.MapListsStruct.from_buffer_copy(dl.struct)
        setattr(alias.points, f, getattr(sl.struct.points, f))
        assert fn(mi._h, C.addressof(src.struct), C.addressof(sl.struct), C.addressof(dst.struct), C.addressof(alias), a[0], a[1]) == -1, f
    odd = ML.MapListsStruct.from_buffer_copy(dl.struct)           # a misaligned list
    odd.points.desc = dl.struct.points.desc + 4
    assert fn(mi._h, C.addressof(src.struct), C.addressof(sl.struct), C.addressof(dst.struct), C.addressof(odd), a[0], a[1]) == -1
    host_mem = np.zeros((cap["pt_obs_cap"] + 1, 32), np.uint8)    # a list that is not the device's memory
    off = ML.MapListsStruct.from_buffer_copy(dl.struct)
    off.points.desc = (host_mem.ctypes.data + 15) & ~15
    assert fn(mi._h, C.addressof(src.struct), C.addressof(sl.struct), C.addressof(dst.struct), C.addressof(off), a[0], a[1]) == -1
    assert not host_mem.any()
    ml.sync()
    blank()
    # an insert refused in front of its launch leaves the last records valid: the carry of the earlier insert still runs
    small = MI.DeviceMapImage(m, **dict(cap, pt_cap=cap["pt_cap"] - 1), device=ctx.device, blank=BLANK)
    with pytest.raises(PlslamError):
        mi.kf2kf(src, small, kf)
    assert call() == 0
    ml.sync()
    dl.counts = {k: (Lk.n, Lk.n_obs) for k, Lk in (("points", dst.struct.points), ("lines", dst.struct.lines))}
    _same_lists(dl, r["want_a"], "after the refusals")            # the handle and the lists are still usable
    # the refresh's and the fusion's refusals
    assert L.plslam_map_lists_refresh(None, C.addressof(src.struct), C.addressof(sl.struct)) == -1
    assert L.plslam_map_lists_refresh(ctx.handle, None, C.addressof(sl.struct)) == -1
    assert L.plslam_map_lists_refresh(ctx.handle, C.addressof(src.struct), None) == -1
    lf = LF.LcFuse(ctx)
    assert L.plslam_lc_fuse_carry(lf._h, C.addressof(src.struct), C.addressof(sl.struct), C.addressof(dst.struct), C.addressof(dl.struct), None, None) == -1
    assert L.plslam_lc_fuse_carry(None, None, None, None, None, None, None) == -1
    f = R.run_fuse("level_limit")                                 # a run the device refuses (ERANGE) invalidates the records
    over = FC.run_ref("level_over")
    fsrc = LM.DeviceMapIndex(f["m"], ctx.device)
    fcap = LF.fuse_bounds(f["m"], f["lc"])
    fdst = MI.DeviceMapImage(f["m"], **fcap, device=ctx.device, blank=BLANK)
    fsl, fdl = ML.DeviceMapLists(f["lists0"], device=ctx.device), ML.DeviceMapLists(None, **fcap, device=ctx.device, blank=BLANK)
    lf.run(fsrc, fdst, f["lc"])
    with pytest.raises(PlslamError) as e:
        lf.run(fsrc, MI.DeviceMapImage(over[0], **LF.fuse_bounds(over[0], over[1]), device=ctx.device, blank=BLANK), over[1])
    assert e.value.code == -5
    with pytest.raises(PlslamError) as e:
        ml.fuse_carry(lf, fsrc, fsl, fdst, fdl, f["rows"])
    assert e.value.code == -1
    lf.run(fsrc, fdst, f["lc"])
    ml.fuse_carry(lf, fsrc, fsl, fdst, fdl, f["rows"])
    _same_lists(fdl, f["want"], "the fusion after its refusal")
    lf.close()
    mi.close()
