"""GPU tests of the map insertion on the device (plslam_map_insert_*): every array of the destination image, the event records,
row_delta and the counts BIT-EXACT against the sequential restatement (tests/map_insert_ref.py) on the shared cases
(tests/map_insert_cases.py): the KF <-> KF insert, then the map <-> KF insert on the image the first one left on the device; on one
map of 200 000 landmarks; chained with the local map's calls; and the refusals."""
import numpy as np
import pytest

import local_map_ref as LR
import map_insert_cases as CS
import map_insert_ref as R
from plslam_amd import local_map as LM
from plslam_amd import map_insert as MI
from plslam_amd.capi import PlslamError

pytestmark = pytest.mark.gpu

_FIELDS = ("valid", "inlier", "X", "obs_ptr", "obs_kf", "obs_val", "feat_ptr", "feat_idx")
BLANK = 90                                                       # what a destination holds before the call writes it


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


def _same_image(img, want):
    assert img.struct.n_map_kf == want["n_map_kf"]
    assert np.array_equal(img.host("kf_valid"), want["kf_valid"])
    assert np.array_equal(_bits(img.host("x_kf_w")), _bits(want["x_kf_w"].ravel()))
    for kind, L in (("points", img.struct.points), ("lines", img.struct.lines)):
        W = want[kind]
        assert (L.n, L.n_obs, L.n_feat) == (W["n"], W["obs_kf"].size, W["feat_idx"].size), kind
        for f in _FIELDS:
            got = img.host(f"{kind}.{f}")
            assert got.shape == W[f].shape and got.dtype == W[f].dtype, (kind, f, got.shape, W[f].shape)
            assert np.array_equal(_bits(got), _bits(W[f])), (kind, f)


def _same_out(got, ev, want):
    assert np.array_equal(got["row_delta"], want["row_delta"])
    for kind in ("points", "lines"):
        assert got[kind] == want[kind]["counts"], kind
        assert np.array_equal(ev[kind]["ev"], want[kind]["ev"]), kind
        assert np.array_equal(_bits(ev[kind]["dir"]), _bits(want[kind]["dir"])), kind


def _both_passes(ctx, name, handle=None):
    """the two inserts of a case on the device, the second one on the image the first one left there; on `handle` where one is
    given, else on a handle of their own"""
    m, kf, (m_a, out_a), kf_b, (m_b, out_b), _ = CS.run_ref(name)
    mi = handle or MI.MapInsert(ctx)
    src = LM.DeviceMapIndex(m, ctx.device)
    dst = MI.DeviceMapImage(m, **MI.insert_bounds(m, kf, "kf2kf"), device=ctx.device, blank=BLANK)
    got = mi.kf2kf(src, dst, kf)
    _same_out(got, mi.download(), out_a)
    _same_image(dst, m_a)
    dst2 = MI.DeviceMapImage(m, **MI.insert_bounds(m_a, kf_b, "map2kf"), device=ctx.device, blank=BLANK)
    got = mi.map2kf(dst, dst2, kf_b)
    _same_out(got, mi.download(), out_b)
    _same_image(dst2, m_b)
    _same_image(dst, m_a)                                        # the source of the second call is read, not written
    if handle is None:
        mi.close()
    return out_a, out_b


@pytest.mark.parametrize("name", sorted(CS.CASES))
def test_cases_equal_the_restatement(ctx, name):
    a, b = _both_passes(ctx, name)
    if name.startswith("tile_events"):
        n = CS.T + int(name.rsplit("_", 1)[1])
        assert a["points"]["counts"]["n_events"] == a["lines"]["counts"]["n_new"] == b["points"]["counts"]["n_events"] == n
    if name.startswith("tile_landmarks"):
        m_a = CS.run_ref(name)[2][0]
        assert m_a["points"]["n"] == m_a["lines"]["n"] == CS.T + int(name.rsplit("_", 1)[1])
    if name == "no_events":
        assert a["points"]["counts"]["n_events"] == 0 and not a["row_delta"].any()


def test_a_smaller_case_after_a_larger_one_on_one_handle(ctx):
    """the handle's buffer is carved anew by every call: a case, then one without any event (every event slice shrinks to its
    slack, everything behind moves), then the first again, each equal to the restatement"""
    mi = MI.MapInsert(ctx)
    for name in ("mixed", "no_events", "mixed"):
        _both_passes(ctx, name, mi)
    mi.close()


def test_the_tile_the_cases_are_built_around_is_the_kernels():
    import os
    import re
    import lc_fuse_cases
    import local_map_cases
    from plslam_amd import lc_fuse as LF
    src = open(os.path.join(os.path.dirname(os.path.abspath(MI.__file__)), "csrc", "map_image.hpp")).read()
    tile = int(re.search(r"constexpr int MAP_TILE = (\d+);", src).group(1))
    assert tile == LM.LOOKBACK_TILE == MI.LOOKBACK_TILE == LF.LOOKBACK_TILE == CS.T == lc_fuse_cases.T == local_map_cases.T


def test_two_hundred_thousand_landmarks(ctx):
    """the many-tile path: the event scan crosses 9 tiles, the obs_ptr scan 784; 50 landmarks take two events each"""
    a, b = _both_passes(ctx, "big")
    assert a["points"]["counts"] == dict(n_events=2000, n_new=600, n_appended=2600, n_skipped=0)
    assert CS.run_ref("big")[0]["points"]["n"] == 200_000 and b["points"]["counts"]["n_events"] == 94


def test_chain_with_the_local_map(ctx):
    """addKeyFrame's order on the device: insert_kf2kf -> plslam_local_map_candidates on the destination -> insert_map2kf of
    candidates only -> form / gather on ITS destination; every step equals the same chain of restatements"""
    m, kf, _ = CS._base(dict(n_new=15, n_exist=30, n_same_lm=3, genuine=0.3), dict(n_new=6, n_exist=8), seed=21)
    p = dict(anchor=kf["kf2"], min_cov=75, window=3)
    m_a, out_a = R.insert_kf2kf(m, kf)
    mi, lm = MI.MapInsert(ctx), LM.LocalMap(ctx)
    dst = MI.DeviceMapImage(m, **MI.insert_bounds(m, kf, "kf2kf"), device=ctx.device, blank=BLANK)
    got = mi.kf2kf(LM.DeviceMapIndex(m, ctx.device), dst, kf)
    # the local map of the new keyframe, with the row the caller keeps: full_graph[kf2] += row_delta
    row = m["row"] + got["row_delta"]
    assert np.array_equal(got["row_delta"], out_a["row_delta"])
    m_a["row"] = row
    lm.form(dst, p["anchor"], row, p["min_cov"], p["window"])
    lm.candidates(dst, kf["kf2"])
    kf_l, pt_l, ls_l = LR.form(m_a, p["anchor"], p["min_cov"], p["window"])
    cand = dict(points=LR.candidates(m_a, "points", pt_l, kf["kf2"]), lines=LR.candidates(m_a, "lines", ls_l, kf["kf2"]))
    c = lm.download("pt_candidate", "ls_candidate")
    assert np.array_equal(c["pt_candidate"], cand["points"]) and np.array_equal(c["ls_candidate"], cand["lines"])
    assert 20 < cand["points"].sum() < m_a["points"]["n"] and not cand["points"][out_a["points"]["ev"][:, 0]].any()
    kf_b = MI.synthetic_map2kf(m_a, kf, seed=5, points=dict(n_events=20), lines=dict(n_events=6), candidates=cand)
    m_b, out_b = R.insert_map2kf(m_a, kf_b)
    dst2 = MI.DeviceMapImage(m, **MI.insert_bounds(m_a, kf_b, "map2kf"), device=ctx.device, blank=BLANK)
    got = mi.map2kf(dst, dst2, kf_b)
    _same_out(got, mi.download(), out_b)
    _same_image(dst2, m_b)
    row = row + got["row_delta"]
    m_b["row"] = row
    counts = lm.form(dst2, p["anchor"], row, p["min_cov"], p["window"])
    counts.update(lm.gather(dst2))
    g = lm.download()
    kf_l, pt_l, ls_l = LR.form(m_b, p["anchor"], p["min_cov"], p["window"])
    ref = LR.gather(m_b, kf_l, pt_l, ls_l)
    assert counts["n_pt_obs"] == len(ref["pt_obs"]) > 100 and counts["n_ls_obs"] == len(ref["ls_obs"]) > 20
    for k in ("kf_list", "pt_list", "ls_list", "pt_obs", "ls_obs", "pt_obs_uv", "ls_l_obs", "X_aux"):
        assert np.array_equal(_bits(g[k]), _bits(ref[k])), k
    assert np.isin(out_b["points"]["ev"][:, 0], ref["pt_list"]).all()      # the landmarks just matched are in the problem
    mi.close()
    lm.close()


def test_refusals_leave_the_destination_untouched(ctx):
    m, kf, _, _, _, _ = CS.run_ref("mixed")
    need = MI.insert_bounds(m, kf, "kf2kf")
    mi = MI.MapInsert(ctx)
    src = LM.DeviceMapIndex(m, ctx.device)
    names = [f"{k}.{f}" for k in ("points", "lines") for f in _FIELDS if f != "feat_ptr"]
    for short in sorted(need):                                    # each capacity one below the bound the tables give: ERANGE
        dst = MI.DeviceMapImage(m, **dict(need, **{short: need[short] - 1}), device=ctx.device, blank=BLANK)
        with pytest.raises(PlslamError) as e:
            mi.kf2kf(src, dst, kf)
        assert e.value.code == -5, short
        for nm in names:
            assert (dst.raw(nm) == BLANK).all(), (short, nm)
        assert dst.struct.points.n == 0 and dst.struct.lines.n_obs == 0
    need_b = MI.insert_bounds(m, dict(kf2=kf["kf2"], points=kf["points"], lines=None), "map2kf")
    dst = MI.DeviceMapImage(m, **need, device=ctx.device, blank=BLANK)
    bad = [dict(kf, kf1=kf["kf2"]), dict(kf, kf1=-1), dict(kf, kf2=m["n_map_kf"]), dict(kf, kf1=m["n_map_kf"])]
    for k in bad:                                                 # bad slots: EINVAL
        with pytest.raises(PlslamError) as e:
            mi.kf2kf(src, dst, k)
        assert e.value.code == -1
    with pytest.raises(PlslamError) as e:                         # a map_to_kf longer than the map
        mi.map2kf(src, dst, dict(kf2=kf["kf2"], T2=kf["T2"], lines=None, points=dict(
            table=np.zeros(m["points"]["n"] + 1, np.int32), P2=kf["points"]["P2"], obs2=kf["points"]["obs2"])))
    assert e.value.code == -1 and need_b["pt_cap"] == m["points"]["n"]
    with pytest.raises(PlslamError) as e:                         # the destination is the source
        mi.kf2kf(dst, dst, kf)
    assert e.value.code == -1
    L = ctx._L
    assert L.plslam_map_insert_kf2kf(None, None, None, 0, 1, None, None, None, None, None, None) == -1
    assert L.plslam_map_insert_map2kf(mi._h, None, None, 0, None, None, None, None, None) == -1
    assert L.plslam_map_insert_device_buffers(mi._h, None) == -1
    for nm in names:
        assert (dst.raw(nm) == BLANK).all(), nm
    # a kf2kf table beyond the documented limit: ERANGE
    big = dict(kf, points=dict(kf["points"], table=np.full(MI.MAX_TABLE + 1, -1, np.int32)))
    with pytest.raises(PlslamError) as e:
        mi.kf2kf(src, dst, big)
    assert e.value.code == -5
    assert mi.kf2kf(src, dst, kf)["points"]["n_events"] > 0       # and the handle still works
    mi.close()
