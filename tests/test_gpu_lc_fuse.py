"""GPU tests of the loop-closure landmark fusion on the device (plslam_lc_fuse_*): every array of the destination image, the
records (ev, dir, obs_src), graph_delta and the counts BIT-EXACT against the sequential restatement (tests/lc_fuse_ref.py) on the
shared cases (tests/lc_fuse_cases.py); on one map of 200 000 landmarks; chained with the local map's calls; and the refusals."""
import numpy as np
import pytest

import lc_fuse_cases as CS
import local_map_ref as LR
from plslam_amd import lc_fuse as LF
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


def _same_out(got, rec, want):
    assert np.array_equal(got["graph_delta"], want["graph_delta"])
    assert np.array_equal(rec["graph_delta"], want["graph_delta"])          # (the copy that stays on the device)
    for kind in ("points", "lines"):
        assert got[kind] == want[kind]["counts"], (kind, got[kind], want[kind]["counts"])
        assert np.array_equal(rec[kind]["ev"], want[kind]["ev"]), kind
        assert np.array_equal(_bits(rec[kind]["dir"]), _bits(want[kind]["dir"])), kind
        assert np.array_equal(rec[kind]["obs_src"], want[kind]["obs_src"]), kind


def _blank(dst):
    for kind in ("points", "lines"):
        for f in _FIELDS:
            if f != "feat_ptr":
                assert (dst.raw(f"{kind}.{f}") == BLANK).all(), (kind, f)
    assert dst.struct.points.n == 0 and dst.struct.lines.n_obs == 0


def _run(ctx, name, handle=None):
    m, lc, (m2, out), _ = CS.run_ref(name)
    lf = handle or LF.LcFuse(ctx)
    src = MI.DeviceMapImage(m, device=ctx.device)
    dst = MI.DeviceMapImage(m, **LF.fuse_bounds(m, lc), device=ctx.device, blank=BLANK)
    got = lf.run(src, dst, lc)
    _same_out(got, lf.download(), out)
    _same_image(dst, m2)
    _same_image(src, m)                                          # the source is read, not written
    if handle is None:
        lf.close()
    return out


@pytest.mark.parametrize("name", sorted(n for n in CS.CASES if n != "level_over"))
def test_cases_equal_the_restatement(ctx, name):
    out = _run(ctx, name)
    if name.startswith("tile_events"):
        n = CS.T + int(name.rsplit("_", 1)[1])
        assert out["points"]["counts"]["n_a"] == out["lines"]["counts"]["n_c"] == n
    if name.startswith("tile_landmarks"):
        m2 = CS.run_ref(name)[2][0]
        assert m2["points"]["n"] == m2["lines"]["n"] == CS.T + int(name.rsplit("_", 1)[1])
    if name == "no_events":
        assert not out["graph_delta"].any() and out["points"]["ev"].shape == (0, 6)


def test_a_smaller_case_after_a_larger_one_on_one_handle(ctx):
    """the handle's buffer is carved anew by every run: a case, then one without any tuple (every slice sized by the tuples
    shrinks to its slack, everything behind moves), then the first again, each equal to the restatement"""
    lf = LF.LcFuse(ctx)
    for name in ("three_entries", "no_events", "three_entries"):
        _run(ctx, name, lf)
    lf.close()


def test_the_tile_the_cases_are_built_around_is_the_kernels():
    import os
    import re
    import local_map_cases
    import map_insert_cases
    src = open(os.path.join(os.path.dirname(os.path.abspath(LF.__file__)), "csrc", "map_image.hpp")).read()
    tile = int(re.search(r"constexpr int MAP_TILE = (\d+);", src).group(1))
    assert tile == LM.LOOKBACK_TILE == MI.LOOKBACK_TILE == LF.LOOKBACK_TILE == CS.T == map_insert_cases.T == local_map_cases.T
    hdr = open(os.path.join(os.path.dirname(os.path.abspath(LF.__file__)), "..", "include", "plslam_hip.h")).read()
    assert int(re.search(r"#define PLSLAM_LC_FUSE_MAX_LEVEL (\d+)", hdr).group(1)) == LF.MAX_LEVEL == CS.L
    assert int(re.search(r"#define PLSLAM_LC_FUSE_MAX_TUPLES (\d+)", hdr).group(1)) == LF.MAX_TUPLES


def test_two_hundred_thousand_landmarks(ctx):
    """the many-tile path: the obs_ptr scan crosses 785 tiles, the resolve's lanes own 5 events each; 60 tuples name a landmark an earlier
    entry named (level 2; the few that hit one named twice already have level 3)"""
    out = _run(ctx, "big")
    assert out["points"]["counts"] == dict(n_a=1200, n_b=1200, n_c=900, n_d=1200, n_new=900, n_dead=1200, n_skipped=0)
    m, lc = CS.run_ref("big")[:2]
    assert m["points"]["n"] == 200_000 and np.diff(lc["points"]["entry_ptr"]).tolist() == [1500] * 3
    assert np.diff(lc["lines"]["entry_ptr"]).tolist() == [200] * 3 and 50 <= CS.run_ref("big")[3]["level.2"] <= 60


def test_chain_with_the_local_map(ctx):
    """the loop closure's order on the device: fuse -> plslam_local_map_form / _candidates / _gather on the destination, with
    full_graph's last row plus the delta's; every step equals the same chain of restatements"""
    m, lc, (m2, out), _ = CS.run_ref("three_entries")
    nk = m["n_map_kf"]
    p = dict(anchor=nk - 1, min_cov=75, window=3)
    lf, lm = LF.LcFuse(ctx), LM.LocalMap(ctx)
    dst = MI.DeviceMapImage(m, **LF.fuse_bounds(m, lc), device=ctx.device, blank=BLANK)
    got = lf.run(LM.DeviceMapIndex(m, ctx.device), dst, lc)
    assert np.array_equal(got["graph_delta"], out["graph_delta"])
    row = m["row"] + got["graph_delta"][nk - 1]
    m2 = dict(m2, row=row)
    counts = lm.form(dst, p["anchor"], row, p["min_cov"], p["window"])
    lm.candidates(dst, int(lc["lc_idx"][0][1]))
    counts.update(lm.gather(dst))
    kf_l, pt_l, ls_l = LR.form(m2, p["anchor"], p["min_cov"], p["window"])
    c = lm.download("pt_candidate", "ls_candidate")
    assert np.array_equal(c["pt_candidate"], LR.candidates(m2, "points", pt_l, int(lc["lc_idx"][0][1])))
    assert np.array_equal(c["ls_candidate"], LR.candidates(m2, "lines", ls_l, int(lc["lc_idx"][0][1])))
    ref = LR.gather(m2, kf_l, pt_l, ls_l)
    g = lm.download()
    assert counts["n_pt_obs"] == len(ref["pt_obs"]) > 100 and counts["n_ls_obs"] == len(ref["ls_obs"]) > 20
    for k in ("kf_list", "pt_list", "ls_list", "pt_obs", "ls_obs", "pt_obs_uv", "ls_l_obs", "X_aux"):
        assert np.array_equal(_bits(g[k]), _bits(ref[k])), k
    new = np.arange(m["points"]["n"], m2["points"]["n"])
    assert new.size == 60 and np.isin(new, ref["pt_list"]).any()  # landmarks the fusion made are in the problem
    lf.close()
    lm.close()


def test_refusals_leave_the_destination_untouched(ctx):
    m, lc, _, _ = CS.run_ref("three_entries")
    need = LF.fuse_bounds(m, lc)
    lf = LF.LcFuse(ctx)
    src = LM.DeviceMapIndex(m, ctx.device)
    for short in sorted(need):                                    # each capacity one below its bound: ERANGE
        dst = MI.DeviceMapImage(m, **dict(need, **{short: need[short] - 1}), device=ctx.device, blank=BLANK)
        with pytest.raises(PlslamError) as e:
            lf.run(src, dst, lc)
        assert e.value.code == -5, short
        _blank(dst)
    dst = MI.DeviceMapImage(m, **need, device=ctx.device, blank=BLANK)
    nk = m["n_map_kf"]
    for row in ([3, 3, 1], [-1, 30, 1], [3, nk, 1], [nk, 30, 1]):  # kf_prev == kf_curr, bad slots: EINVAL
        bad = dict(lc, lc_idx=np.array([row, lc["lc_idx"][1], lc["lc_idx"][2]], np.int32))
        with pytest.raises(PlslamError) as e:
            lf.run(src, dst, bad)
        assert e.value.code == -1, row
    with pytest.raises(PlslamError) as e:                         # the destination is the source
        lf.run(dst, dst, lc)
    assert e.value.code == -1
    L = ctx._L
    assert L.plslam_lc_fuse_run(None, None, None, 1, None, None, None, None, None, None) == -1
    assert L.plslam_lc_fuse_run(lf._h, None, None, 0, None, None, None, None, None, None) == -1
    assert L.plslam_lc_fuse_device_buffers(lf._h, None) == -1
    over = dict(lc, points=dict(lc["points"], entry_ptr=np.array([0, 0, 0, LF.MAX_TUPLES + 1], np.int32)))
    with pytest.raises(PlslamError) as e:                         # more tuples than the documented limit
        lf.run(src, dst, over)
    assert e.value.code == -5
    _blank(dst)
    # a level above the limit: refused on the device, by the status word, with nothing of the destination written
    m_o, lc_o, after, _ = CS.run_ref("level_over")
    assert after is None
    dst_o = MI.DeviceMapImage(m_o, **LF.fuse_bounds(m_o, lc_o), device=ctx.device, blank=BLANK)
    with pytest.raises(PlslamError) as e:
        lf.run(LM.DeviceMapIndex(m_o, ctx.device), dst_o, lc_o)
    assert e.value.code == -5
    _blank(dst_o)
    got = lf.run(src, dst, lc, graph=False)                       # and the handle still works; the graph may stay on the device
    assert got["points"]["n_d"] == 60 and got["graph_delta"] is None
    assert np.array_equal(lf.download()["graph_delta"], CS.run_ref("three_entries")[2][1]["graph_delta"])
    lf.close()
