"""CPU tests of the device-resident global bundle adjustment's host pieces: the numpy restatement of the GBA gather
(tests/gba_dev_ref.py, from src/mapHandler.cpp:1995-2092) against the LBA gather's restatement with every flag set, and
plslam_amd.gba.map_image's round trip on every input the device tests use."""
import numpy as np
import pytest

from plslam_amd import gba
from plslam_amd.local_map import synthetic_map

import gba_dev_cases as DC
import gba_dev_ref as R
import local_map_ref

SYNTHETIC = {
    "mixed": dict(n_kf=40, n_pt=600, n_ls=150, seed=1, null_kf=(3, 17, 39)),
    "null_slot_0": dict(n_kf=25, n_pt=300, n_ls=80, seed=2, null_kf=(0, 11)),
    "dense_tracks": dict(n_kf=6, n_pt=200, n_ls=60, seed=3, max_obs=9, null_kf=(2,)),
    "no_lines": dict(n_kf=12, n_pt=150, n_ls=0, seed=4),
}


@pytest.mark.parametrize("name", list(SYNTHETIC))
def test_the_gba_gather_is_the_lba_gather_with_every_flag_set(name):
    m = synthetic_map(**SYNTHETIC[name])
    P, L = m["points"], m["lines"]
    got = R.gba_gather(m)
    ref = local_map_ref.gather(m, m["kf_valid"].copy(), P["valid"].copy(), L["valid"].copy())
    for k in R.GATHER_KEYS:
        assert R.same_bits(got[k], ref[k]), (name, k)
    # the maps contain what the comparison is for
    if name != "no_lines":
        assert (m["kf_valid"] == 0).any() and (P["valid"] == 0).any() and (L["valid"] == 0).any()
        assert (np.diff(P["obs_ptr"])[P["valid"] != 0] == 0).any(), "a listed landmark without observations"
        assert (got["pt_obs"][:, 4] == -1).any() and (got["pt_obs"][:, 4] >= 0).any()
    if name == "dense_tracks":
        o = got["pt_obs"]
        twice = (o[1:, 1] == o[:-1, 1]) & (o[1:, 3] == o[:-1, 3])      # (list order: ascending keyframes per landmark)
        assert twice.any(), "a landmark seen twice by one keyframe"
    assert 0 not in got["kf_list"] and (np.diff(got["kf_list"]) > 0).all()


def _round_trip(m):
    g = R.gba_gather(gba.map_image(m))
    nkf = len(m["kf_list"])
    assert R.same_bits(g["kf_list"], np.asarray(m["kf_list"], np.int32))
    assert R.same_bits(g["pt_obs"], m["pt_obs"]) and R.same_bits(g["ls_obs"], m["ls_obs"])
    assert R.same_bits(g["pt_obs_uv"], m["pt_uv"]) and R.same_bits(g["ls_l_obs"], m["ls_l"])
    assert R.same_bits(g["pt_list"], np.arange(m["npt"], dtype=np.int32)) and R.same_bits(g["ls_list"], np.arange(m["nls"], dtype=np.int32))
    assert R.same_bits(g["X_aux"], np.concatenate([m["x_kf"].ravel(), m["Xw"].ravel(), m["Lw"].ravel()]))
    assert g["X_aux"].size == 6 * nkf + 3 * m["npt"] + 6 * m["nls"]


@pytest.mark.parametrize("name", list(DC.MAPS))
def test_map_image_round_trip(name):
    m = DC.MAPS[name]()
    _round_trip(m)
    # the cases are what their names say
    if name == "twice":
        for obs, which in ((m["pt_obs"], DC.TWICE_POINTS), (m["ls_obs"], DC.TWICE_LINES)):
            for j in which:
                kf = obs[obs[:, 1] == j, 3]
                assert len(set(kf.tolist())) < kf.size
    if name == "nkf1":
        assert len(m["kf_list"]) == 1
    if name == "points_only":
        assert m["nls"] == 0 and m["ls_obs"].shape[0] == 0 and m["npt"] > 0
    if name == "lines_only":
        assert m["npt"] == 0 and m["pt_obs"].shape[0] == 0 and m["nls"] > 0
    if name == "gaps":
        assert (gba.map_image(m)["kf_valid"] == 0).sum() > 0 and (m["pt_obs"][:, 4] == -1).any()
    if name == "no_point_obs":
        assert m["npt"] > 0 and m["pt_obs"].shape[0] == 0


# COLUMNS: random rows that no gather makes.  The two smallest happen to satisfy map_image's precondition (no row / one row) and
# round-trip; every other one is refused by it -- its rows are not grouped by landmark -- and is uploaded as columns instead.
COLUMNS_THAT_ARE_A_GATHER = ("both_0", "both_1")


@pytest.mark.parametrize("name", list(DC.COLUMNS))
def test_which_column_cases_are_a_gather(name):
    m = DC.COLUMNS[name]()
    if name in COLUMNS_THAT_ARE_A_GATHER:
        m = dict(m, npt=m["npt"], nls=m["nls"])
        _round_trip(m)
    else:
        assert (np.diff(m["pt_obs"][:, 1]) < 0).any(), "rows not grouped by landmark"
        with pytest.raises(AssertionError, match="grouped by ascending landmark"):
            gba.map_image(m)
    n = int(name.split("_")[1])
    if name.startswith("both_"):
        assert m["pt_obs"].shape[0] == n and m["ls_obs"].shape[0] == n
        if n >= 3 * DC.T:
            # the pair enumeration spans at least three look-back tiles: observations by optimised keyframes, both kinds
            assert int((m["pt_obs"][:, 4] >= 0).sum() + (m["ls_obs"][:, 4] >= 0).sum()) > 3 * DC.LOOKBACK
    else:
        assert len(m["kf_list"]) == n


def test_map_image_refuses_what_is_not_a_gather():
    m = DC.MAPS["nkf16"]()
    bad = dict(m, pt_obs=m["pt_obs"].copy())
    bad["pt_obs"][5, 2] += 1
    with pytest.raises(AssertionError, match="column 2"):
        gba.map_image(bad)
    bad = dict(m, pt_obs=m["pt_obs"].copy())
    bad["pt_obs"][5, 4] = -1 if bad["pt_obs"][5, 4] >= 0 else 0
    with pytest.raises(AssertionError, match="column 4"):
        gba.map_image(bad)
    with pytest.raises(AssertionError, match="kf_list"):
        gba.map_image(dict(m, kf_list=m["kf_list"][::-1]))


def test_ragged_blocks_fill_more_than_one_tile_of_the_block_compaction():
    assert len(gba.covisible_blocks(DC.MAPS["ragged"]())) > 3 * DC.LOOKBACK
