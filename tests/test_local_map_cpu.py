"""CPU tests of the local-map restatement (tests/local_map_ref.py), of the seeded generator and of the shared cases: the
restatement is checked on maps whose answers are written out here; the text it rests on is pinned in the reference's source;
every case of tests/local_map_cases.py reaches the branches it is named for."""
import collections
import os
import re

import numpy as np
import pytest

import local_map_cases as CS
import local_map_ref as R
from plslam_amd import local_map as LM

REF_SRC = "/root/reference/src/mapHandler.cpp"


def _small():
    """5 keyframes, slot 2 NULL.  Points 0..5; point 4 is NULL but still named by a feature of keyframe 4."""
    pts = [(1, 1, [0, 1]), (1, 1, [1, 3]), (1, 1, [3, 4]), (1, 1, [0]), (0, 1, [4]), (1, 1, [])]
    return CS.hand_map([1, 1, 0, 1, 1], [80, 10, 99, 10, 0], points=pts, lines=[(1, 1, [1, 4]), (1, 1, [0, 3])],
                       pt_feats={0: [0, 3, -1], 1: [1, 0], 3: [2, LM.FEAT_NULL, 1], 4: [LM.FEAT_NULL, 4, 2, -1]},
                       ls_feats={0: [1], 1: [0], 3: [1, -1], 4: [0]})


def test_form_by_hand_both_overloads():
    m = _small()
    # formLocalMap(): anchor 4; row[0] = 80 >= 75 -> keyframe 0; the NULL slot 2 (row 99) is skipped; window 0
    kf, pt, ls = R.form(m, 4, 75, 0)
    assert kf.tolist() == [1, 0, 0, 0, 1]
    assert pt.tolist() == [1, 0, 1, 1, 0, 0]          # keyframe 4 names 4 (NULL: not set) and 2; keyframe 0 names 0 and 3
    assert ls.tolist() == [1, 1]
    # window 1: keyframe 3 (|4 - 1 - ...|: g_size - i = 1) joins, with points 2 and 1
    kf, pt, ls = R.form(m, 4, 75, 1)
    assert kf.tolist() == [1, 0, 0, 1, 1] and pt.tolist() == [1, 1, 1, 1, 0, 0]
    # formLocalMap(kf): anchor 1, and the graph loop STILL reads the last row: keyframe 0 by row[0], not keyframe 4
    kf, pt, ls = R.form(m, 1, 75, 0)
    assert kf.tolist() == [1, 1, 0, 0, 0] and pt.tolist() == [1, 1, 0, 1, 0, 0] and ls.tolist() == [1, 1]


def test_candidates_by_hand():
    m = _small()
    kf, pt, ls = R.form(m, 4, 75, 1)
    # local points 0 1 2 3; last observers 1 3 4 0; point 5 has none
    assert R.candidates(m, "points", pt, 4).tolist() == [1, 1, 0, 1, 0, 0]
    assert R.candidates(m, "points", pt, 3).tolist() == [1, 0, 1, 1, 0, 0]
    assert R.candidates(m, "lines", ls, 4).tolist() == [0, 1]


def test_gather_by_hand():
    m = _small()
    kf, pt, ls = R.form(m, 4, 75, 1)                    # local keyframes 0 3 4, points 0 1 2 3, lines 0 1
    g = R.gather(m, kf, pt, ls)
    assert g["kf_list"].tolist() == [3, 4]              # slot 0 is local but excluded (:1231)
    assert g["pt_list"].tolist() == [0, 1, 2, 3] and g["ls_list"].tolist() == [0, 1]
    assert g["pt_obs"].tolist() == [[0, 0, 0, 0, -1, 1], [0, 0, 1, 1, -1, 1], [1, 1, 0, 1, -1, 1], [1, 1, 1, 3, 0, 1],
                                    [2, 2, 0, 3, 0, 1], [2, 2, 1, 4, 1, 1], [3, 3, 0, 0, -1, 1]]
    assert g["ls_obs"].tolist() == [[0, 0, 0, 1, -1, 1], [0, 0, 1, 4, 1, 1], [1, 1, 0, 0, -1, 1], [1, 1, 1, 3, 0, 1]]
    P, L = m["points"], m["lines"]
    assert np.array_equal(g["pt_obs_uv"], P["obs_val"][:7]) and np.array_equal(g["ls_l_obs"], L["obs_val"])
    want = np.concatenate([m["x_kf_w"][3], m["x_kf_w"][4], P["X"][:4].ravel(), L["X"].ravel()])
    assert np.array_equal(g["X_aux"], want) and not g["empty"]
    # nothing local but the anchor, which has no landmark left: the reference's return -1
    e = CS.hand_map([1, 1], [0, 0], points=[(1, 1, [0])], pt_feats={0: [0]})
    assert R.gather(e, *R.form(e, 1, 75, 0))["empty"]


def test_cull_by_hand():
    m, p = CS.cull_edges()
    out, after = CS.run_ref(m, p)
    assert out["pt_local"].sum() == 0 and out["kf_local"].tolist() == [0] * 13 + [1]
    assert out["pt_removed"].tolist() == [1, 1, 0, 1, 0, 1, 0] and out["ls_removed"].tolist() == [1]
    assert after["points"]["valid"].tolist() == [0, 0, 1, 0, 1, 0, 1]
    # keyframe 2: [3, NULL, 0, -1, 0, 6] -> point 3's and the FIRST of point 0's two features go, the duplicate stays
    assert after["points"]["feat_idx"].tolist() == [-1, LM.FEAT_NULL, -1, -1, 0, 6, 2, 6, 0, 6, 1]
    assert after["lines"]["feat_idx"].tolist() == [-1, -1, 0, 0]
    # one keyframe later point 2 is 11 behind as well
    out2, _ = CS.run_ref(m, dict(p, max_kf_idx=14))
    assert out2["pt_removed"].tolist() == [1, 1, 1, 1, 0, 1, 0]


def test_generator_is_seeded():
    a, b, c = LM.synthetic_map(seed=5, null_kf=(3,)), LM.synthetic_map(seed=5, null_kf=(3,)), LM.synthetic_map(seed=6, null_kf=(3,))

    def flat(m):
        return [m[k] for k in ("kf_valid", "x_kf_w", "row")] + [m[kind][k] for kind in ("points", "lines") for k in sorted(m[kind])]
    assert all(np.array_equal(x, y) for x, y in zip(flat(a), flat(b)))
    assert not all(np.array_equal(x, y) for x, y in zip(flat(a), flat(c)))
    P = a["points"]
    assert P["obs_ptr"][-1] == P["obs_kf"].size == P["obs_val"].shape[0] and P["feat_ptr"][-1] == P["feat_idx"].size
    assert (P["feat_idx"] == LM.FEAT_NULL).any() and (P["feat_idx"] == -1).any() and (P["valid"] == 0).any()
    assert P["feat_ptr"][4] == P["feat_ptr"][3]         # the NULL slot has no features, but landmarks still list it
    assert (P["obs_kf"] == 3).any() and (np.diff(P["obs_ptr"]) == 0).any()


def _ref_text(name, nth=0):
    if not os.path.exists(REF_SRC):
        pytest.skip("the reference source is not on this machine")
    src = open(REF_SRC).read()
    a = [x.start() for x in re.finditer(re.escape(name), src)][nth]
    return src[a:src.index("\n}\n", a)]


def test_the_text_the_restatement_rests_on():
    plain, overload = _ref_text("void MapHandler::formLocalMap()"), _ref_text("void MapHandler::formLocalMap( KeyFrame * kf )")
    for body in (plain, overload):
        # the graph loop reads the LAST row in both overloads, and dereferences slot and features without a NULL check
        assert "int g_size = full_graph.size()-1;" in body
        assert "if( full_graph[g_size][i] >= SlamConfig::minLMCovGraph() || abs(g_size-i) <= SlamConfig::minKFLocalMap() )" in body
        loop = body[body.index("for( int i = 0; i < g_size; i++ )"):]
        assert "map_keyframes[i]->local = true;" in loop and "NULL" not in loop.replace("map_points[lm_idx] != NULL", "").replace("map_lines[lm_idx] != NULL", "")
        assert "int lm_idx = (*pt_it)->idx;\n                if( lm_idx != -1 && map_points[lm_idx] != NULL )" in loop
        # ... while the anchor's features are checked
        head = body[:body.index("int g_size")]
        assert head.count("if( (*pt_it) != NULL )") == 2 and head.count("if( (*ls_it) != NULL )") == 2
    assert "map_keyframes.back()->local = true;" in plain and "kf->local = true;" in overload
    lba = _ref_text("int MapHandler::localBundleAdjustment()")
    assert "if( (*kf_it)->local && (*kf_it)->kf_idx != 0 )" in lba
    assert "obs_aux(4) = -1;" in lba and "obs_aux(5) = 1;" in lba and "if( kf_list[j] == kf_obs_list_ )" in lba
    assert "if( pt_obs_list.size() + ls_obs_list.size() != 0 )" in lba and "return -1;" in lba
    cull = _ref_text("void MapHandler::removeBadMapLandmarks()")
    assert "if( (*pt_it)->local == false && max_kf_idx - (*pt_it)->kf_obs_list[0] > 10 )" in cull
    assert "if( (*ls_it)->local == false && max_kf_idx-(*ls_it)->kf_obs_list[0] > 10 )" in cull
    assert "if( (*pt_it)->inlier == false || (*pt_it)->obs_list.size() < SlamConfig::minLMObs() )" in cull
    assert re.search(r"if\( \(\*st_pt\)->idx == lm_idx \)\s*\{\s*\(\*st_pt\)->idx = -1;\s*break;", cull)
    assert re.search(r"if\( \(\*st_ls\)->idx == lm_idx \)\s*\{\s*\(\*st_ls\)->idx = -1;\s*break;", cull)
    m2kf = _ref_text("int MapHandler::matchMap2KFPoints()")
    assert "if (pt != nullptr && pt->local && pt->kf_obs_list.back() != kf2_idx) {" in m2kf


def _hits(name):
    m, p = CS.CASES[name]()
    h = collections.Counter()
    CS.run_ref(m, p, h)
    return h


@pytest.mark.parametrize("name", sorted(CS.REACHES))
def test_cases_reach_their_branches(name):
    h = _hits(name)
    missing = [b for b in CS.REACHES[name] if not h[b]]
    assert not missing, (missing, dict(h))


def test_the_cases_reach_every_branch_between_them():
    h = collections.Counter()
    for name in CS.CASES:
        h.update(_hits(name))
    assert set(h) <= set(R.BRANCHES) | {"cull.feat_none"}
    assert not [b for b in R.BRANCHES if not h[b]]
    # with every keyframe local no keyframe is left out: the case is not a copy of the mixed ones
    a = _hits("all_local")
    assert not a["gather.kf_not_local"] and not a["form.graph_neither"]
