"""CPU tests of the loop-closure fusion's restatement (tests/lc_fuse_ref.py), of the seeded generators and of the shared cases
(tests/lc_fuse_cases.py): the quirks the restatement keeps are pinned in the reference's source; every case takes the branches it
exists for; what the restatement leaves stays within the bounds the call states and is a consistent image; the level rule refuses
exactly one step past the limit; and the pure host half of the call (plslam_amd/csrc/lc_fuse_plan.hpp) runs clean under the
sanitizers in a stand-alone program."""
import os
import subprocess

import numpy as np
import pytest

import lc_fuse_cases as CS
import lc_fuse_ref as R
from plslam_amd import lc_fuse as LF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_SRC = "/root/reference/src/mapHandler.cpp"
ALL = sorted(CS.CASES)


def test_the_text_the_restatement_rests_on():
    if not os.path.exists(REF_SRC):
        pytest.skip("the reference source is not on this machine")
    src = open(REF_SRC).read()
    a = src.index("void MapHandler::loopClosureFuseLandmarks()")
    body = src[a:src.index("\n}\n", a)]
    pts, lns = body[:body.index("// line segment matches")], body[body.index("// line segment matches"):]
    for part, mp in ((pts, "map_points"), (lns, "map_lines")):
        assert "if( lc_idx_list[lc_idx](2) == 1 )" in part
        # A: against kf_curr, after the observation went in; B: against kf_prev
        a_, b_ = part.index("if( lm_idx0 == -1 && lm_idx1 != -1 )"), part.index("if( lm_idx0 != -1 && lm_idx1 == -1 )")
        c_, d_ = part.index("if( lm_idx0 == -1 && lm_idx1 == -1 )"), part.index("if( lm_idx0 != -1 && lm_idx1 != -1 )")
        assert a_ < b_ < c_ < d_
        first, second, fourth = part[a_:b_], part[b_:c_], part[d_:]
        assert "full_graph[(*kf_it)][kf_curr_idx]++;" in first and "full_graph[kf_curr_idx][(*kf_it)]++;" in first
        assert "kf_prev_idx]++" not in first
        assert "full_graph[(*kf_it)][kf_prev_idx]++;" in second and "kf_curr_idx]++" not in second
        assert first.index("Observation(") < first.index(f"for( auto kf_it = {mp}[lm_idx1]->kf_obs_list.begin()")
        # D: the length before, every pair, the first observer, and no guard on an empty list or on a == b
        assert f"int Nobs_lm_prev = {mp}[lm_idx0]->kf_obs_list.size();" in fourth
        assert "full_graph[idx][jdx]++;" in fourth and "full_graph[jdx][idx]++;" in fourth
        assert f"int kf_lm_obs = {mp}[lm_idx1]->kf_obs_list[0];" in fourth
        assert f"{mp}[lm_idx1] = nullptr;" in fourth and "lm_idx0 != lm_idx1" not in fourth and "empty()" not in fourth
        assert f"{mp}[lm_idx0] != NULL && {mp}[lm_idx1] != NULL" in fourth
    assert "stereo_pt[lm_ldx0]->P / map_keyframes[kf_prev_idx]->stereo_frame->stereo_pt[lm_ldx0]->P.norm();" in pts
    assert "Vector3d dir = P3d / P3d.norm();" in pts and "Vector3d dir = mP3d / mP3d.norm();" in lns
    assert "Vector3d mP3d = 0.5 * ( sP3d + eP3d );" in lns
    # the pts quirk that never reaches the call (line 4626 of the file)
    quirk = "pts.tail(2) = map_keyframes[kf_prev_idx]->stereo_frame->stereo_ls[lm_ldx1]->epl;"
    assert src.split("\n")[4625].strip() == quirk and lns.count(quirk) == 1


@pytest.mark.parametrize("name", sorted(CS.REACHES))
def test_cases_take_their_branches(name):
    hits = CS.run_ref(name)[3]
    missing = [b for b in CS.REACHES[name] if hits[b] < 3]
    assert not missing, (missing, dict(hits))


def test_the_cases_take_every_branch_between_them():
    seen = set()
    for name in ALL:
        h = CS.run_ref(name)[3]
        assert set(h) <= set(R.BRANCHES)
        seen |= {b for b in h if h[b] >= 3}
    assert not [b for b in R.BRANCHES if b not in seen]


def _lists(K):
    p = K["obs_ptr"]
    return [K["obs_kf"][p[i]:p[i + 1]].tolist() for i in range(K["n"])]


@pytest.mark.parametrize("name", [n for n in ALL if n != "level_over"])
def test_invariants_and_bounds(name):
    m, lc, (m2, out), _ = CS.run_ref(name)
    need = LF.fuse_bounds(m, lc)
    g = out["graph_delta"].astype(np.int64)
    assert np.array_equal(g, g.T) and (g >= 0).all()
    pairs = 0
    for kind, tag in (("points", "pt"), ("lines", "ls")):
        A, B, o, c = m[kind], m2[kind], out[kind], out[kind]["counts"]
        ev = o["ev"]
        assert B["n"] == A["n"] + c["n_new"] <= need[tag + "_cap"] and B["obs_kf"].size <= need[tag + "_obs_cap"]
        assert B["n"] == B["valid"].size == B["inlier"].size == B["X"].shape[0] == B["obs_ptr"].size - 1
        assert B["obs_ptr"][0] == 0 and (np.diff(B["obs_ptr"]) >= 0).all() and B["obs_ptr"][-1] == B["obs_kf"].size
        # a fusion moves observations: every source observation is somewhere exactly once, every made one too
        src = o["obs_src"]
        assert np.array_equal(np.sort(src[src >= 0]), np.arange(A["obs_kf"].size))
        made = -1 - src[src < 0]
        assert made.size == np.unique(made).size == c["n_a"] + c["n_b"] + 2 * c["n_c"]
        assert np.array_equal(B["obs_kf"][src >= 0], A["obs_kf"][src[src >= 0]])
        assert np.array_equal(B["obs_val"][src >= 0], A["obs_val"][src[src >= 0]])
        # the records
        codes = [int((ev[:, 0] == k).sum()) for k in range(1, 5)]
        assert codes == [c["n_a"], c["n_b"], c["n_c"], c["n_d"]] and c["n_new"] == c["n_c"] and c["n_dead"] == c["n_d"]
        assert np.array_equal(ev[ev[:, 0] == 3, 1], A["n"] + np.arange(c["n_new"]))
        dead = ev[ev[:, 0] == 4, 2]
        assert np.unique(dead).size == dead.size and not B["valid"][dead].any() and (np.diff(B["obs_ptr"])[dead] == 0).all()
        assert (np.diff(B["obs_ptr"])[A["n"]:] == 2).all() and B["valid"][A["n"]:].all()
        acted = ev[ev[:, 0] > 0]
        assert (acted[:, 4] >= 0).all() and (acted[:, 4] + acted[:, 5] <= B["obs_kf"].size).all()
        d = ev[ev[:, 0] == 4]
        assert np.array_equal(B["obs_kf"][d[:, 4]], d[:, 3])      # the anchor is the first moved observation's keyframe
        assert not o["dir"][ev[:, 0] == 0].any() and not o["dir"][ev[:, 0] == 4].any()
        assert not o["dir"][ev[:, 0] == 1][:, 3:].any() and not o["dir"][ev[:, 0] == 2][:, :3].any()
        unit = np.concatenate([o["dir"][ev[:, 0] == 1][:, :3], o["dir"][ev[:, 0] == 2][:, 3:], o["dir"][ev[:, 0] == 3][:, :3],
                               o["dir"][ev[:, 0] == 3][:, 3:]])
        assert np.allclose(np.linalg.norm(unit, axis=1), 1.0, atol=1e-12)
        pairs += c["n_c"]
    # every increment goes to [i][j] and [j][i]: an even total, and at least the new landmarks' one pair each (the values
    # themselves rest on the restatement's own loops: it is the definition the device is held to)
    assert g.sum() % 2 == 0 and g.sum() >= 2 * pairs


def test_the_level_rule():
    assert CS.run_ref("level_limit")[2] is not None and CS.run_ref("level_over")[2] is None
    m, lc = CS.CASES["level_over"]()
    m2, out = R.fuse(m, lc, max_level=R.MAX_LEVEL + 1)            # one more level allowed: the same input goes through
    assert out["points"]["counts"]["n_a"] + out["points"]["counts"]["n_b"] == 2 * (R.MAX_LEVEL + 1)
    assert R.MAX_LEVEL == LF.MAX_LEVEL == CS.L


def test_state_carries_from_event_to_event():
    m, lc, (m2, out), _ = CS.run_ref("nested")
    P, ev = m2["points"], out["points"]["ev"]
    t = lc["points"]["tuples"]
    a, b, c = int(t[2, 0]), int(t[2, 2]), int(t[1, 2])          # the first set: (a, b) fused by tuple 2, c appended to by tuple 1
    la, lb, lc_ = (_lists(m["points"])[x] for x in (a, b, c))
    got = _lists(P)[c]
    assert not _lists(P)[a] and not _lists(P)[b] and not P["valid"][a] and not P["valid"][b] and P["valid"][c]
    kp, kc, kp2, kc2 = 3, 30, 5, 33
    assert got == lc_ + [kp] + [kc2] + la + lb + [kp] + [kc] + [kp2]
    src = out["points"]["obs_src"][P["obs_ptr"][c]:P["obs_ptr"][c + 1]]
    assert (np.diff(-1 - src[src < 0]) < 0).any()                 # the order of the list is not the order of the events
    # two writers of one feature: the later event's landmark stays
    m, lc, (m2, out), _ = CS.run_ref("same_feature")
    t, A, B = lc["points"]["tuples"], m["points"], m2["points"]
    assert t[0, 1] == t[1, 1] and B["feat_idx"][A["feat_ptr"][3] + t[1, 1]] == t[1, 2] != t[0, 2]
    assert t[2, 3] == t[3, 3] and B["feat_idx"][A["feat_ptr"][30] + t[3, 3]] == t[3, 0] != t[2, 0]


def test_generators_are_seeded():
    a, b = CS.CASES["mixed"](), CS.CASES["mixed"]()
    assert np.array_equal(a[1]["points"]["tuples"], b[1]["points"]["tuples"]) and np.array_equal(a[1]["T_kf_w"], b[1]["T_kf_w"])
    c = LF.synthetic_loop_closure(CS.base_map(), CS.ENTRIES[:1], CS._PT, CS._LS, seed=4)
    d = LF.synthetic_loop_closure(CS.base_map(), CS.ENTRIES[:1], CS._PT, CS._LS, seed=5)
    assert not np.array_equal(c["points"]["P0"], d["points"]["P0"])
    assert c["points"]["tuples"].shape == (100, 4) and c["lines"]["tuples"].shape == (30, 4) and c["lines"]["P0"].shape == (30, 6)
    need = LF.fuse_bounds(CS.base_map(), c)
    assert need["pt_cap"] == 600 + 20 and need["pt_obs_cap"] == CS.base_map()["points"]["obs_kf"].size + 60 + 40
    off = dict(c, lc_idx=np.array([[3, 30, 0]], np.int32))
    assert LF.fuse_bounds(CS.base_map(), off)["pt_cap"] == 600   # an entry already optimised asks for nothing


def test_the_host_half_under_the_sanitizers(tmp_path):
    """tests/cpp/test_lc_fuse_pack.cpp: validation, bounds, packing and the device layout (lc_fuse_plan.hpp) in a stand-alone program
    built with -fsanitize=address,undefined"""
    exe = str(tmp_path / "test_lc_fuse_pack")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra",
                        "-Werror", os.path.join(ROOT, "tests", "cpp", "test_lc_fuse_pack.cpp"), "-I" + os.path.join(ROOT, "include"),
                        "-I" + os.path.join(ROOT, "plslam_amd", "csrc"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "lc_fuse_pack: ok" in r.stdout and "lc_fuse_layout: ok" in r.stdout, (r.stdout[-2000:], r.stderr[-3000:])
