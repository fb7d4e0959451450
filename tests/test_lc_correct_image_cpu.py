"""The loop-closure correction on the map image, without a GPU: the invariant that lets it do without anchor lists (the reference's
map_*_kf_idx containers, replayed from the records of the image calls by the reference's own push / erase rules, always equal the
lists derived from the image), the numpy restatement of the image rule against the anchor-list restatement, its vectorised form against
the loop, the reach of the maps the GPU tests run at scale, and the host half of the call under the sanitizers."""
import copy
import os
import subprocess

import numpy as np
import pytest

import lc_correct_image_cases as CS
import lc_correct_image_ref as R
import lc_fuse_ref as FR
import local_map_ref as LR
import map_insert_ref as IR
import pgo_ref
from plslam_amd import lc_fuse as LF
from plslam_amd import local_map as LM
from plslam_amd import map_insert as MI

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _assert_lists(lists, m, step):
    for kind in R.KINDS:
        ptr, idx = LM.anchor_lists(m, kind)
        assert lists[kind] == R.lists_of(ptr, idx), (step, kind)


def _with_observations(m):
    """the landmarks an event may name: the reference has no landmark without an observation, and one that received its first
    observation from an event would be anchored nowhere in the reference's lists"""
    return {kind: ((m[kind]["valid"] == 1) & (np.diff(m[kind]["obs_ptr"]) > 0)).astype(np.uint8) for kind in R.KINDS}


def test_the_replayed_containers_equal_the_lists_of_the_image():
    m = LM.synthetic_map()
    lists = {kind: R.lists_of(*LM.anchor_lists(m, kind)) for kind in R.KINDS}
    n_new = n_culled = 0
    for step in range(4):
        m_kf, kf = MI.synthetic_keyframe(m, 96, 32, seed=20 + step, points=dict(n_new=14, n_exist=14, n_invalid=3, n_out_of_range=2, n_same_lm=2),
                                         lines=dict(n_new=6, n_exist=5, n_invalid=2))
        for kind in R.KINDS:
            lists[kind].append([])                                # the new slot kf2
        _assert_lists(lists, m_kf, (step, "slot"))
        m_a, out = IR.insert_kf2kf(m_kf, kf)
        for kind in R.KINDS:
            R.replay_insert(lists[kind], kf, out[kind])
            n_new += out[kind]["counts"]["n_new"]
        _assert_lists(lists, m_a, (step, "kf2kf"))
        kf_b = MI.synthetic_map2kf(m_a, kf, seed=30 + step, points=dict(n_events=8, n_same_i2=2, n_invalid=2), lines=dict(n_events=3),
                                   candidates=_with_observations(m_a))
        m_b, out = IR.insert_map2kf(m_a, kf_b)
        assert out["points"]["counts"]["n_events"] >= 8           # (a map <-> keyframe insert creates no landmark: nothing to replay)
        _assert_lists(lists, m_b, (step, "map2kf"))
        nk = m_b["n_map_kf"]
        _, pt_l, ls_l = LR.form(m_b, nk - 1, 75, 3)
        before = copy.deepcopy(m_b)
        removed = LR.cull(m_b, pt_l, ls_l, nk + 4, 3)
        for kind, rem in zip(R.KINDS, removed):
            R.replay_cull(lists[kind], before[kind], rem)
            n_culled += int(rem.sum())
        _assert_lists(lists, m_b, (step, "cull"))
        m = m_b
    assert n_new >= 60 and n_culled >= 20, (n_new, n_culled)
    mix_pt, mix_ls = dict(n_a=12, n_b=12, n_c=9, n_d=9, n_invalid=2, n_self=1), dict(n_a=4, n_b=4, n_c=4, n_d=4)
    lc = LF.synthetic_loop_closure(m, entries=((3, 30, 1), (5, 41, 1)), points=mix_pt, lines=mix_ls, seed=5)
    m_f, out = FR.fuse(m, lc)
    for kind in R.KINDS:
        c = out[kind]["counts"]
        assert min(c["n_a"], c["n_b"], c["n_c"], c["n_d"]) >= 4, (kind, c)         # events of all four branches
        lists[kind] = copy.deepcopy(lists[kind])
        R.replay_fuse(lists[kind], out[kind])
    _assert_lists(lists, m_f, "fuse")


def _edge_map():
    """NULL keyframe slots, invalid landmarks, landmarks with empty lists, a first observer of -1 and of n_map_kf"""
    m = LM.synthetic_map(n_kf=12, n_pt=300, n_ls=70, seed=31, null_kf=(2, 7), null_lm_frac=0.1, no_obs_frac=0.1)
    for kind in R.KINDS:
        K = m[kind]
        has = np.flatnonzero((K["valid"] == 1) & (np.diff(K["obs_ptr"]) > 1))
        K["obs_kf"] = K["obs_kf"].copy()
        K["obs_kf"][K["obs_ptr"][has[0]]] = -1
        K["obs_kf"][K["obs_ptr"][has[1]]] = m["n_map_kf"]
        K["obs_kf"][K["obs_ptr"][has[2]] + 1] = -1                # (a later observer out of range changes nothing)
    return m


def _inputs(m, seed, p_corrected=0.6):
    rng = np.random.Generator(np.random.PCG64(seed))
    nk = m["n_map_kf"]
    T_corr = np.stack([MI._pose(rng) for _ in range(nk)])
    corrected = rng.random(nk) < p_corrected
    dirs = {kind: rng.standard_normal((m[kind]["obs_kf"].size, 3)) for kind in R.KINDS}
    med = {kind: rng.standard_normal((m[kind]["n"], 3)) for kind in R.KINDS}
    return T_corr, corrected, dirs, med


def test_the_image_rule_equals_the_anchor_list_restatement_bit_for_bit():
    for m, seed in ((_edge_map(), 1), (LM.synthetic_map(null_kf=(0, 13, 39)), 2)):
        nk = m["n_map_kf"]
        T_corr, corrected, dirs, med = _inputs(m, seed)
        assert corrected.any() and not corrected.all()
        for kind in R.KINDS:
            K = m[kind]
            ptr, idx = LM.anchor_lists(m, kind)
            assert idx.size < int((K["valid"] == 1).sum())        # some valid landmark is anchored nowhere
            X, md, dd = pgo_ref.correct_landmarks(T_corr, corrected, ptr, idx, K["valid"], K["X"], med[kind], K["obs_ptr"], dirs[kind],
                                                  line=kind == "lines")
            got = R.correct_kind(K, nk, T_corr, corrected, dirs[kind], med[kind])
            assert np.array_equal(_bits(got["X"]), _bits(X)) and not np.array_equal(X, K["X"]), kind
            assert np.array_equal(_bits(got["med_dir"]), _bits(md)) and np.array_equal(_bits(got["dirs"]), _bits(dd)), kind
            slot = R.anchor_slots(K, nk, corrected)
            assert got["n"] == int(corrected[np.repeat(np.arange(nk), np.diff(ptr))].sum()) == int((slot >= 0).sum())
            assert got["n_dirs"] == int(np.diff(K["obs_ptr"])[slot >= 0].sum())


def test_anchor_lists_leave_out_what_the_image_rule_leaves_out():
    m = _edge_map()
    nk = m["n_map_kf"]
    for kind in R.KINDS:
        K = m[kind]
        ptr, idx = LM.anchor_lists(m, kind)
        assert ptr.dtype == idx.dtype == np.int32 and ptr.shape == (nk + 1,) and ptr[0] == 0 and ptr[-1] == idx.size
        first = np.array([K["obs_kf"][K["obs_ptr"][j]] if K["obs_ptr"][j + 1] > K["obs_ptr"][j] else -9 for j in range(K["n"])])
        for k in range(nk):
            want = [j for j in range(K["n"]) if K["valid"][j] and first[j] == k]
            assert idx[ptr[k]:ptr[k + 1]].tolist() == want, (kind, k)
        assert (first == -1).any() and (first == nk).any() and (first == -9).any() and (K["valid"] == 0).any()
        assert ptr[3] > ptr[2] and ptr[8] > ptr[7]                # a NULL keyframe slot still anchors what it first observed


# ---- the vectorised restatement is the loop ----------------------------------------------------------------------------------------
def _same_restatement(m, T_corr, corrected, x_new, lists, med, what):
    want = R.correct_image(m, T_corr, corrected, x_new, lists, med)
    got = R.correct_image_fast(m, T_corr, corrected, x_new, lists, med)
    assert got["counts"] == want["counts"], (what, got["counts"], want["counts"])
    assert np.array_equal(_bits(got["x_kf_w"]), _bits(want["x_kf_w"])), (what, "x_kf_w")
    for kind in R.KINDS:
        for f in ("X", "dirs", "med_dir"):
            g, w = got[kind][f], want[kind][f]
            assert (g is None) == (w is None), (what, kind, f)
            assert g is None or (g.shape == w.shape and np.array_equal(_bits(g), _bits(w))), (what, kind, f)
    return want["counts"]


def _fast_cases():
    yield "decision map", CS.decision_map(), ([1, 1, 1, 1], [1, 0, 0, 0], [0, 0, 0, 1], [0, 0, 0, 0])
    for nk in (1, 2):
        for lines_too in (True, False):
            yield f"length map {nk} {lines_too}", CS.length_map(nk, lines_too), ([1] * nk, [1] + [0] * (nk - 1), [0] * (nk - 1) + [1])
    for n in (0, 1, CS.T - 1, CS.T, CS.T + 1):                    # test_landmark_counts_at_the_tile_edges
        yield f"tile edge {n}", LM.synthetic_map(n_kf=6, n_pt=n, n_ls=n, seed=300 + n, no_obs_frac=0.1), ([1, 0, 1, 1, 0, 1],)
    yield "edge map", _edge_map(), (None,)
    yield "inside map", CS.inside_map(), ([1, 1, 1], [1, 0, 0], [0, 0, 1])
    for ends_empty in (False, True):
        yield f"depth map {ends_empty}", CS.depth_map(CS.T + 1, ends_empty), ([1, 1, 1, 1, 1], [1, 0, 1, 0, 1])


def test_the_vectorised_restatement_equals_the_loop_bit_for_bit():
    moved = 0
    for what, m, patterns in _fast_cases():
        T_corr, lists, med, x_new = CS.inputs(m, 70)
        for co in patterns:
            co = np.random.Generator(np.random.PCG64(71)).random(m["n_map_kf"]) < 0.6 if co is None else np.asarray(co, bool)
            moved += _same_restatement(m, T_corr, co, x_new, lists, med, (what, co.tolist()))["n_pt_dirs"]
    assert moved > 5000
    m = LM.synthetic_map()                                        # ... with and without the arrays that need not be carried
    T_corr, lists, med, x_new = CS.inputs(m, 72)
    co = np.arange(m["n_map_kf"]) % 3 > 0
    for with_dir in (True, False):
        for with_med in (True, False):
            for with_x in (True, False):
                c = _same_restatement(m, T_corr, co, x_new if with_x else None, lists if with_dir else None, med if with_med else None,
                                      ("synthetic_map", with_dir, with_med, with_x))
                assert c["n_pt"] > 300 and (c["n_pt_dirs"] > c["n_pt"]) == with_dir


def test_the_vectorised_restatement_refuses_what_it_is_not_defined_for():
    m = CS.length_map(2)
    T_corr, lists, med, x_new = CS.inputs(m, 73)
    for j, by in ((5, -70), (0, 1)):                              # obs_ptr descends; obs_ptr does not start at 0
        mb = dict(m, points=dict(m["points"], obs_ptr=m["points"]["obs_ptr"].copy()))
        mb["points"]["obs_ptr"][j] += by
        with pytest.raises(AssertionError, match="obs_ptr must start at 0 and never descend"):
            R.correct_image_fast(mb, T_corr, [1, 1], x_new, lists, med)


# ---- the maps of test_gpu_lc_correct_image_scale.py reach what they are named for -------------------------------------------------
def test_the_constants_the_cases_are_built_around():
    assert CS.T == LM.LOOKBACK_TILE and CS.G >= 2 and CS.DEPTH_SIZES == (255, 256, 257, 65535, 65536, 65537)
    assert [len(CS.search_rounds(n, 0)[0]) for n in CS.DEPTH_SIZES] == list(CS.DEPTH_ROUNDS) == [1, 1, 2, 2, 2, 3]
    assert CS.search_rounds(CS.T * CS.T + 1, CS.T * CS.T) == ([(0, 65537, 257), (65535, 2, 1)], True)


@pytest.mark.parametrize("ends_empty", [False, True])
@pytest.mark.parametrize("n", CS.DEPTH_SIZES)
def test_the_depth_maps_reach_their_rounds(n, ends_empty):
    m = CS.depth_map(n, ends_empty)
    CS.depth_reach(m, n)
    lens = np.diff(m["points"]["obs_ptr"])
    assert (lens[0] == 0) == (lens[-1] == 0) == ends_empty and set(lens[2:-2].tolist()) == {0, 1, 2, 3}


def test_the_inside_map_has_tiles_inside_one_list():
    assert CS.inside_reach(CS.inside_map()) == 12


def test_the_walk_map_has_more_tiles_than_workgroups():
    m = CS.walk_map()
    assert CS.walk_reach(m) == (CS.G + 5, 2 * CS.G + 874)
    nk = m["n_map_kf"]
    assert [int(CS.walk_corrected(p, nk)[[CS.WALK_A, CS.WALK_B, CS.WALK_C]] @ [1, 2, 4]) for p in CS.WALK_PATTERNS] == [7, 5, 2, 6, 0]


def test_the_host_half_under_the_sanitizers(tmp_path):
    """tests/cpp/test_lc_image_plan.cpp: the argument checks and the packing (lc_image_plan.hpp) in a stand-alone program built with
    -fsanitize=address,undefined"""
    exe = str(tmp_path / "test_lc_image_plan")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra",
                        "-Werror", os.path.join(ROOT, "tests", "cpp", "test_lc_image_plan.cpp"), "-I" + os.path.join(ROOT, "include"),
                        "-I" + os.path.join(ROOT, "plslam_amd", "csrc"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "lc_image_plan: ok" in r.stdout, (r.stdout[-2000:], r.stderr[-3000:])
