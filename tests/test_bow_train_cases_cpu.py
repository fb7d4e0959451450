"""The cases of tests/bow_train_cases.py do what they are named for, from the restatement (tests/bow_train_ref.py) alone: a case
that silently missed its branch would leave tests/test_gpu_bow_train_edges.py passing for nothing.  Also here: the vectorised
descent the restatement now uses (descend_all) against the per-row one that is pinned to the compiled reference (descend), on
every row of every input of tests/test_bow_train_cpu.py (taken from the builders that file uses, tests/bow_train_ref.py) and of
every new case -- the rows of the two cases of 70000 and 2^20 rows in four consecutive parts, a test each --, and the inverse
of the draw function's mixer.  No GPU."""
import os
import re

import numpy as np
import pytest

from tests import bow_train_cases as C
from tests import bow_train_ref as T

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bow_train_golden.npz")


# ---- the draw function inverted ----------------------------------------------------------------------------------------------
def test_unmix_inverts_the_mixer():
    rng = np.random.default_rng(3)
    for x in [0, 1, 2 ** 64 - 1, 2 ** 63, 0x9E3779B97F4A7C15, 7128774783429081126] + [int(v) for v in
                                                                                     rng.integers(0, 2 ** 64, 50, dtype=np.uint64)]:
        assert C.unmix(T.mix64(x)) == x and T.mix64(C.unmix(x)) == x, x


def test_seed_for_hits_its_draw():
    assert C.seed_for(1, 0, 0) == 7128774783429081126
    for j, t, r in list(C.DRAW_SEEDS.values()) + [(0, 0, 12345), (255, 0, 1), (7, 3, C.R_MAX), (1, 1, 0)]:
        for low in (0x1234567, 0, 2 ** 33 - 1):
            seed = C.seed_for(j, t, r, low)
            assert 0 <= seed < 2 ** 64 and T.counter_draw(T.root_key(seed), j, t) == r, (j, t, r, low)
    assert sum(C.seed_for(*a) >= 2 ** 63 for a in C.DRAW_SEEDS.values()) >= 2       # seeds beyond int64 reach the binding


# ---- the vectorised descent ------------------------------------------------------------------------------------------------
def _same_descent(res, docs, rows=None):
    desc = np.concatenate([np.asarray(d, np.uint8).reshape(-1, 32) for d in docs])
    if rows is not None:
        desc = desc[rows]
    fast = T.descend_all(res["children"], res["ndesc"], desc)
    slow = np.array([T.descend(res["children"], res["ndesc"], f) for f in desc], np.int64)
    assert np.array_equal(fast, slow)
    return fast


@pytest.mark.parametrize("weighting", T.WEIGHTINGS)
def test_descend_all_is_descend_on_the_live_inputs_pinned_to_the_reference(weighting):
    """the 36 uniform and 12 heavy-duplicate inputs of tests/test_bow_train_cpu.py, with the C library's draws, by its own rule
    (the first seed of eight without an empty group or a capped node)"""
    n = 0
    for make, seed0, kl in ((T.uniform_docs, T.uniform_seed0, [(k, L) for k in T.UNIFORM_K for L in T.UNIFORM_L]),
                            (T.duplicate_docs, T.duplicate_seed0, T.DUPLICATE_KL)):
        for k, L in kl:
            docs, _, mine = T.clean_input(make, k, L, weighting, seed0(k, L, weighting))
            _same_descent(mine, docs)
            n += 1
    assert n == 9 + 3


def test_descend_all_is_descend_on_the_recorded_and_the_departure_inputs():
    """the recorded reference inputs, the clustered input on which groups run empty, the uniform input capped at 1 and 2 rounds"""
    g = np.load(GOLDEN)
    for name in g["cases"].tolist():
        k, L, weighting, seed = (int(x) for x in g[f"{name}__params"])
        off = g[f"{name}__off"]
        docs = [g[f"{name}__desc"][a:b] for a, b in zip(off[:-1], off[1:])]
        _same_descent(T.train(docs, k, L, weighting, T.LibcDraws(seed)), docs)
    rs, k, L, weighting, seed = T.DEPARTURE_CLUSTERED
    docs = T.clustered_docs(np.random.default_rng(rs), 4, 150, 6, 15)
    res = T.train(docs, k, L, weighting, T.CounterDraws(seed))
    assert res["stats"]["empty_groups"] > 0
    _same_descent(res, docs)
    rs, k, L, weighting, seed, caps = T.DEPARTURE_CAPPED
    docs = T.uniform_docs(np.random.default_rng(rs))
    for cap in caps:
        res = T.train(docs, k, L, weighting, T.CounterDraws(seed), cap)
        assert res["stats"]["capped_nodes"] > 0
        _same_descent(res, docs)


SCALE_PARTS = 4
WALKS = [(name, p) for name in C.CASES for p in range(SCALE_PARTS if name.startswith("scale_") else 1)]


@pytest.mark.parametrize("name,part", WALKS, ids=[n + (f"-part{p}" if n.startswith("scale_") else "") for n, p in WALKS])
def test_descend_all_is_descend_on_the_new_cases(name, part):
    """every row; the two scale cases in SCALE_PARTS consecutive parts that together are all their rows"""
    docs = C.case(name)[0]
    res = C.expect(name)[0]
    n = res["leaf"].shape[0]
    rows = None
    if name.startswith("scale_"):
        cuts = [n * i // SCALE_PARTS for i in range(SCALE_PARTS + 1)]
        assert cuts[0] == 0 and cuts[-1] == n
        rows = np.arange(cuts[part], cuts[part + 1])
    node = _same_descent(res, docs, rows)
    word_of = np.full(res["nodes"].shape[0] + 1, -1, np.int64)
    word_of[res["words"]["node_id"]] = res["words"]["word_id"]
    assert np.array_equal(word_of[node], res["word"] if rows is None else res["word"][rows])


def test_descend_all_refuses_children_that_are_not_consecutive():
    nd = [np.zeros(32, np.uint8)] * 4
    with pytest.raises(AssertionError):
        T.descend_all([[1, 3], [], [], []], nd, np.zeros((2, 32), np.uint8))
    assert T.descend_all([[1, 2, 3], [], [], []], nd, np.zeros((2, 32), np.uint8)).tolist() == [1, 1]     # the first minimum


# ---- each case reaches its branch -------------------------------------------------------------------------------------------
def _root_children(exp):
    return int((exp["nodes"]["parent_id"] == 0).sum())


def test_level_profile_on_a_tree_small_enough_to_count_by_hand():
    """6 rows, k = 2, L = 2, a tree written down here: root -> nodes 1 (rows 0, 2, 3, 5) and 2 (rows 1, 4); node 1 -> leaves 3
    (rows 0, 5) and 4 (rows 2, 3); node 2 has two rows, k = 2: trivial, leaves 5 and 6"""
    nodes = np.zeros(6, T.NODE_DTYPE)
    nodes["node_id"], nodes["parent_id"] = np.arange(1, 7), [0, 0, 1, 1, 2, 2]
    exp = dict(nodes=nodes, leaf=np.array([3, 5, 4, 4, 6, 3]))
    assert C.level_profile(exp, 2) == [(1, 1, 2), (2, 1, 4)]


@pytest.mark.parametrize("name", C.GROUPS["deep"])
def test_deep_cases_fill_a_second_tile_and_a_second_workgroup_of_nodes(name):
    docs, k, L, _, _, _ = C.case(name)
    exp = C.expect(name)[0]
    prof = C.level_profile(exp, k)
    assert len(docs) == 40 and exp["stats"]["capped_nodes"] == 0
    assert max(g for _, _, g in prof) >= 10                        # a wave with ten and more (node, cluster) groups
    assert any(0 < run < vis for vis, run, _ in prof)              # running and trivial nodes on one level
    if name.startswith("deep_k2_L13"):
        assert len(prof) == 13
        assert any(vis > 1024 and run > 256 for vis, run, _ in prof), prof
    elif name.startswith("deep_k2_L16"):
        assert L == 16 and len(prof) == 15, prof                   # the tree ends before L
        assert max(run for _, run, _ in prof) > 256
    else:
        assert len(prof) == 8 and max(vis for vis, _, _ in prof) > 256


@pytest.mark.parametrize("name", C.GROUPS["wide"])
def test_wide_cases_seed_k_clusters_on_the_root(name):
    docs, k, L, _, _, _ = C.case(name)
    exp = C.expect(name)[0]
    prof = C.level_profile(exp, k)
    assert k in (64, 65, 256) and L == 2 and _root_children(exp) == k
    assert prof[0][:2] == (1, 1) and prof[0][2] > 32
    if k == 256:
        assert len(prof) == 2 and prof[1][0] > 0 and prof[1][1] == 0           # every node of level 2 is trivial


@pytest.mark.parametrize("name", C.GROUPS["far_tied"])
def test_far_and_tied_cases(name):
    exp = C.expect(name)[0]
    fig = C.figures(name)
    if name.startswith("alternating_k"):
        assert fig["root_max_min_d"] == 256
        assert (exp["stats"]["nodes"], exp["stats"]["words"]) == (4, 2)        # seeding stops at one centre on level 2
        assert sorted(exp["nodes"]["descriptor"].sum(axis=1).tolist()) == [0, 0, 32 * 255, 32 * 255]
    elif name == "alternating_flipped":
        assert 252 <= fig["root_max_min_d"] <= 256 and exp["stats"]["nodes"] > 4
    else:
        assert 0 < fig["root_max_min_d"] <= 10                     # 8 + 2 bits ever differ
        assert fig["tied_rows"] > 0 and fig["half_majorities"] > 0


@pytest.mark.parametrize("name", C.GROUPS["draws"])
def test_draw_cases_reach_the_edges_of_the_draws(name):
    docs, k, L, _, seed, _ = C.case(name)
    exp, draws = C.expect(name)
    key0, n = T.root_key(seed), exp["leaf"].shape[0]
    retries = [(key, j, t) for key, j, t in draws.asked if t > 0]
    root_cuts = {j: (s, c) for key, j, s, c in draws.cuts if key == key0}
    assert draws.firsts[0][:2] == (key0, n) and sorted(root_cuts) == [1, 2]
    if name.startswith("draw_retry"):
        j = C.DRAW_SEEDS[name][0]
        assert retries == [(key0, j, 1)] and root_cuts[j][1] > 0.0
    else:
        assert retries == []
    if name == "draw_cut_is_the_sum":
        assert root_cuts[1][0] == root_cuts[1][1]
    if name == "draw_first_is_the_last_row":
        assert draws.firsts[0][2] == n - 1
    if name == "draw_first_is_row_0":
        assert draws.firsts[0][2] == 0


@pytest.mark.parametrize("name", C.GROUPS["documents"])
def test_document_cases(name):
    docs, k, L, weighting, _, _ = C.case(name)
    exp = C.expect(name)[0]
    n = exp["leaf"].shape[0]
    weights = np.unique(exp["nodes"]["weight"][exp["words"]["node_id"] - 1])
    assert weighting in (T.IDF, T.TF_IDF) and any(d.shape[0] == 0 for d in docs)
    if name.startswith("documents_499"):
        assert (len(docs), n) == (500, 3000) and weights.size >= 10
        empty = [d.shape[0] == 0 for d in docs]
        assert any(a and b for a, b in zip(empty, empty[1:]))      # a run of empty documents
    else:
        assert (len(docs), n) == (200, 40) and len(docs) > n and weights.size >= 2


def test_scale_cases():
    docs, k, L, _, _, max_iters = C.case("scale_words")
    exp = C.expect("scale_words")[0]
    assert (sum(d.shape[0] for d in docs), k, L, max_iters, len(docs)) == (70000, 64, 3, 1, 50)
    assert exp["stats"]["words"] >= 65536                          # a third radix pass of the word sort
    docs, k, L, _, _, max_iters = C.case("scale_tiles")
    n = sum(d.shape[0] for d in docs)
    assert (n, k, L, max_iters) == (2 ** 20 + 1500, 2, 1, 1) and [d.shape[0] == 0 for d in docs] == [False, True, False]
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "plslam_amd", "csrc",
                            "bow_train_plan.hpp")).read()
    tile, nt = (int(re.search(r"constexpr int %s = (\d+);" % c, hdr).group(1)) for c in ("BT_SCAN_TILE", "BT_SCAN_NT"))
    assert (tile, nt) == (1024, 1024)                              # K114's items per tile, K115's lanes: the planner's constants
    assert (n + tile - 1) // tile > nt                             # K115's carry loop over the tiles' totals takes a second trip
    assert C.expect("scale_tiles")[0]["stats"]["words"] == 2


def test_no_case_but_the_scale_cases_is_above_6000_rows():
    for name in C.CASES:
        if not name.startswith("scale_"):
            assert sum(d.shape[0] for d in C.case(name)[0]) <= 6000, name
    assert sorted(n for g in C.GROUPS.values() for n in g) == sorted(C.CASES)
