"""GPU tests of the vocabulary training (plslam_bow_train_*, bow_train.hip) against the restatement of
TemplatedVocabulary::create with the counter draws (tests/bow_train_ref.py, pinned to the reference's own create by
tests/test_bow_train_cpu.py).  Every comparison is exact: records, weights as uint64, statistics, the partition and the words.

The design has no limit on the nodes of a level per launch (the kernels run over positions, nodes and (node, cluster) pairs in
grids sized by them), so there is no case for one."""
import numpy as np
import pytest

from plslam_amd import bow, bow_train
from plslam_amd.capi import EINVAL, ENOTSUP, PlslamError
from tests import bow_train_ref as T
from tests import dbow_ref as R

pytestmark = pytest.mark.gpu

SIZES = ["1", "2", "k", "k+1", "63", "64", "65", "257", "1025", "3000"]


def _split(rng, desc, kind):
    """documents over the rows of desc: "mixed" has an empty first document, a single-row one and an empty last one"""
    n = desc.shape[0]
    if kind == "one":
        return [desc]
    cuts = np.sort(rng.integers(0, n + 1, 3)) if n > 1 else np.array([0, 1, 1])
    cuts = np.concatenate([[0, 0, min(1, n)], np.maximum(cuts, min(1, n)), [n, n]])
    return [desc[a:b] for a, b in zip(cuts[:-1], cuts[1:])]


def _expect(docs, k, L, weighting, seed, max_iters=1000):
    """the restatement; TF and BINARY differ from IDF in the leaves' weights alone"""
    return T.train(docs, k, L, weighting, T.CounterDraws(seed), max_iters)


def _train(ctx, docs, k, L, weighting, seed, max_iters=1000):
    parts = [np.asarray(d, np.uint8).reshape(-1, 32) for d in docs]
    t = bow_train.BowTrainer(ctx, np.concatenate(parts), bow_train.doc_offsets(parts), k, L, weighting, seed, max_iters)
    stats = t.run()
    voc = t.export()
    leaf, word = t.download()
    t.close()
    return voc, stats, leaf, word


def _assert_same(got, exp, what=""):
    voc, stats, leaf, word = got
    for f in ("node_id", "parent_id", "descriptor"):
        assert np.array_equal(voc.nodes[f], exp["nodes"][f]), f"{what}: nodes.{f}"
    assert np.array_equal(voc.nodes["weight"].view(np.uint64), exp["nodes"]["weight"].view(np.uint64)), f"{what}: weights"
    for f in ("word_id", "node_id"):
        assert np.array_equal(voc.words[f], exp["words"][f]), f"{what}: words.{f}"
    s = exp["stats"]
    assert (stats["n_nodes"], stats["n_words"], stats["lloyd_rounds"], stats["lloyd_rounds_max"], stats["empty_groups"],
            stats["capped_nodes"]) == (s["nodes"], s["words"], s["rounds_total"], s["rounds_max"], s["empty_groups"],
                                       s["capped_nodes"]), f"{what}: stats {stats} != {s}"
    assert np.array_equal(leaf, exp["leaf"]), f"{what}: the training partition"
    assert np.array_equal(word, exp["word"]), f"{what}: the words of the descent"


@pytest.mark.parametrize("k", [2, 3, 10])
@pytest.mark.parametrize("size", SIZES)
def test_training_equals_the_restatement_in_every_bit(ctx, size, k):
    """N in {1, 2, k, k + 1, 63, 64, 65, 257, 1025, 3000} x k in {2, 3, 10} x L in {1, 2, 4}; the four weightings go round over
    the cases, a weighted and an unweighted one on every tree; documents with an empty, a single-row and an all-in-one split."""
    n = {"k": k, "k+1": k + 1}.get(size) or int(size)
    si = SIZES.index(size)
    rng = np.random.default_rng(1000 + 10 * si + k)
    desc = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    for li, L in enumerate((1, 2, 4)):
        docs = _split(rng, desc, "one" if (si + li) % 3 == 0 else "mixed")
        seed = int(rng.integers(0, 2 ** 63))
        for weighting in ((R.TF_IDF, R.BINARY) if (si + li + k) % 2 else (R.IDF, R.TF)):
            exp = _expect(docs, k, L, weighting, seed)
            _assert_same(_train(ctx, docs, k, L, weighting, seed), exp, f"N={n} k={k} L={L} w={weighting}")


CLUSTERED = [(33, 4, 3), (32, 5, 3), (32, 3, 4)]         # (rng seed, k, L): the restatement reports empty groups on each


@pytest.mark.parametrize("case", CLUSTERED)
def test_clustered_inputs_with_empty_groups(ctx, case):
    """prototypes with a few flipped bits: groups run empty (the input on which the reference itself crashes); the device reports
    the restatement's count and builds its tree"""
    rs, k, L = case
    rng = np.random.default_rng(rs)
    docs = T.clustered_docs(rng, 4, 150, 6, 15)
    exp = _expect(docs, k, L, R.TF_IDF, 17 + rs)
    assert exp["stats"]["empty_groups"] > 0
    _assert_same(_train(ctx, docs, k, L, R.TF_IDF, 17 + rs), exp)


def test_inputs_that_are_all_duplicates(ctx):
    """one descriptor 300 times, and three descriptors 100 times each under k = 5: the seeding stops early with fewer than k
    clusters, and the trivial case meets duplicates (where the descent and the training partition differ)"""
    rng = np.random.default_rng(5)
    three = rng.integers(0, 256, (3, 32), dtype=np.uint8)
    for desc in (np.repeat(three[:1], 300, axis=0), np.tile(three, (100, 1)), np.tile(three, (1, 1)).repeat(2, axis=0)):
        docs = [desc[: len(desc) // 3], desc[len(desc) // 3:]]
        for weighting in (R.IDF, R.TF):
            _assert_same(_train(ctx, docs, 5, 3, weighting, 99), _expect(docs, 5, 3, weighting, 99))


@pytest.mark.parametrize("max_iters", [1, 2])
def test_round_cap_leaves_capped_nodes(ctx, max_iters):
    rng = np.random.default_rng(60 + max_iters)
    docs = [rng.integers(0, 256, (n, 32), dtype=np.uint8) for n in (400, 300, 333)]
    exp = _expect(docs, 4, 3, R.TF_IDF, 3, max_iters)
    assert exp["stats"]["capped_nodes"] > 0 and exp["stats"]["rounds_max"] == max_iters
    _assert_same(_train(ctx, docs, 4, 3, R.TF_IDF, 3, max_iters), exp)


def test_a_node_straddles_a_tile_and_a_wave_boundary_between_two_neighbours(ctx):
    """N = 3000, k = 3, L = 2: the second level's middle node holds position 2048 (the scan's and the distribution's tile, a
    workgroup and a wave boundary) and has a node on either side"""
    rng = np.random.default_rng(77)
    docs = [rng.integers(0, 256, (3000, 32), dtype=np.uint8)]
    exp = _expect(docs, 3, 2, R.IDF, 3)
    top = exp["nodes"]["parent_id"][exp["leaf"] - 1]               # L = 2: every leaf hangs off a child of the root
    sizes = [int((top == c).sum()) for c in sorted(set(top.tolist()))]
    assert len(sizes) == 3 and sizes[0] < 2048 < sizes[0] + sizes[1]
    _assert_same(_train(ctx, docs, 3, 2, R.IDF, 3), exp)


def test_the_same_call_twice_gives_identical_bytes(ctx):
    rng = np.random.default_rng(81)
    docs = T.uniform_docs(rng)
    a, b = (_train(ctx, docs, 10, 4, R.TF_IDF, 12345) for _ in range(2))
    assert a[0].nodes.tobytes() == b[0].nodes.tobytes() and a[0].words.tobytes() == b[0].words.tobytes()
    assert a[1] == b[1] and a[2].tobytes() == b[2].tobytes() and a[3].tobytes() == b[3].tobytes()


def test_the_trained_vocabulary_transforms_as_the_restatement_of_dbow2(ctx, tmp_path):
    """train_vocabulary -> save / load -> BowVocabulary: fuzz sets transform exactly as tests/dbow_ref.py does on the records"""
    rng = np.random.default_rng(90)
    voc, stats = bow_train.train_vocabulary(ctx, T.uniform_docs(rng), 6, 3, R.TF_IDF, seed=4)
    assert stats["n_nodes"] == voc.nodes.shape[0] and stats["n_words"] == voc.words.shape[0]
    path = str(tmp_path / "trained.yml.gz")
    bow.save_vocabulary(path, voc)
    back = bow.load_vocabulary(path)
    assert back.nodes.tobytes() == voc.nodes.tobytes() and back.words.tobytes() == voc.words.tobytes()
    gv, rv = bow.BowVocabulary(ctx, voc), R.Vocab(voc)
    sets = [np.concatenate([bow.near_leaf_descriptors(rng, voc, n // 2), rng.integers(0, 256, (n - n // 2, 32), dtype=np.uint8)])
            for n in (1, 5, 64, 65, 300)]
    off = bow_train.doc_offsets(sets)
    word, weight, bword, bweight, blen = gv.transform(np.concatenate(sets), off)
    for s, feats in enumerate(sets):
        v, per = rv.transform(feats)
        a, b = off[s], off[s + 1]
        assert [p[0] for p in per] == word[a:b].tolist()
        assert np.array_equal(np.array([p[1] for p in per]).view(np.uint64), weight[a:b].view(np.uint64))
        items = R.sorted_items(v)
        assert blen[s] == len(items) and bword[a:a + blen[s]].tolist() == [w for w, _ in items]
        assert np.array_equal(np.array([x for _, x in items]).view(np.uint64), bweight[a:a + blen[s]].view(np.uint64))
    gv.close()


def test_create_refusals_leave_no_handle(ctx):
    d = np.zeros((4, 32), np.uint8)
    for kw, code in ((dict(k=1, L=2), EINVAL), (dict(k=2, L=0), EINVAL), (dict(k=2, L=2, scoring=1), ENOTSUP),
                     (dict(k=2, L=2, weighting=4), EINVAL)):
        with pytest.raises(PlslamError) as e:
            bow_train.BowTrainer(ctx, d, [0, 4], **kw)
        assert e.value.code == code
    with pytest.raises(PlslamError) as e:
        bow_train.BowTrainer(ctx, d[:0], [0, 0, 0], 2, 2)
    assert e.value.code == EINVAL


def test_the_device_pointer_form_trains_where_the_descriptors_lie(ctx):
    """plslam_bow_train_create_dev over a caller's device block: the same export as the host form, and the block is untouched"""
    import torch
    rng = np.random.default_rng(95)
    docs = T.uniform_docs(rng)
    docs.insert(1, docs[0][:0])
    desc, off = np.concatenate(docs), bow_train.doc_offsets(docs)
    dd, doff = torch.from_numpy(desc).to("cuda"), torch.from_numpy(off).to("cuda")
    torch.cuda.synchronize()
    t = bow_train.BowTrainer(ctx, dd.data_ptr(), doff.data_ptr(), 7, 3, R.IDF, 31, dev=True, n_docs=len(docs), n_total=desc.shape[0])
    stats = t.run()
    got = (t.export(), stats) + t.download()
    t.close()
    _assert_same(got, _expect(docs, 7, 3, R.IDF, 31))
    assert np.array_equal(dd.cpu().numpy(), desc)
