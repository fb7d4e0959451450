"""Restatement of DBoW2's vocabulary training, TemplatedVocabulary::create (3rdparty/DBoW2/include/DBoW2/TemplatedVocabulary.h
:536-976: HKmeansStep, initiateClustersKMpp, createWords, setNodeWeights) with FORB's distance and meanValue
(src/DBoW2/FORB.cpp:25-101).  Test infrastructure, never imported by the product.

It is `create` as written, with three stated departures ("Training a vocabulary"):
  1. the random numbers come from a draw source.  LibcDraws(seed) is the reference's own stream -- srand(seed), one rand() per
     draw, in the recursion's depth-first order -- and pins this module to the reference bit for bit (tests/test_bow_train_cpu.py).
     CounterDraws(seed) makes every draw a function of (seed, node path, centre index j, retry t): what the device computes
     (plslam_amd/csrc/bow_train_draw.h states the same function for the planner and the kernels).
  2. a group that is empty when the centres are recomputed keeps its centre (the reference releases it and then reads the empty
     matrix: undefined behaviour).  Counted in stats["empty_groups"].
  3. at most max_iters rounds per node; a node that hits the cap keeps its last centres and assignment.  Counted in
     stats["capped_nodes"].  A round is one pass of the reference's while(goon) loop, the seeding pass included.
"""
from __future__ import annotations

import ctypes
import math

import numpy as np

TF_IDF, TF, IDF, BINARY = 0, 1, 2, 3
_M64 = (1 << 64) - 1
_POP = np.array([bin(i).count("1") for i in range(256)], np.int64)

NODE_DTYPE = np.dtype([("node_id", np.int32), ("parent_id", np.int32), ("weight", np.float64), ("descriptor", np.uint8, 32)])
WORD_DTYPE = np.dtype([("word_id", np.int32), ("node_id", np.int32)])


def mix64(z: int) -> int:
    """the splitmix64 finaliser"""
    z &= _M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    return z ^ (z >> 31)


def root_key(seed: int) -> int:
    return mix64(seed)


def child_key(key: int, c: int) -> int:
    return mix64(key + c + 1)


def counter_draw(key: int, j: int, t: int) -> int:
    """the 31-bit draw of (node key, centre index j, retry t)"""
    return mix64(key + 0x9E3779B97F4A7C15 * ((j << 32) + t + 1)) >> 33


class Draws:
    """r(key, j, t) -> a 31-bit integer in place of rand(); the arithmetic on it is the reference's."""

    def r(self, key, j, t):
        raise NotImplementedError

    def first(self, key, n):
        """DUtils::Random::RandomInt(0, n - 1), Random.cpp:49"""
        return int((self.r(key, 0, 0) / 2147483648.0) * n)

    def cut(self, key, j, dist_sum):
        """DUtils::Random::RandomValue<double>(0, dist_sum), Random.h:57, drawn again while it is 0.0 (:868-871)"""
        t = 0
        while True:
            c = (self.r(key, j, t) / 2147483647.0) * dist_sum
            t += 1
            if c != 0.0:
                return c


class LibcDraws(Draws):
    """The C library's stream: srand(seed) now, rand() per draw whatever the node."""

    def __init__(self, seed):
        self._libc = ctypes.CDLL(None)
        self._libc.rand.restype = ctypes.c_int
        self._libc.srand(ctypes.c_uint(seed))

    def r(self, key, j, t):
        return self._libc.rand()


class CounterDraws(Draws):
    def __init__(self, seed):
        self.seed = seed

    def r(self, key, j, t):
        return counter_draw(key, j, t)


def _dist(rows, centre):
    """FORB::distance of every row to one centre"""
    return _POP[rows ^ centre].sum(axis=1)


def mean_value(rows):
    """FORB::meanValue: bit b set iff count_b >= n / 2 + n % 2; one descriptor is copied"""
    n = rows.shape[0]
    if n == 1:
        return rows[0].copy()
    cnt = np.unpackbits(rows, axis=1).astype(np.int64).sum(axis=0)
    return np.packbits(cnt >= n // 2 + n % 2)


def _seed_clusters(rows, k, draws, key):
    """initiateClustersKMpp, :812-893"""
    n = rows.shape[0]
    centres = [rows[draws.first(key, n)].copy()]
    min_d = _dist(rows, centres[0])
    while len(centres) < k:
        min_d = np.minimum(min_d, _dist(rows, centres[-1]))
        dist_sum = int(min_d.sum())
        if dist_sum <= 0:
            break
        cut_d = draws.cut(key, len(centres), float(dist_sum))
        up = np.cumsum(min_d).astype(np.float64)
        hit = np.flatnonzero(up >= cut_d)
        centres.append(rows[int(hit[0]) if hit.size else n - 1].copy())
    return centres


def _assign(rows, centres):
    d = np.stack([_dist(rows, c) for c in centres], axis=1)
    return np.argmin(d, axis=1)                                  # the first minimum: strict '<' over the clusters


class _Train:
    def __init__(self, desc, k, L, draws, max_iters):
        self.desc, self.k, self.L, self.draws, self.max_iters = desc, k, L, draws, max_iters
        self.parent = [0]
        self.ndesc = [np.zeros(32, np.uint8)]
        self.children = [[]]
        self.leaf = np.full(desc.shape[0], -1, np.int64)
        self.rounds_total = self.rounds_max = self.empty = self.capped = 0

    def step(self, parent_id, idx, level, key):
        """HKmeansStep, :620-797; idx: the node's descriptors in their original order"""
        if idx.size == 0:
            return
        rows = self.desc[idx]
        if idx.size <= self.k:
            centres = [r.copy() for r in rows]
            assoc = np.arange(idx.size)
        else:
            it, last = 0, None
            while True:
                it += 1
                if it == 1:
                    centres = _seed_clusters(rows, self.k, self.draws, key)
                else:
                    for c in range(len(centres)):
                        g = rows[last == c]
                        if g.shape[0] == 0:
                            self.empty += 1                      # departure 2: the centre stays
                        else:
                            centres[c] = mean_value(g)
                assoc = _assign(rows, centres)
                if it > 1 and np.array_equal(assoc, last):
                    break
                last = assoc
                if it >= self.max_iters:                         # departure 3
                    self.capped += 1
                    break
            self.rounds_total += it
            self.rounds_max = max(self.rounds_max, it)
        first = len(self.parent)
        for c in centres:
            self.children[parent_id].append(len(self.parent))
            self.parent.append(parent_id)
            self.ndesc.append(c)
            self.children.append([])
        for c in range(len(centres)):
            g = idx[assoc == c]
            if level < self.L and g.size > 1:
                self.step(first + c, g, level + 1, child_key(key, c))
            else:
                self.leaf[g] = first + c


def descend(children, ndesc, feature):
    """transform(feature, word_id), :1198-1240 -> the leaf's node id"""
    node = 0
    while children[node]:
        kids = children[node]
        d = _dist(np.stack([ndesc[c] for c in kids]), feature)
        node = kids[int(np.argmin(d))]
    return node


def descend_all(children, ndesc, desc):
    """descend() for every row of desc at once, level by level: the first minimum over a node's children by strict '<'.  The
    children of a node are consecutive ids (HKmeansStep makes them in one go), which is asserted."""
    first = np.array([c[0] if c else 0 for c in children], np.int64)
    count = np.array([len(c) for c in children], np.int64)
    for c, f in zip(children, first):
        assert c == list(range(int(f), int(f) + len(c))), "the children of a node are not consecutive ids"
    desc = np.ascontiguousarray(desc, np.uint8).reshape(-1, 32)
    q = desc.view(np.uint64)                                       # (N, 4)
    nd = np.ascontiguousarray(np.stack(ndesc), np.uint8).view(np.uint64)
    node = np.zeros(desc.shape[0], np.int64)
    live = np.flatnonzero(count[node] > 0)
    while live.size:
        at, m = first[node[live]], count[node[live]]
        best = at.copy()
        best_d = np.bitwise_count(q[live] ^ nd[at]).sum(axis=1, dtype=np.int64)
        for c in range(1, int(m.max())):
            has = np.flatnonzero(c < m)
            d = np.bitwise_count(q[live[has]] ^ nd[at[has] + c]).sum(axis=1, dtype=np.int64)
            less = d < best_d[has]
            best_d[has[less]] = d[less]
            best[has[less]] = at[has[less]] + c
        node[live] = best
        live = live[count[best] > 0]
    return node


def train(docs, k, L, weighting, draws, max_iters=1000):
    """create(training_features) for TemplatedVocabulary(k, L, weighting, L1_NORM).  docs: a list of (n_i, 32) uint8 arrays.
    Returns a dict: nodes (NODE_DTYPE, ascending node id, no root), words (WORD_DTYPE), stats, leaf (per descriptor: the node
    of the training partition), word (per descriptor: the word of the descent), children and ndesc (the tree that descend and
    descend_all walk)."""
    docs = [np.asarray(d, np.uint8).reshape(-1, 32) for d in docs]
    desc = np.concatenate(docs) if docs else np.zeros((0, 32), np.uint8)
    N = desc.shape[0]
    seed = getattr(draws, "seed", 0)
    T = _Train(desc, k, L, draws, max_iters)
    T.step(0, np.arange(N), 1, root_key(seed))
    nn = len(T.parent) - 1
    word_of = {}
    for nid in range(1, nn + 1):                                  # createWords, :898-918
        if not T.children[nid]:
            word_of[nid] = len(word_of)
    weight = np.zeros(nn + 1)
    word_at = np.full(nn + 1, -1, np.int64)
    word_at[list(word_of.keys())] = list(word_of.values())
    word = word_at[descend_all(T.children, T.ndesc, desc)] if N else np.zeros(0, np.int64)
    assert (word >= 0).all()
    if weighting in (TF, BINARY):                                 # setNodeWeights, :923-976
        for nid in word_of:
            weight[nid] = 1.0
    else:
        ndocs = len(docs)
        ni = np.zeros(len(word_of), np.int64)
        at = 0
        for d in docs:
            ni[np.unique(word[at:at + d.shape[0]])] += 1
            at += d.shape[0]
        for nid, w in word_of.items():
            if ni[w] > 0:
                weight[nid] = math.log(float(ndocs) / float(ni[w]))
    nodes = np.zeros(nn, NODE_DTYPE)
    nodes["node_id"] = np.arange(1, nn + 1)
    nodes["parent_id"] = T.parent[1:]
    nodes["weight"] = weight[1:]
    if nn:
        nodes["descriptor"] = np.stack(T.ndesc[1:])
    words = np.zeros(len(word_of), WORD_DTYPE)
    words["word_id"] = list(word_of.values())
    words["node_id"] = list(word_of.keys())
    stats = dict(nodes=nn, words=len(word_of), rounds_total=T.rounds_total, rounds_max=T.rounds_max, empty_groups=T.empty,
                 capped_nodes=T.capped)
    return dict(nodes=nodes, words=words, stats=stats, leaf=T.leaf, word=word, children=T.children, ndesc=T.ndesc)


def uniform_docs(rng, n_docs=5, lo=50, hi=400):
    """the documents tests/test_bow_cpu.py trains its fuzz vocabularies on"""
    docs = [rng.integers(0, 256, (int(rng.integers(lo, hi)), 32), dtype=np.uint8) for _ in range(n_docs)]
    return [np.concatenate([d, docs[0][:20]]) for d in docs]


def clustered_docs(rng, n_docs, n_per, n_proto, flips):
    """prototype descriptors with `flips` random bits flipped in each copy: inputs on which groups run empty"""
    proto = rng.integers(0, 256, (n_proto, 32), dtype=np.uint8)
    docs = []
    for _ in range(n_docs):
        d = np.unpackbits(proto[rng.integers(0, n_proto, n_per)], axis=1)
        for row in d:
            row[rng.integers(0, 256, flips)] ^= 1
        docs.append(np.packbits(d, axis=1))
    return docs


def duplicate_docs(rng, n_docs=4, n_distinct=30, max_rep=12):
    """a few distinct descriptors, each repeated 1 .. max_rep times, shuffled over the documents: nodes with fewer distinct rows
    than k (the seeding's early break) and trivial nodes made of duplicates"""
    base = rng.integers(0, 256, (n_distinct, 32), dtype=np.uint8)
    rows = np.repeat(base, rng.integers(1, max_rep + 1, n_distinct), axis=0)
    rows = rows[rng.permutation(rows.shape[0])]
    cuts = np.sort(rng.integers(0, rows.shape[0] + 1, n_docs - 1))
    return [rows[a:b] for a, b in zip(np.concatenate([[0], cuts]), np.concatenate([cuts, [rows.shape[0]]]))]


# The inputs on which tests/test_bow_train_cpu.py holds this module to the reference's compiled create: stated here once, for
# that file and for the tests that walk the same inputs again (tests/test_bow_train_cases_cpu.py).
WEIGHTINGS = [TF_IDF, TF, IDF, BINARY]
UNIFORM_K, UNIFORM_L = [2, 3, 10], [1, 2, 4]
DUPLICATE_KL = [(10, 2), (3, 4), (2, 4)]
DEPARTURE_CLUSTERED = (33, 4, 3, TF_IDF, 50)                       # (rng seed, k, L, weighting, draw seed): groups run empty
DEPARTURE_CAPPED = (1, 4, 2, TF, 1, (1, 2))                        # (rng seed, k, L, weighting, draw seed, the caps)


def uniform_seed0(k, L, weighting):
    return 300 + 16 * k + 4 * L + weighting


def duplicate_seed0(k, L, weighting):
    return 500 + 16 * k + 4 * L + weighting


def clean_input(make_docs, k, L, weighting, seed0):
    """-> (docs, seed, train(docs, ..., LibcDraws(seed))) for the first seed of seed0 .. seed0 + 7 on which the restatement sees
    no empty group and no capped node, or None: only such an input may reach the reference (which would read a released
    matrix on any other and take the process down)."""
    for seed in range(seed0, seed0 + 8):
        docs = make_docs(np.random.default_rng(seed))
        mine = train(docs, k, L, weighting, LibcDraws(seed))
        if mine["stats"]["empty_groups"] == 0 and mine["stats"]["capped_nodes"] == 0:
            return docs, seed, mine
    return None


def reference_records(O, docs, k, L, weighting, seed):
    """The reference's own create() through the compiled DBoW2 (O: the module oracle.oracle; its ref_dbow_train must exist) ->
    (nodes in ascending node id, words), as train() returns them.  Only for inputs on which train(..., LibcDraws(seed)) reports
    no empty group and no capped node: on any other the reference reads a released matrix."""
    rv = O.ref_dbow_train(k, L, weighting, docs, seed)
    _, nid, pid, wt, strings, wid, wn = rv.export()
    rv.close()
    o = np.argsort(nid, kind="stable")
    nodes = np.zeros(len(nid), NODE_DTYPE)
    nodes["node_id"], nodes["parent_id"], nodes["weight"] = np.asarray(nid)[o], np.asarray(pid)[o], np.asarray(wt)[o]
    if len(nid):
        nodes["descriptor"] = np.array([O.ref_forb_from_string(s) for s in strings], np.uint8).reshape(-1, 32)[o]
    words = np.zeros(len(wid), WORD_DTYPE)
    words["word_id"], words["node_id"] = wid, wn
    return nodes, words


def same_records(a_nodes, a_words, b_nodes, b_words):
    return (a_nodes.shape == b_nodes.shape and a_words.shape == b_words.shape and
            all(np.array_equal(a_nodes[f], b_nodes[f]) for f in ("node_id", "parent_id", "descriptor")) and
            np.array_equal(a_nodes["weight"].view(np.uint64), b_nodes["weight"].view(np.uint64)) and
            all(np.array_equal(a_words[f], b_words[f]) for f in ("word_id", "node_id")))
