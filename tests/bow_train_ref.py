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


def train(docs, k, L, weighting, draws, max_iters=1000):
    """create(training_features) for TemplatedVocabulary(k, L, weighting, L1_NORM).  docs: a list of (n_i, 32) uint8 arrays.
    Returns a dict: nodes (NODE_DTYPE, ascending node id, no root), words (WORD_DTYPE), stats, leaf (per descriptor: the node
    of the training partition), word (per descriptor: the word of the descent), key0."""
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
    word = np.array([word_of[descend(T.children, T.ndesc, f)] for f in desc], np.int64).reshape(N)
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
    return dict(nodes=nodes, words=words, stats=stats, leaf=T.leaf, word=word)


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
