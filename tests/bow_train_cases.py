"""Named inputs that take the vocabulary training (plslam_amd/csrc/bow_train.hip, K111-K129; specification = the restatement
tests/bow_train_ref.py with the counter draws) off uniform bytes, k <= 10 and L <= 4, for tests/test_bow_train_cases_cpu.py
(which checks from the restatement alone that each case reaches the branch it is named for) and for
tests/test_gpu_bow_train_edges.py (the same inputs through the device, compared in every bit).  numpy only.

A case is (docs, k, L, weighting, seed, max_iters); CASES maps its name to its builder, GROUPS lists the names of a group.
expect(name) is the restatement's result on it, computed once per process, with the draws it asked; level_profile and figures
read what a case reaches off that result, so the restatement itself carries no instrumentation.

  deep        k = 2 and 3 down to L = 8, 13 and 16 (PLSLAM_BOW_TRAIN_MAX_L): levels of more than 1024 visited and more than 256
              running nodes (a second tile of the flag scan, a second workgroup of the per-node kernels), waves that hold ten
              and more (node, cluster) groups, a tree that ends before L
  wide        k = 64, 65 and 256 (PLSLAM_BOW_TRAIN_MAX_K): as many clusters as lanes, one more, and 255 seeding rounds
  far, tied   rows that alternate between all-0x00 and all-0xFF (a distance of 256: the ninth bit of the popcount sum), the
              same with two random bits flipped, and rows that are zero but for byte 0 and two bits of byte 31 (most
              comparisons of the assignment are ties, most majorities fall on n / 2)
  draws       seeds made by seed_for: the root's cut is 0.0 and is drawn again, the cut equals the distance sum, the first
              centre is row n - 1 and row 0
  documents   499 cuts with empty documents among them; more documents than rows
  scale       65536 words and more (a third radix pass of the word sort), more than 1024 tiles of the prefix sum
"""
from __future__ import annotations

import functools

import numpy as np

from tests import bow_train_ref as T

_M64 = (1 << 64) - 1
_GOLDEN = 0x9E3779B97F4A7C15
_INV1 = pow(0xBF58476D1CE4E5B9, -1, 1 << 64)
_INV2 = pow(0x94D049BB133111EB, -1, 1 << 64)
R_MAX = 2 ** 31 - 1


def unmix(z: int) -> int:
    """the inverse of T.mix64: the three xor-shifts undone, the two multipliers inverted mod 2^64"""
    z &= _M64
    z ^= (z >> 31) ^ (z >> 62)
    z = (z * _INV2) & _M64
    z ^= (z >> 27) ^ (z >> 54)
    z = (z * _INV1) & _M64
    z ^= (z >> 30) ^ (z >> 60)
    return z


def seed_for(j: int, t: int, r: int, low: int = 0x1234567) -> int:
    """the seed whose root draw (j, t) is r: T.counter_draw(T.root_key(seed), j, t) == r.  low: the 33 bits the draw drops."""
    assert 0 <= r < 2 ** 31 and 0 <= low < 2 ** 33
    return unmix((unmix((r << 33) | low) - _GOLDEN * ((j << 32) + t + 1)) & _M64)


class RecordingDraws(T.CounterDraws):
    """the counter draws, with every question kept: asked (key, j, t), firsts (key, n, index), cuts (key, j, dist_sum, cut)"""

    def __init__(self, seed):
        super().__init__(seed)
        self.asked, self.firsts, self.cuts = [], [], []

    def r(self, key, j, t):
        self.asked.append((key, j, t))
        return super().r(key, j, t)

    def first(self, key, n):
        i = super().first(key, n)
        self.firsts.append((key, n, i))
        return i

    def cut(self, key, j, dist_sum):
        c = super().cut(key, j, dist_sum)
        self.cuts.append((key, j, dist_sum, c))
        return c


# ---- the inputs ------------------------------------------------------------------------------------------------------------
def cut_docs(rng, rows, n_docs):
    """rows cut at n_docs - 1 sorted random points; equal points leave empty documents"""
    cuts = np.sort(rng.integers(0, rows.shape[0] + 1, n_docs - 1))
    return [rows[a:b] for a, b in zip(np.concatenate([[0], cuts]), np.concatenate([cuts, [rows.shape[0]]]))]


def _uniform(rs, n, n_docs):
    rng = np.random.default_rng(rs)
    return cut_docs(rng, rng.integers(0, 256, (n, 32), dtype=np.uint8), n_docs)


def _alternating(n):
    rows = np.zeros((n, 32), np.uint8)
    rows[1::2] = 0xFF
    return rows


def _alternating_flipped(rs, n, flips):
    rng = np.random.default_rng(rs)
    bits = np.unpackbits(_alternating(n), axis=1)
    for row in bits:
        row[rng.integers(0, 256, flips)] ^= 1
    return np.packbits(bits, axis=1)


def _low_entropy(rs, n):
    """zero but for byte 0 (uniform) and byte 31 (0 .. 3): 10 bits of 256 ever differ"""
    rng = np.random.default_rng(rs)
    rows = np.zeros((n, 32), np.uint8)
    rows[:, 0] = rng.integers(0, 256, n)
    rows[:, 31] = rng.integers(0, 4, n)
    return rows


def _sparse_docs(rs, n, n_docs):
    """n rows, each a document of its own, spread over n_docs documents: the others are empty"""
    rng = np.random.default_rng(rs)
    rows = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    at = np.sort(rng.choice(n_docs, n, replace=False))
    docs = [rows[:0]] * n_docs
    for i, d in enumerate(at):
        docs[int(d)] = rows[i:i + 1]
    return docs


def _scale_tiles():
    rng = np.random.default_rng(1201)
    rows = rng.integers(0, 256, (2 ** 20 + 1500, 32), dtype=np.uint8)
    return [rows[:400000], rows[:0], rows[400000:]]


DRAW_SEEDS = {"draw_retry_j1": (1, 0, 0), "draw_retry_j2": (2, 0, 0), "draw_cut_is_the_sum": (1, 0, R_MAX),
              "draw_first_is_the_last_row": (0, 0, R_MAX), "draw_first_is_row_0": (0, 0, 0)}

CASES = {
    "deep_k2_L13_tfidf": lambda: (_uniform(1101, 6000, 40), 2, 13, T.TF_IDF, 11, 1000),
    "deep_k2_L13_binary": lambda: (_uniform(1101, 6000, 40), 2, 13, T.BINARY, 11, 1000),
    "deep_k2_L16_tfidf": lambda: (_uniform(1102, 1500, 40), 2, 16, T.TF_IDF, 12, 1000),
    "deep_k2_L16_binary": lambda: (_uniform(1102, 1500, 40), 2, 16, T.BINARY, 12, 1000),
    "deep_k3_L8_tfidf": lambda: (_uniform(1103, 2000, 40), 3, 8, T.TF_IDF, 13, 1000),
    "deep_k3_L8_binary": lambda: (_uniform(1103, 2000, 40), 3, 8, T.BINARY, 13, 1000),
    "wide_k64": lambda: (_uniform(1111, 2000, 5), 64, 2, T.IDF, 21, 1000),
    "wide_k65": lambda: (_uniform(1112, 1300, 5), 65, 2, T.TF_IDF, 22, 1000),
    "wide_k256": lambda: (_uniform(1113, 700, 5), 256, 2, T.IDF, 23, 1000),
    "alternating_k2": lambda: (cut_docs(np.random.default_rng(1121), _alternating(600), 4), 2, 2, T.IDF, 31, 1000),
    "alternating_k3": lambda: (cut_docs(np.random.default_rng(1122), _alternating(600), 4), 3, 2, T.TF_IDF, 32, 1000),
    "alternating_flipped": lambda: (cut_docs(np.random.default_rng(1123), _alternating_flipped(1123, 1200, 2), 6), 3, 4, T.TF_IDF,
                                    33, 1000),
    "low_entropy_k4_L5": lambda: (cut_docs(np.random.default_rng(1124), _low_entropy(1124, 2500), 8), 4, 5, T.TF_IDF, 34, 1000),
    "low_entropy_k10_L3": lambda: (cut_docs(np.random.default_rng(1125), _low_entropy(1125, 2500), 8), 10, 3, T.IDF, 35, 1000),
    "low_entropy_k2_L8": lambda: (cut_docs(np.random.default_rng(1126), _low_entropy(1126, 2500), 8), 2, 8, T.TF_IDF, 36, 1000),
    **{name: (lambda a=a: (_uniform(1131, 300, 3), 3, 2, T.TF_IDF, seed_for(*a), 1000)) for name, a in DRAW_SEEDS.items()},
    "documents_499_cuts_idf": lambda: (_uniform(1141, 3000, 500), 10, 3, T.IDF, 41, 1000),
    "documents_499_cuts_tfidf": lambda: (_uniform(1141, 3000, 500), 10, 3, T.TF_IDF, 41, 1000),
    "documents_more_than_rows_idf": lambda: (_sparse_docs(1142, 40, 200), 3, 3, T.IDF, 42, 1000),
    "documents_more_than_rows_tfidf": lambda: (_sparse_docs(1142, 40, 200), 3, 3, T.TF_IDF, 42, 1000),
    "scale_words": lambda: (_uniform(1151, 70000, 50), 64, 3, T.IDF, 51, 1),
    "scale_tiles": lambda: (_scale_tiles(), 2, 1, T.IDF, 52, 1),
}
GROUPS = {g: [n for n in CASES if n.startswith(p)] for g, p in
          (("deep", "deep_"), ("wide", "wide_"), ("far_tied", ("alternating", "low_entropy")), ("draws", "draw_"),
           ("documents", "documents_"), ("scale", "scale_"))}


@functools.lru_cache(maxsize=None)
def case(name):
    return CASES[name]()


@functools.lru_cache(maxsize=None)
def expect(name):
    """-> (the restatement's result, the RecordingDraws); computed once and left unchanged"""
    docs, k, L, weighting, seed, max_iters = case(name)
    draws = RecordingDraws(seed)
    return T.train(docs, k, L, weighting, draws, max_iters), draws


# ---- what a case reaches, from the restatement's records ------------------------------------------------------------------------
def _paths(exp):
    """path[row, d]: the row's node of depth d in the training partition (0: the root), -1 below its leaf"""
    parent = np.concatenate([[0], exp["nodes"]["parent_id"]]).astype(np.int64)
    depth = np.zeros(parent.shape[0], np.int64)
    for i in range(1, parent.shape[0]):                            # (a parent's id is smaller than its children's)
        depth[i] = depth[parent[i]] + 1
    leaf = np.asarray(exp["leaf"], np.int64)
    D = int(depth.max())
    path = np.full((leaf.shape[0], D + 1), -1, np.int64)
    cur = leaf.copy()
    for d in range(D, 0, -1):
        m = depth[cur] == d
        path[m, d] = cur[m]
        cur[m] = parent[cur[m]]
    path[:, 0] = 0
    return path


def figures(name):
    """What the distances of a case reach, recomputed from its input, its finished tree and its first draw -- for a case without
    a capped node, where every running node's last Lloyd round assigned its rows to the centres the tree holds, and those
    centres are FORB::meanValue of the groups the partition shows:
      root_max_min_d   the largest distance of a row to the root's first centre (the seeding's first round of min distances)
      tied_rows        rows of running nodes whose minimum over the node's centres is reached twice or more in that last round
      half_majorities  bits of those centres whose count is exactly n / 2 in a group of even n: set by '>=' alone"""
    docs, k, _, _, _, _ = case(name)
    exp, draws = expect(name)
    assert exp["stats"]["capped_nodes"] == 0
    desc = np.concatenate([np.asarray(d, np.uint8).reshape(-1, 32) for d in docs])
    q = desc.view(np.uint64)
    cent = np.concatenate([np.zeros((1, 32), np.uint8), exp["nodes"]["descriptor"]]).view(np.uint64)
    kids_of = exp["children"]
    path = _paths(exp)
    out = dict(root_max_min_d=0, tied_rows=0, half_majorities=0)
    if desc.shape[0] > k:
        first = draws.firsts[0][2]
        out["root_max_min_d"] = int(np.bitwise_count(q ^ q[first]).sum(axis=1).max())
    for lv in range(1, path.shape[1]):
        live = np.flatnonzero(path[:, lv] >= 0)
        for v in np.unique(path[live, lv - 1]):
            rows = live[path[live, lv - 1] == v]
            if rows.shape[0] <= k:
                continue
            kids = np.asarray(kids_of[int(v)], np.int64)
            d = np.bitwise_count(q[rows][:, None, :] ^ cent[kids][None, :, :]).sum(axis=2)
            assert np.array_equal(kids[np.argmin(d, axis=1)], path[rows, lv])          # the partition IS that last round
            out["tied_rows"] += int(((d == d.min(axis=1, keepdims=True)).sum(axis=1) > 1).sum())
            for c in kids:
                g = desc[rows[path[rows, lv] == c]]
                n = g.shape[0]
                if n > 1 and n % 2 == 0:
                    cnt = np.unpackbits(g, axis=1).astype(np.int64).sum(axis=0)
                    assert np.array_equal(np.packbits(cnt >= n // 2), cent[c].view(np.uint8))
                    out["half_majorities"] += int((cnt == n // 2).sum())
    return out


def level_profile(exp, k):
    """Per level 1, 2, ...: (visited nodes, running nodes: more than k rows, the largest number of distinct (node, cluster)
    groups in 64 consecutive positions -- a wave -- of the level's row order).  A level's rows are grouped by node, the nodes in
    the order they were made (ascending id among the nodes of one depth), the rows of a node in their original order."""
    path = _paths(exp)
    out = []
    for lv in range(1, path.shape[1]):
        live = np.flatnonzero(path[:, lv] >= 0)
        order = live[np.argsort(path[live, lv - 1], kind="stable")]
        node, group = path[order, lv - 1], path[order, lv]
        _, rows = np.unique(node, return_counts=True)
        pad = (-group.shape[0]) % 64
        w = np.sort(np.concatenate([group, np.full(pad, group[-1])]).reshape(-1, 64), axis=1)
        out.append((int(rows.shape[0]), int((rows > k).sum()), int(((w[:, 1:] != w[:, :-1]).sum(axis=1) + 1).max())))
    return out
