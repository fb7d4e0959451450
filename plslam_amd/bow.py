"""The bag-of-words entry points (plslam_bow_*, include/plslam_hip.h): the ctypes binding (BowVocabulary, BowDatabase) and the
DBoW2 vocabularies it is fed with.

``load_vocabulary`` reads the files PL-SLAM loads at MapHandler construction (src/mapHandler.cpp:38-41 ->
TemplatedVocabulary::load(filename), which opens them with cv::FileStorage): the YAML layout written by
TemplatedVocabulary::save (3rdparty/DBoW2/include/DBoW2/TemplatedVocabulary.h:1340-1435), plain or gzip-compressed, with
every descriptor in FORB::toString's form -- 32 space-separated byte values (src/DBoW2/FORB.cpp:104-140).
``save_vocabulary`` writes that layout.  ``synth_vocabulary`` builds vocabularies for tests and tools.

Node records stay in FILE order: load() appends each node to its parent's children list in that order (:1466-1474), and
the descent keeps the first child of that list on a distance tie.
"""
from __future__ import annotations

import ctypes as C
import gzip
import re
from dataclasses import dataclass

import numpy as np

from ._lib import Handle, _arr, _check, _p, proto

BOW_TF_IDF, BOW_TF, BOW_IDF, BOW_BINARY = 0, 1, 2, 3
BOW_L1_NORM = 0
BOW_MAX_SET = 16384      # include/plslam_hip.h: PLSLAM_BOW_MAX_SET

# plslam_bow_node / plslam_bow_word as numpy records
BOW_NODE_DTYPE = np.dtype([("node_id", np.int32), ("parent_id", np.int32), ("weight", np.float64), ("descriptor", np.uint8, 32)])
BOW_WORD_DTYPE = np.dtype([("word_id", np.int32), ("node_id", np.int32)])


class BowVocabDesc(C.Structure):
    """plslam_bow_vocab_desc"""
    _fields_ = [("k", C.c_int32), ("L", C.c_int32), ("scoring_type", C.c_int32), ("weighting_type", C.c_int32),
                ("n_nodes", C.c_int32), ("n_words", C.c_int32), ("nodes", C.c_void_p), ("words", C.c_void_p)]


class BowPlStats(C.Structure):
    """plslam_bow_pl_stats"""
    _fields_ = [("n_pt", C.c_int32), ("n_ls", C.c_int32), ("std_pt", C.c_double), ("std_ls", C.c_double)]


def _bow_stats(stats):
    if stats is None:
        return None
    if isinstance(stats, BowPlStats):
        return stats
    n_pt, n_ls, std_pt, std_ls = stats
    return BowPlStats(int(n_pt), int(n_ls), float(std_pt), float(std_ls))


_vp, _i32 = C.c_void_p, C.c_int32
proto("plslam_bow_vocab_create", [_vp, C.POINTER(BowVocabDesc), C.POINTER(_vp)])
proto("plslam_bow_transform", [_vp, _vp, _vp, _i32, _vp, _vp, _vp, _vp, _vp])
proto("plslam_bow_transform_dev", [_vp, _vp, _vp, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp])
proto("plslam_bow_vocab_destroy", [_vp], None)


class BowVocabulary(Handle):
    """plslam_bow_vocab: a DBoW2 vocabulary on the device (TemplatedVocabulary::load, TemplatedVocabulary.h:1437-1485).

    voc: anything with the fields k, L, scoring_type, weighting_type, nodes (BOW_NODE_DTYPE records in file order) and words
    (BOW_WORD_DTYPE records) -- the Vocabulary below."""

    def __init__(self, ctx: Context, voc):
        nodes = np.ascontiguousarray(voc.nodes, dtype=BOW_NODE_DTYPE)
        words = np.ascontiguousarray(voc.words, dtype=BOW_WORD_DTYPE)
        desc = BowVocabDesc(int(voc.k), int(voc.L), int(voc.scoring_type), int(voc.weighting_type), nodes.shape[0],
                            words.shape[0], _p(nodes), _p(words))
        h = C.c_void_p()
        _check(ctx._L.plslam_bow_vocab_create(ctx.handle, C.byref(desc), C.byref(h)), "plslam_bow_vocab_create")
        self._open(ctx, "plslam_bow_vocab_destroy", h)

    def transform(self, desc, offsets):
        """TemplatedVocabulary::transform over ragged sets -> (word_id[total], word_weight[total], bow_word[total],
        bow_weight[total], bow_len[nsets]); set s's BowVector is bow_word / bow_weight[offsets[s] : offsets[s] + bow_len[s]]."""
        d = _arr(desc, np.uint8, (-1, 32))
        off = _arr(offsets, np.int32)
        nsets = off.shape[0] - 1
        total = d.shape[0]
        word, weight = np.empty(total, np.int32), np.empty(total, np.float64)
        bword, bweight = np.empty(total, np.int32), np.empty(total, np.float64)
        blen = np.empty(max(nsets, 0), np.int32)
        _check(self._L.plslam_bow_transform(self._h, _p(d), _p(off), nsets, _p(word), _p(weight), _p(bword), _p(bweight),
                                            _p(blen)), "plslam_bow_transform")
        return word, weight, bword, bweight, blen

    def transform_dev(self, d_desc, d_offsets, nsets, total, max_set, d_word, d_weight, d_bow_word, d_bow_weight, d_bow_len,
                      stream=None):
        """Device-pointer form (addresses as ints); enqueues on `stream` (None = the context's stream), no sync."""
        _check(self._L.plslam_bow_transform_dev(self._h, int(d_desc), int(d_offsets), int(nsets), int(total), int(max_set),
                                                int(d_word), d_weight or None, int(d_bow_word), int(d_bow_weight),
                                                int(d_bow_len), stream or None), "plslam_bow_transform_dev")


proto("plslam_bow_db_create", [_vp, _vp, _vp, _i32, C.POINTER(_vp)])
proto("plslam_bow_db_size", [_vp, C.POINTER(_i32)])
proto("plslam_bow_db_insert", [_vp, _i32, _vp, _i32, _vp, _i32, C.POINTER(BowPlStats), _vp, _vp])
proto("plslam_bow_db_insert_dev", [_vp, _i32, _vp, _i32, _vp, _i32, C.POINTER(BowPlStats), _vp, _vp])
proto("plslam_bow_db_score", [_vp, _vp, _i32, _vp])
proto("plslam_bow_db_destroy", [_vp], None)


class BowDatabase(Handle):
    """plslam_bow_db: the keyframes' BowVectors on the device and MapHandler::insertKFBowVector{P,L,PL}
    (src/mapHandler.cpp:3007-3128).  vocab_p / vocab_l: BowVocabulary or None (the mode follows :196-201).  Close it before
    its vocabularies."""

    def __init__(self, ctx: Context, vocab_p, vocab_l, capacity_hint: int = 0):
        self._voc = (vocab_p, vocab_l)          # kept alive as long as the database
        h = C.c_void_p()
        _check(ctx._L.plslam_bow_db_create(ctx.handle, vocab_p.handle if vocab_p else None,
                                           vocab_l.handle if vocab_l else None, int(capacity_hint), C.byref(h)),
               "plslam_bow_db_create")
        self._open(ctx, "plslam_bow_db_destroy", h)

    @property
    def size(self) -> int:
        n = C.c_int32()
        _check(self._L.plslam_bow_db_size(self._h, C.byref(n)), "plslam_bow_db_size")
        return n.value

    def insert(self, kf_idx, pdesc=None, ldesc=None, stats=None, alive=None, conf_row=None):
        """One keyframe: conf_row (float64, >= kf_idx + 1 entries, updated in place; None = a fresh NaN row) gets
        score(new, i) for every alive i < kf_idx and the self score at kf_idx.  stats: (n_pt, n_ls, std_pt, std_ls), PL mode.
        alive: kf_idx uint8 flags (None = all alive)."""
        kf_idx = int(kf_idx)
        pd = _arr(pdesc if pdesc is not None else np.zeros((0, 32), np.uint8), np.uint8, (-1, 32))
        ld = _arr(ldesc if ldesc is not None else np.zeros((0, 32), np.uint8), np.uint8, (-1, 32))
        al = _arr(np.ones(kf_idx, np.uint8) if alive is None else alive, np.uint8)
        assert al.shape[0] >= kf_idx
        row = np.full(kf_idx + 1, np.nan) if conf_row is None else conf_row
        assert row.dtype == np.float64 and row.flags.c_contiguous and row.shape[0] >= kf_idx + 1
        st = _bow_stats(stats)
        _check(self._L.plslam_bow_db_insert(self._h, kf_idx, _p(pd), pd.shape[0], _p(ld), ld.shape[0],
                                            C.byref(st) if st is not None else None, _p(al), _p(row)), "plslam_bow_db_insert")
        return row

    def insert_dev(self, kf_idx, d_pdesc, n_pdesc, d_ldesc, n_ldesc, stats, d_alive, d_conf_row):
        """Device-pointer form (addresses as ints), enqueued on the context's stream, no sync."""
        st = _bow_stats(stats)
        _check(self._L.plslam_bow_db_insert_dev(self._h, int(kf_idx), d_pdesc or None, int(n_pdesc), d_ldesc or None,
                                                int(n_ldesc), C.byref(st) if st is not None else None, d_alive or None,
                                                int(d_conf_row)), "plslam_bow_db_insert_dev")

    def score(self, queries):
        """plslam_bow_db_score -> (nq, size) float64; NaN where a keyframe was never inserted."""
        q = _arr(queries, np.int32)
        out = np.empty((q.shape[0], self.size), np.float64)
        _check(self._L.plslam_bow_db_score(self._h, _p(q), q.shape[0], _p(out)), "plslam_bow_db_score")
        return out


# ---- the vocabulary files -----------------------------------------------------------------------------------------------------


@dataclass
class Vocabulary:
    k: int
    L: int
    scoring_type: int
    weighting_type: int
    nodes: np.ndarray          # BOW_NODE_DTYPE, file order (the root has no record)
    words: np.ndarray          # BOW_WORD_DTYPE, file order


_NUM = r"[-+]?(?:\.[Ii]nf|\.[Nn]a[Nn]|[0-9.]+(?:[eE][-+]?[0-9]+)?)"
_NODE_RE = re.compile(r"nodeId\s*:\s*(\d+)\s*,\s*parentId\s*:\s*(\d+)\s*,\s*weight\s*:\s*(" + _NUM + r")\s*,\s*"
                      r"descriptor\s*:\s*\"([^\"]*)\"")
_WORD_RE = re.compile(r"wordId\s*:\s*(\d+)\s*,\s*nodeId\s*:\s*(\d+)")


def _yaml_double(s: str) -> float:
    t = s.lower().lstrip("+")
    if t in (".inf", "-.inf", ".nan", "-.nan"):
        return float(t.replace(".", ""))
    return float(s)


def _scalar(text: str, key: str) -> int:
    m = re.search(r"\b" + key + r"\s*:\s*(-?\d+)", text)
    if not m:
        raise ValueError(f"vocabulary file: no '{key}'")
    return int(m.group(1))


def load_vocabulary(path: str) -> Vocabulary:
    """A file in TemplatedVocabulary::save's YAML layout ('.gz' = gzip-compressed, as cv::FileStorage reads it)."""
    opener = gzip.open if path.endswith(".gz") else open
    with opener(path, "rt") as f:
        text = f.read()
    head, sep, tail = text.partition("nodes")
    if not sep:
        raise ValueError("vocabulary file: no 'nodes'")
    node_part, _, word_part = tail.partition("words")
    k, L = _scalar(head, "k"), _scalar(head, "L")
    scoring, weighting = _scalar(head, "scoringType"), _scalar(head, "weightingType")
    recs = _NODE_RE.findall(node_part)
    nodes = np.zeros(len(recs), BOW_NODE_DTYPE)
    if recs:
        nodes["node_id"] = [int(r[0]) for r in recs]
        nodes["parent_id"] = [int(r[1]) for r in recs]
        nodes["weight"] = [_yaml_double(r[2]) for r in recs]
        nodes["descriptor"] = np.array([np.array(r[3].split(), dtype=np.int64) for r in recs]).reshape(-1, 32).astype(np.uint8)
    wrecs = _WORD_RE.findall(word_part)
    words = np.zeros(len(wrecs), BOW_WORD_DTYPE)
    if wrecs:
        words["word_id"] = [int(r[0]) for r in wrecs]
        words["node_id"] = [int(r[1]) for r in wrecs]
    return Vocabulary(k, L, scoring, weighting, nodes, words)


def _fmt_double(x: float) -> str:
    if np.isnan(x):
        return ".Nan"
    if np.isinf(x):
        return ".Inf" if x > 0 else "-.Inf"
    return repr(float(x))          # shortest string that reads back to the same double


def save_vocabulary(path: str, voc: Vocabulary, name: str = "vocabulary") -> None:
    """TemplatedVocabulary::save's layout (:1340-1435) as cv::FileStorage writes YAML; records in the order of voc."""
    out = ["%YAML:1.0", "---", f"{name}:", f"   k: {int(voc.k)}", f"   L: {int(voc.L)}",
           f"   scoringType: {int(voc.scoring_type)}", f"   weightingType: {int(voc.weighting_type)}", "   nodes:"]
    for r in voc.nodes:
        d = " ".join(str(int(b)) for b in r["descriptor"]) + " "
        out.append(f"      - {{ nodeId:{int(r['node_id'])}, parentId:{int(r['parent_id'])}, weight:{_fmt_double(r['weight'])},\n"
                   f"          descriptor:\"{d}\" }}")
    out.append("   words:")
    for r in voc.words:
        out.append(f"      - {{ wordId:{int(r['word_id'])}, nodeId:{int(r['node_id'])} }}")
    text = "\n".join(out) + "\n"
    opener = gzip.open if path.endswith(".gz") else open
    with opener(path, "wt") as f:
        f.write(text)


def _flip(rng, d: np.ndarray, log2_inv_p: int) -> np.ndarray:
    """Every bit flipped with probability 2^-log2_inv_p (the AND of that many random masks)."""
    m = rng.integers(0, 256, d.shape, dtype=np.uint8)
    for _ in range(log2_inv_p - 1):
        m &= rng.integers(0, 256, d.shape, dtype=np.uint8)
    return d ^ m


def synth_vocabulary(rng: np.random.Generator, k: int = 10, L: int = 6, weighting: int = BOW_TF_IDF, irregular: bool = False,
                     leaf_frac: float = 0.25, stop_frac: float = 0.0, shuffle_ids: bool = False,
                     permute_words: bool = False, flip_log2: int = 2, scoring: int = BOW_L1_NORM) -> Vocabulary:
    """A vocabulary tree of branching k and depth L, built level by level: a child's descriptor is its parent's with every bit
    flipped with probability 2^-flip_log2 (so that descents follow the tree rather than ties); level 1 is random.
      irregular      1..k children per node, and a node above level L becomes a leaf with probability leaf_frac
      stop_frac      fraction of the words whose weight is 0 (stopped)
      shuffle_ids    node ids are a random permutation (children-list order no longer follows id order)
      permute_words  word ids are a random permutation of the leaves' order
    Records come in save()'s order: a stack of parents, every parent's children written together (:1376-1405).
    k = 10, L = 6 (1 111 110 node records) takes about a second."""
    parents = [np.zeros(0, np.int64)]
    descs = [np.zeros((1, 32), np.uint8)]          # the root's (unused)
    frontier = np.zeros(1, np.int64)
    n = 1
    for level in range(1, L + 1):
        if frontier.size == 0:
            break
        counts = rng.integers(1, k + 1, frontier.size) if irregular else np.full(frontier.size, k)
        par = np.repeat(frontier, counts)
        if level == 1:
            d = rng.integers(0, 256, (par.size, 32), dtype=np.uint8)
        else:
            d = _flip(rng, np.concatenate(descs)[par], flip_log2)
        new = np.arange(n, n + par.size)
        n += par.size
        parents.append(par)
        descs.append(d)
        if level == L:
            break
        if irregular:
            keep = rng.random(new.size) >= leaf_frac
            keep[0] = True                              # at least one branch reaches level L
            frontier = new[keep]
        else:
            frontier = new
    parent = np.concatenate([np.zeros(1, np.int64)] + parents[1:])     # parent[0] unused
    desc = np.concatenate(descs)
    nn = n - 1
    # children of every node, in creation order (CSR)
    kids = np.argsort(parent[1:], kind="stable") + 1
    start = np.zeros(n + 1, np.int64)
    np.add.at(start, parent[1:] + 1, 1)
    start = np.cumsum(start)
    nkids = start[1:] - start[:-1]
    # save()'s order: pop a parent, write all its children, push the ones that have children
    order = np.empty(nn, np.int64)
    w = 0
    stack = [0]
    while stack:
        p = stack.pop()
        c = kids[start[p]:start[p + 1]]
        order[w:w + c.size] = c
        w += c.size
        stack.extend(c[nkids[c] > 0].tolist())
    ids = np.arange(n)
    if shuffle_ids:
        ids[1:] = rng.permutation(nn) + 1
    leaves = order[nkids[order] == 0]
    nw = leaves.size
    wid = rng.permutation(nw) if permute_words else np.arange(nw)
    lw = rng.uniform(0.05, 4.0, nw)
    if weighting in (1, 3):                            # TF / BINARY: every word weighs 1 (HKmeans' setNodeWeights)
        lw[:] = 1.0
    if stop_frac > 0:
        lw[rng.random(nw) < stop_frac] = 0.0
    weight = np.zeros(n)
    weight[leaves] = lw
    nodes = np.zeros(nn, BOW_NODE_DTYPE)
    nodes["node_id"] = ids[order]
    nodes["parent_id"] = ids[parent[order]]
    nodes["weight"] = weight[order]
    nodes["descriptor"] = desc[order]
    words = np.zeros(nw, BOW_WORD_DTYPE)
    wo = np.argsort(wid)                               # save() writes the words in id order
    words["word_id"] = wid[wo]
    words["node_id"] = ids[leaves[wo]]
    return Vocabulary(k, L, scoring, weighting, nodes, words)


def near_leaf_descriptors(rng: np.random.Generator, voc: Vocabulary, n: int, flip_log2: int = 5) -> np.ndarray:
    """n descriptors made from random leaves' descriptors with a few bits flipped (descents that follow real branches)."""
    rec = np.empty(int(voc.nodes["node_id"].max()) + 1, np.int64)
    rec[voc.nodes["node_id"]] = np.arange(voc.nodes.shape[0])
    pick = rng.choice(voc.words["node_id"], n)
    return _flip(rng, voc.nodes["descriptor"][rec[pick]], flip_log2)
