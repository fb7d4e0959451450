"""Generates tests/golden/bow_ref_golden.npz.  Run from the repo root IN THE BUILD CONTAINER (needs /root/reference):
    python tests/golden/make_bow_ref_golden.py

Outputs of the REFERENCE'S OWN DBoW2 (3rdparty/DBoW2: TemplatedVocabulary.h, BowVector.cpp, ScoringObject.cpp, FORB.cpp,
DUtils) and of MapHandler::insertKFBowVector{P,L,PL} (src/mapHandler.cpp:3007-3128, cut out of the file where it lies),
compiled into oracle/_ref by oracle/ref_wrap_dbow.cpp:
  voc__<name>__*   vocabularies as TemplatedVocabulary::save writes them (records in save()'s order; descriptors read back
                   with FORB::fromString); descriptor sets, as indices into the node descriptors followed by a pool of the
                   other distinct descriptors; each descriptor's (word, node weight), each set's BowVector (ascending ids)
                   and the score of every pair of sets
  run__<name>__*   keyframe runs (descriptors as indices into a pool) through the cut insertKFBowVector* text: the
                   final conf_matrix, cells the reference never wrote still holding the sentinel, with double cells (conf)
                   and as mapHandler.h:147 stores them (conf32)
Deterministic (fixed seeds).  Written only if tests/dbow_ref.py reproduces every reference output bit for bit.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from oracle import oracle as O  # noqa: E402
from plslam_amd import bow  # noqa: E402
from plslam_amd.capi import BOW_MAX_SET  # noqa: E402
from tests import dbow_ref as R  # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "bow_ref_golden.npz")
STAGE_NODES = 1228          # bow_plan.hpp: K19 stages the first 1228 breadth-first nodes in LDS
SENTINEL = -3.0             # not a score: conf_matrix cells the reference leaves alone keep it
SPECIAL = [-0.0, -1.5, float("nan"), float("inf"), 1e-310, float(np.finfo(np.float64).max)]


def bits_equal(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(a[~na].view(np.uint64), b[~nb].view(np.uint64))


def records(rv):
    """the reference's save() records -> bow.Vocabulary (descriptors parsed by FORB::fromString, and by bow.py's parser)"""
    head, nid, pid, w, strings, wid, wn = rv.export()
    desc = np.array([O.ref_forb_from_string(s) for s in strings], np.uint8).reshape(-1, 32)
    assert np.array_equal(desc, np.array([[int(x) for x in s.split()] for s in strings], np.uint8).reshape(-1, 32))
    nodes = np.zeros(nid.size, bow.BOW_NODE_DTYPE)
    nodes["node_id"], nodes["parent_id"], nodes["weight"], nodes["descriptor"] = nid, pid, w, desc
    words = np.zeros(wid.size, bow.BOW_WORD_DTYPE)
    words["word_id"], words["node_id"] = wid, wn
    return bow.Vocabulary(int(head[0]), int(head[1]), int(head[2]), int(head[3]), nodes, words)


def ref_load(v, weighting=None):
    """bow.Vocabulary -> the reference's load(), descriptors written as bow.save_vocabulary writes them"""
    strings = [" ".join(str(int(b)) for b in d) + " " for d in v.nodes["descriptor"]]
    return O.ref_dbow_load(v.k, v.L, v.scoring_type, v.weighting_type if weighting is None else weighting, v.nodes["node_id"],
                           v.nodes["parent_id"], v.nodes["weight"], strings, v.words["word_id"], v.words["node_id"])


def bfs_positions(v):
    """K19's layout: breadth-first from the root, each parent's children in list (record) order"""
    kids = {}
    for n, p in zip(v.nodes["node_id"].tolist(), v.nodes["parent_id"].tolist()):
        kids.setdefault(p, []).append(n)
    order = [0]
    for u in order:
        order.extend(kids.get(u, []))
    return {n: i for i, n in enumerate(order)}, kids


def node_desc(v):
    return dict(zip(v.nodes["node_id"].tolist(), [bytes(d) for d in v.nodes["descriptor"]]))


def midpoint(rng, a, b):
    """a descriptor at the same Hamming distance from a and b: agreeing bits copied, half the differing ones from each"""
    x = np.frombuffer(a, np.uint8).copy()
    ab = np.unpackbits(np.frombuffer(a, np.uint8))
    bb = np.unpackbits(np.frombuffer(b, np.uint8))
    diff = np.flatnonzero(ab != bb)
    take = rng.permutation(diff)[:diff.size // 2]
    bits = ab.copy()
    bits[take] = bb[take]
    x[:] = np.packbits(bits)
    return x


def tie_descriptors(rng, v, n):
    """descriptors equidistant to two siblings: at a random depth along a random path, the midpoint of the first two
    children of a node, then (when tied) kept only if that tie is for the smallest distance there"""
    rv = R.Vocab(v)
    desc = node_desc(v)
    out = []
    tries = 0
    while len(out) < n and tries < 50 * n:
        tries += 1
        node = 0
        while True:
            ch = rv.children[node]
            if len(ch) >= 2 and rng.random() < 0.5:
                break
            if not ch:
                break
            node = ch[int(rng.integers(0, len(ch)))]
        ch = rv.children[node]
        if len(ch) < 2:
            continue
        i, j = sorted(rng.choice(len(ch), 2, replace=False))
        x = midpoint(rng, desc[ch[i]], desc[ch[j]])
        # the tie must hold where x really descends: require x to pass through `node`
        cur = 0
        ok = True
        while cur != node and rv.children[cur]:
            cs = rv.children[cur]
            d = [R.forb_distance(bytes(x), desc[c]) for c in cs]
            cur = cs[int(np.argmin(d))]
            if not rv.children[cur] and cur != node:
                ok = False
        d = [R.forb_distance(bytes(x), desc[c]) for c in ch]
        if ok and cur == node and sorted(d)[0] == sorted(d)[1]:
            out.append(x)
    return np.array(out, np.uint8).reshape(-1, 32)


def tie_levels(v, feats):
    """per descriptor: the number of levels of its descent at which the smallest distance is shared, and its depth"""
    rv = R.Vocab(v)
    res = []
    for f in feats:
        node, t, depth = 0, 0, 0
        while rv.children[node]:
            ch = rv.children[node]
            d = [R.forb_distance(bytes(f), rv.desc[c]) for c in ch]
            m = min(d)
            t += d.count(m) > 1
            depth += 1
            node = ch[d.index(m)]
        res.append((t, depth))
    return np.array(res).reshape(-1, 2)


def near(rng, v, nodes, flip_log2=5):
    """descriptors near the given nodes (a few bits flipped)"""
    desc = node_desc(v)
    d = np.array([np.frombuffer(desc[n], np.uint8) for n in nodes], np.uint8).reshape(-1, 32)
    return bow._flip(rng, d, flip_log2) if d.size else d


def make_sets(rng, v, sizes, extra=()):
    """descriptor sets of the given sizes mixing centroids of every level, descriptors near leaves, descriptors tied
    between siblings and random ones; `extra` sets are appended as they are"""
    leaves = v.words["node_id"]
    all_nodes = v.nodes["node_id"]
    ties = tie_descriptors(rng, v, 64)
    out = []
    for n in sizes:
        if n == 0:
            out.append(np.zeros((0, 32), np.uint8))
            continue
        big = n > 256          # large sets: mostly centroids and ties, which the golden stores as indices
        parts = [near(rng, v, rng.choice(all_nodes, max(1, n // (2 if big else 8))), 30),   # centroids (no bit flipped)
                 ties[rng.integers(0, ties.shape[0], max(1, n // (4 if big else 8)))],
                 near(rng, v, rng.choice(leaves, max(1, n // (8 if big else 2)))),
                 rng.integers(0, 256, (n, 32), dtype=np.uint8)]
        s = np.concatenate(parts)[:n]
        out.append(s[rng.permutation(s.shape[0])])
    out.extend(np.asarray(e, np.uint8).reshape(-1, 32) for e in extra)
    return out


def record_vocab(out, name, rv, sets):
    """records + per-set reference outputs, checked against the restatement"""
    v = records(rv)
    p = "voc__" + name + "__"
    out[p + "head"] = np.array([v.k, v.L, v.scoring_type, v.weighting_type], np.int32)
    out[p + "node_id"], out[p + "parent_id"] = v.nodes["node_id"].astype(np.int32), v.nodes["parent_id"].astype(np.int32)
    out[p + "weight"], out[p + "desc"] = v.nodes["weight"].copy(), v.nodes["descriptor"].copy()
    out[p + "word_id"], out[p + "word_node"] = v.words["word_id"].astype(np.int32), v.words["node_id"].astype(np.int32)
    off = np.zeros(len(sets) + 1, np.int32)
    off[1:] = np.cumsum([s.shape[0] for s in sets])
    # the sets as indices into the node descriptors followed by a pool of the other distinct descriptors (sets hold
    # centroids, share descriptors and repeat them)
    alld = np.concatenate(sets) if sets else np.zeros((0, 32), np.uint8)
    at = {}
    for i, d in enumerate(v.nodes["descriptor"]):
        at.setdefault(d.tobytes(), i)
    pool = []
    idx = np.empty(alld.shape[0], np.int32)
    for i, d in enumerate(alld):
        b = d.tobytes()
        if b not in at:
            at[b] = v.nodes.shape[0] + len(pool)
            pool.append(d)
        idx[i] = at[b]
    out[p + "pool"] = np.array(pool, np.uint8).reshape(-1, 32)
    out[p + "sets_idx"] = idx
    out[p + "sets_off"] = off
    pv = R.Vocab(v)
    words, weights, bw, bv, boff, bows = [], [], [], [], [0], []
    for s in sets:
        w, wt, a, b = rv.transform(s)
        mine, per = pv.transform(s)
        assert [x[0] for x in per] == w.tolist() and bits_equal([x[1] for x in per], wt), name
        items = R.sorted_items(mine)
        assert [x[0] for x in items] == a.tolist() and bits_equal([x[1] for x in items], b), name
        words.append(w)
        weights.append(wt)
        bw.append(a)
        bv.append(b)
        boff.append(boff[-1] + a.size)
        bows.append((a, b, mine))
    out[p + "word"] = np.concatenate(words).astype(np.int32)
    out[p + "node_weight"] = np.concatenate(weights)
    out[p + "bow_word"], out[p + "bow_weight"] = np.concatenate(bw).astype(np.int32), np.concatenate(bv)
    out[p + "bow_off"] = np.array(boff, np.int32)
    S = len(sets)
    score = np.empty((S, S))
    for i in range(S):
        for j in range(S):
            score[i, j] = rv.score(bows[i][0], bows[i][1], bows[j][0], bows[j][1])
            assert bits_equal(score[i, j], R.l1_score(bows[i][2], bows[j][2])), (name, i, j)
    out[p + "score"] = score
    return v, bows


def keyframe_run(rng, vp, vl, n_kf, mode):
    """about 40 keyframes drawn around a few places; keyframe 0 and others dead along the way; one keyframe whose stereo
    point count differs from its descriptor rows; PL keyframes with n_pt = 0, n_ls = 0, both 0 and std_pt + std_ls == 0"""
    places = 6
    pool_p = [near(rng, vp, rng.choice(vp.words["node_id"], 60)) for _ in range(places)]
    pool_l = [near(rng, vl, rng.choice(vl.words["node_id"], 30)) for _ in range(places)]
    pd, ld, n_pt, n_ls, stdv = [], [], [], [], []
    alive = np.zeros((n_kf, n_kf), np.uint8)
    dead_from = {0: 1, 5: 9, 11: 12, 17: 30, 23: 24}            # keyframe -> first insert at which it is dead
    for k in range(n_kf):
        pl = int(rng.integers(0, places))
        a = pool_p[pl][rng.integers(0, 60, int(rng.integers(10, 90)))] if mode & 1 else np.zeros((0, 32), np.uint8)
        b = pool_l[pl][rng.integers(0, 30, int(rng.integers(4, 40)))] if mode & 2 else np.zeros((0, 32), np.uint8)
        if k == 7 and mode & 1:
            a = a[:0]                                           # no point descriptors at all
        pd.append(a)
        ld.append(b)
        npt, nls = a.shape[0], b.shape[0]
        if k == 4:
            npt = a.shape[0] + 13                               # stereo_pt count != pdesc_l.rows
        if k == 9:
            npt = 0
        if k == 13:
            nls = 0
        if k == 19:
            npt, nls = 0, 0                                     # n_pl = 0: 0 / 0
        n_pt.append(npt)
        n_ls.append(nls)
        s = rng.uniform(0, 120, 4)
        if k == 21:
            s[:] = 0.0                                          # std_pl = 0
        if k == 25:
            s = np.array([3.5, 1.25, -3.5, -1.25])              # std_pt + std_ls == 0 with both nonzero
        stdv.append(s)
        for i in range(k):
            alive[k, i] = not (i in dead_from and k >= dead_from[i])
    return pd, ld, np.array(n_pt, np.int32), np.array(n_ls, np.int32), np.array(stdv), alive


def record_run(out, name, mode, pname, lname, vocs, refs, rng, n_kf=40):
    vp = vocs[pname] if pname else vocs[lname]
    vl = vocs[lname] if lname else vocs[pname]
    pd, ld, n_pt, n_ls, stdv, alive = keyframe_run(rng, vp, vl, n_kf, mode)
    conf, conf32 = O.ref_bow_insert_run(mode, refs[pname] if pname else None, refs[lname] if lname else None, pd, ld, n_pt,
                                        n_ls, stdv, alive, SENTINEL)
    mine = R.MapBow(R.Vocab(vp) if mode & 1 else None, R.Vocab(vl) if mode & 2 else None, n_kf, fill=SENTINEL)
    for k in range(n_kf):
        mine.insert(k, pd[k], ld[k], alive[k, :k], R.run_stats(n_pt, n_ls, stdv, k))
    assert bits_equal(conf, np.array(mine.conf)), name
    assert bits_equal(conf32, conf.astype(np.float32)), name
    assert (conf == SENTINEL).any() and np.isnan(conf).any() == (mode == 3), name
    p = "run__" + name + "__"
    out[p + "mode"] = np.array([mode], np.int32)
    out[p + "voc_p"], out[p + "voc_l"] = np.array([pname]), np.array([lname])
    for key, xs in (("p", pd), ("l", ld)):
        off = np.zeros(n_kf + 1, np.int32)
        off[1:] = np.cumsum([x.shape[0] for x in xs])
        out[p + key + "_off"] = off
        pool, idx = np.unique(np.concatenate(xs), axis=0, return_inverse=True)     # keyframes repeat a place's descriptors
        out[p + key + "pool"], out[p + key + "idx"] = pool, idx.reshape(-1).astype(np.int32)
    out[p + "n_pt"], out[p + "n_ls"], out[p + "stdv"], out[p + "alive"] = n_pt, n_ls, stdv, alive
    out[p + "sentinel"] = np.array([SENTINEL])
    out[p + "conf"], out[p + "conf32"] = conf, conf32


def main():
    if O.ref_forb_from_string("1 2 3") is None:
        raise SystemExit("oracle/_ref lacks the DBoW2 wrapper: run `make -C oracle ref` with /root/reference present")
    rng = np.random.default_rng(20261015)
    out, vocs, refs = {}, {}, {}
    sizes = [0, 1, 63, 64, 65]

    # 1. TF_IDF, k = 10, L = 3, trained over 8 documents; 12 descriptors recur in every document (their words weigh log(1) = 0)
    common = rng.integers(0, 256, (12, 32), dtype=np.uint8)
    docs = [np.concatenate([rng.integers(0, 256, (260, 32), dtype=np.uint8), common]) for _ in range(8)]
    refs["tfidf_k10L3"] = O.ref_dbow_train(10, 3, R.TF_IDF, docs, 11)
    v = records(refs["tfidf_k10L3"])
    leaf = set(v.words["node_id"].tolist())
    zero = [n for n, w in zip(v.nodes["node_id"].tolist(), v.nodes["weight"].tolist()) if w == 0.0 and n in leaf]
    assert zero, "no naturally stopped word"
    stopped_only = [near(rng, v, zero[:3] * 5, 30)]                # every word stopped: an empty BowVector
    sets = make_sets(rng, v, sizes + [1025], extra=stopped_only + [common, docs[0][:100]])
    sets += [sets[len(sizes)][:1023], sets[len(sizes)][:1024]]     # 1023 and 1024: prefixes of the 1025 set
    vocs["tfidf_k10L3"], _ = record_vocab(out, "tfidf_k10L3", refs["tfidf_k10L3"], sets)

    # 2. TF, k = 8, L = 4, trained on 1240 descriptors (more than 1024 words): a level-4 group of children straddles
    #    STAGE_NODES in breadth-first order (the first training seed from 12 on whose tree has such a group)
    docs = [rng.integers(0, 256, (310, 32), dtype=np.uint8) for _ in range(4)]
    for seed in range(12, 40):
        refs["tf_k8L4"] = O.ref_dbow_train(8, 4, R.TF, docs, seed)
        v = records(refs["tf_k8L4"])
        pos, kids = bfs_positions(v)
        strad = [p for p, c in kids.items() if min(pos[x] for x in c) < STAGE_NODES <= max(pos[x] for x in c)]
        if strad:
            break
        refs["tf_k8L4"].close()
    assert strad, "no children group straddles STAGE_NODES"
    through = []
    for p in strad:
        for c in kids[p]:
            leaves = [c]
            while kids.get(leaves[0]):
                leaves = kids[leaves[0]]
            through += [c] * 4 + leaves
    big_set = np.concatenate([near(rng, v, rng.choice(v.words["node_id"], 1040, replace=False), 30),     # > 1024 words
                              np.repeat(near(rng, v, rng.choice(v.words["node_id"], 5)), 3069, axis=0)])[:BOW_MAX_SET]
    sets = make_sets(rng, v, sizes, extra=[near(rng, v, through, 6), near(rng, v, through, 30),
                                                    big_set[rng.permutation(big_set.shape[0])]])
    vocs["tf_k8L4"], _ = record_vocab(out, "tf_k8L4", refs["tf_k8L4"], sets)

    # 3. too few descriptors for k^L: nodes with fewer than k children, leaves at several depths (IDF)
    docs = [rng.integers(0, 256, (90, 32), dtype=np.uint8) for _ in range(3)]
    refs["idf_sparse"] = O.ref_dbow_train(10, 4, R.IDF, docs, 13)
    v = records(refs["idf_sparse"])
    pos, kids = bfs_positions(v)
    assert any(0 < len(c) < 10 for c in kids.values())
    sets = make_sets(rng, v, sizes, extra=[np.concatenate(docs)])
    vocs["idf_sparse"], _ = record_vocab(out, "idf_sparse", refs["idf_sparse"], sets)

    # 4. special leaf weights (-0.0, negative, NaN, +inf, subnormal, DBL_MAX) under all four weightings; and a tie copy:
    #    every parent's second child carries its first child's descriptor, so descents tie at every level
    docs = [rng.integers(0, 256, (120, 32), dtype=np.uint8) for _ in range(3)]
    base = O.ref_dbow_train(6, 3, R.TF_IDF, docs, 15)
    bv = records(base)
    base.close()
    leaves = bv.words["node_id"].tolist()
    for wname, wt in (("tfidf", R.TF_IDF), ("tf", R.TF), ("idf", R.IDF), ("binary", R.BINARY)):
        name = "special_" + wname
        refs[name] = ref_load(bv, wt)
        for i, leaf in enumerate(leaves):
            if i % 3 == 0:
                refs[name].set_weight(leaf, SPECIAL[(i // 3) % len(SPECIAL)])
        v = records(refs[name])
        wmap = dict(zip(v.nodes["node_id"].tolist(), v.nodes["weight"].tolist()))
        by = {}
        for leaf in leaves:
            by.setdefault(repr(wmap[leaf]), []).append(leaf)
        plain = [l for l in leaves if np.isfinite(wmap[l]) and wmap[l] > 1e-300 and wmap[l] < 1e300]
        spec = []
        for sv in SPECIAL:
            ls = by[repr(sv)]
            spec.append(near(rng, v, ls[:1] * 2 + plain[:3], 30))   # each special word twice (a TF fold) with plain words
        dmax = by[repr(SPECIAL[-1])]
        extra = spec + [near(rng, v, dmax[:2] * 2, 30),                   # DBL_MAX + DBL_MAX = inf: norm inf, NaN and 0
                        near(rng, v, by[repr(1e-310)][:1], 30),           # a subnormal alone: normalised to 1
                        near(rng, v, by[repr(SPECIAL[0])] + by[repr(SPECIAL[1])] + by["nan"], 30)]   # all stopped
        vocs[name], _ = record_vocab(out, name, refs[name], make_sets(rng, v, [65], extra=extra))
    tv = bow.Vocabulary(bv.k, bv.L, bv.scoring_type, bv.weighting_type, bv.nodes.copy(), bv.words.copy())
    pid = tv.nodes["parent_id"]
    starts = np.flatnonzero(np.r_[True, pid[1:] != pid[:-1]])
    for s in starts:
        if s + 1 < pid.size and pid[s + 1] == pid[s]:
            tv.nodes["descriptor"][s + 1] = tv.nodes["descriptor"][s]
    refs["ties"] = ref_load(tv)
    v = records(refs["ties"])
    sets = make_sets(rng, v, [64], extra=[near(rng, v, v.nodes["node_id"], 3), near(rng, v, v.nodes["node_id"], 30)])
    vocs["ties"], _ = record_vocab(out, "ties", refs["ties"], sets)
    tl = tie_levels(v, np.concatenate(sets))
    full = ((tl[:, 0] == tl[:, 1]) & (tl[:, 1] == bv.L)).sum()
    print("[bow golden] ties: %d descriptors tie at every level of a full-depth descent" % full)
    assert full > 0

    # ties on the trained vocabularies, for the record
    for name in ("tfidf_k10L3", "tf_k8L4"):
        t = tie_levels(vocs[name], golden_all_sets(out, name))[:, 0]
        assert (t > 0).sum() > 20, name
        print("[bow golden] %s: %d descriptors tie at some level, %d at two or more" % (name, (t > 0).sum(), (t > 1).sum()))

    # 5. keyframe runs through the cut insertKFBowVector{P,L,PL}
    record_run(out, "P", 1, "tfidf_k10L3", "", vocs, refs, rng)
    record_run(out, "L", 2, "", "idf_sparse", vocs, refs, rng)
    record_run(out, "PL", 3, "tf_k8L4", "special_idf", vocs, refs, rng)
    for r in refs.values():
        r.close()
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


def golden_all_sets(out, name):
    p = "voc__" + name + "__"
    return np.concatenate([out[p + "desc"], out[p + "pool"]])[out[p + "sets_idx"]]


if __name__ == "__main__":
    main()
