"""Generates tests/golden/bow_train_golden.npz.  Run from the repo root where oracle/_ref carries the DBoW2 wrapper:
    python tests/golden/make_bow_train_golden.py

Outputs of the REFERENCE'S OWN TemplatedVocabulary::create (3rdparty/DBoW2, compiled into oracle/_ref by
oracle/ref_wrap_dbow.cpp) after DUtils::Random::SeedRand(seed): per case the documents, k, L, the weighting, the seed, and the
records create() left (ascending node id; weights as uint64).  Deterministic.  A case is handed to the reference only if the
restatement (tests/bow_train_ref.py with LibcDraws) reports no empty group and no capped node on it, and the file is written
only if the restatement reproduces every reference output bit for bit.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from oracle import oracle as O  # noqa: E402
from tests import bow_train_ref as T  # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "bow_train_golden.npz")
CASES = [("uniform_k10_L4_tfidf", "uniform", 10, 4, T.TF_IDF, 21), ("uniform_k3_L2_idf", "uniform", 3, 2, T.IDF, 22),
         ("uniform_k2_L1_tf", "uniform", 2, 1, T.TF, 23), ("duplicates_k10_L2_idf", "duplicates", 10, 2, T.IDF, 24),
         ("duplicates_k3_L4_binary", "duplicates", 3, 4, T.BINARY, 25)]


def main():
    assert O.ref_lib() is not None and hasattr(O.ref_lib(), "ref_dbow_train"), "oracle/_ref lacks the DBoW2 wrapper"
    out = {"cases": np.array([c[0] for c in CASES])}
    for name, kind, k, L, weighting, seed in CASES:
        rng = np.random.default_rng(seed)
        docs = T.uniform_docs(rng, 4, 30, 120) if kind == "uniform" else T.duplicate_docs(rng)
        mine = T.train(docs, k, L, weighting, T.LibcDraws(seed))
        assert mine["stats"]["empty_groups"] == 0 and mine["stats"]["capped_nodes"] == 0, name
        nodes, words = T.reference_records(O, docs, k, L, weighting, seed)
        assert T.same_records(mine["nodes"], mine["words"], nodes, words), name
        off = np.zeros(len(docs) + 1, np.int32)
        off[1:] = np.cumsum([len(d) for d in docs])
        out.update({f"{name}__desc": np.concatenate(docs), f"{name}__off": off,
                    f"{name}__params": np.array([k, L, weighting, seed], np.int64), f"{name}__node_id": nodes["node_id"],
                    f"{name}__parent_id": nodes["parent_id"], f"{name}__weight_bits": nodes["weight"].view(np.uint64),
                    f"{name}__descriptor": nodes["descriptor"], f"{name}__word_id": words["word_id"],
                    f"{name}__word_node": words["node_id"]})
        print(name, mine["stats"])
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
