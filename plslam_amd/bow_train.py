"""Training a DBoW2 vocabulary on the device (plslam_bow_train_*, include/plslam_bow_train.h): TemplatedVocabulary::create's
hierarchical k-means++ (3rdparty/DBoW2/include/DBoW2/TemplatedVocabulary.h:536-976), one whole tree level per pass.

``train_vocabulary(ctx, docs, k, L, weighting, seed)`` returns a ``bow.Vocabulary`` -- what ``bow.save_vocabulary`` writes and
``BowVocabulary(ctx, voc)`` uploads -- and the run's statistics.  ``BowTrainer`` is the handle underneath, with the
device-pointer form.

The prototypes of this header are kept in a registry of their own (TRAIN_PROTOTYPES) and applied to load()'s handle on first
use; ``plslam_amd`` does not import this module.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import bow
from ._lib import Handle, _arr, _check, _p, load

HEADER = "plslam_bow_train.h"
MAX_N, MAX_K, MAX_L, DEFAULT_MAX_ITERS = 1 << 24, 256, 16, 1000


class BowTrainParams(C.Structure):
    """plslam_bow_train_params"""
    _fields_ = [("k", C.c_int32), ("L", C.c_int32), ("weighting_type", C.c_int32), ("scoring_type", C.c_int32),
                ("seed", C.c_uint64), ("max_iters", C.c_int32), ("reserved", C.c_int32)]


class BowTrainStats(C.Structure):
    """plslam_bow_train_stats"""
    _fields_ = [("n_nodes", C.c_int32), ("n_words", C.c_int32), ("lloyd_rounds", C.c_int64), ("empty_groups", C.c_int64),
                ("capped_nodes", C.c_int64), ("lloyd_rounds_max", C.c_int32), ("levels", C.c_int32)]

    def as_dict(self):
        return {n: int(getattr(self, n)) for n, _ in self._fields_}


_vp, _i32 = C.c_void_p, C.c_int32
# name -> (argtypes, restype) of every entry point include/plslam_bow_train.h declares
TRAIN_PROTOTYPES = {
    "plslam_bow_train_create": ([_vp, C.POINTER(BowTrainParams), _vp, _vp, _i32, C.POINTER(_vp)], C.c_int),
    "plslam_bow_train_create_dev": ([_vp, C.POINTER(BowTrainParams), _vp, _vp, _i32, _i32, C.POINTER(_vp)], C.c_int),
    "plslam_bow_train_run": ([_vp, C.POINTER(BowTrainStats)], C.c_int),
    "plslam_bow_train_sizes": ([_vp, C.POINTER(_i32), C.POINTER(_i32)], C.c_int),
    "plslam_bow_train_export": ([_vp, _vp, _vp], C.c_int),
    "plslam_bow_train_download": ([_vp, _vp, _vp], C.c_int),
    "plslam_bow_train_destroy": ([_vp], None),
}
_applied = None


def _lib():
    """load()'s handle with this header's prototypes on it"""
    global _applied
    L = load()
    if _applied is not L:
        for name, (argtypes, restype) in TRAIN_PROTOTYPES.items():
            f = getattr(L, name)
            f.argtypes, f.restype = argtypes, restype
        _applied = L
    return L


def _params(k, L, weighting, seed, max_iters, scoring=bow.BOW_L1_NORM):
    return BowTrainParams(int(k), int(L), int(weighting), int(scoring), int(seed) & (2 ** 64 - 1), int(max_iters), 0)


class BowTrainer(Handle):
    """plslam_bow_trainer.  desc: (N, 32) uint8, offsets: n_docs + 1 int32 document offsets (host arrays, copied); or, with
    dev=True, two device addresses as ints with n_docs and n_total stated (the memory stays the caller's)."""

    def __init__(self, ctx, desc, offsets, k, L, weighting=bow.BOW_TF_IDF, seed=0, max_iters=DEFAULT_MAX_ITERS,
                 scoring=bow.BOW_L1_NORM, dev=False, n_docs=None, n_total=None):
        lib = _lib()
        prm = _params(k, L, weighting, seed, max_iters, scoring)
        self.k, self.L, self.weighting, self.scoring = int(k), int(L), int(weighting), int(scoring)
        h = C.c_void_p()
        if dev:
            self.n_total = int(n_total)
            _check(lib.plslam_bow_train_create_dev(ctx.handle, C.byref(prm), int(desc), int(offsets), int(n_docs), int(n_total),
                                                   C.byref(h)), "plslam_bow_train_create_dev")
        else:
            d = _arr(desc, np.uint8, (-1, 32))
            off = _arr(offsets, np.int32)
            self.n_total = d.shape[0]
            if off.shape[0] < 1 or int(off[-1]) != d.shape[0]:
                raise ValueError("the last document offset must be the number of descriptors")
            _check(lib.plslam_bow_train_create(ctx.handle, C.byref(prm), _p(d), _p(off), off.shape[0] - 1, C.byref(h)),
                   "plslam_bow_train_create")
        self._open(ctx, "plslam_bow_train_destroy", h)

    def run(self) -> dict:
        st = BowTrainStats()
        _check(self._L.plslam_bow_train_run(self._h, C.byref(st)), "plslam_bow_train_run")
        return st.as_dict()

    def sizes(self):
        n, w = C.c_int32(), C.c_int32()
        _check(self._L.plslam_bow_train_sizes(self._h, C.byref(n), C.byref(w)), "plslam_bow_train_sizes")
        return n.value, w.value

    def export(self) -> bow.Vocabulary:
        n, w = self.sizes()
        nodes, words = np.zeros(n, bow.BOW_NODE_DTYPE), np.zeros(w, bow.BOW_WORD_DTYPE)
        _check(self._L.plslam_bow_train_export(self._h, _p(nodes), _p(words)), "plslam_bow_train_export")
        return bow.Vocabulary(self.k, self.L, self.scoring, self.weighting, nodes, words)

    def download(self):
        """-> (leaf node id of the training partition, word of the descent), per training descriptor"""
        leaf, word = np.empty(self.n_total, np.int32), np.empty(self.n_total, np.int32)
        _check(self._L.plslam_bow_train_download(self._h, _p(leaf), _p(word)), "plslam_bow_train_download")
        return leaf, word


def doc_offsets(docs):
    off = np.zeros(len(docs) + 1, np.int32)
    off[1:] = np.cumsum([np.asarray(d).reshape(-1, 32).shape[0] for d in docs])
    return off


def train_vocabulary(ctx, docs, k, L, weighting=bow.BOW_TF_IDF, seed=0, max_iters=DEFAULT_MAX_ITERS):
    """docs: a list of (n_i, 32) uint8 arrays (empty ones count as documents) -> (bow.Vocabulary, stats dict)"""
    parts = [np.asarray(d, np.uint8).reshape(-1, 32) for d in docs]
    desc = np.concatenate(parts) if parts else np.zeros((0, 32), np.uint8)
    t = BowTrainer(ctx, desc, doc_offsets(parts), k, L, weighting, seed, max_iters)
    try:
        stats = t.run()
        return t.export(), stats
    finally:
        t.close()
