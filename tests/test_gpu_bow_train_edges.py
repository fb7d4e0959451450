"""GPU tests of the vocabulary training (plslam_bow_train_*, bow_train.hip K111-K129) off uniform bytes, k <= 10 and L <= 4: the
named cases of tests/bow_train_cases.py -- deep trees (L = 8, 13, 16), wide nodes (k = 64, 65, 256), distances of 256 and
low-entropy rows, the edges of the draws, hundreds of documents, 65536 words and more, more than 1024 scan tiles -- against the
restatement with the counter draws (tests/bow_train_ref.py), and the trainer's life cycle and refusals.  Every comparison is
test_gpu_bow_train.py's _assert_same: records, weights as uint64, statistics, the partition and the words, all exact.
tests/test_bow_train_cases_cpu.py shows without a GPU that each case reaches the branch it is named for.

Left out on purpose: a distance prefix sum beyond int32 needs more than 8.4 million adversarial rows (2^31 / 256 bits each),
which no test of seconds reaches."""
import ctypes as C_

import numpy as np
import pytest

from plslam_amd import bow, bow_train
from plslam_amd._lib import _p
from plslam_amd.capi import EINVAL, ERANGE, PlslamError
from tests import bow_train_cases as C
from tests import bow_train_ref as T
from tests.test_gpu_bow_train import _assert_same, _train

pytestmark = pytest.mark.gpu


def _same(ctx, name):
    _assert_same(_train(ctx, *C.case(name)), C.expect(name)[0], name)


@pytest.mark.parametrize("name", C.GROUPS["deep"])
def test_deep_trees(ctx, name):
    """levels with more than 1024 visited and more than 256 running nodes, waves of ten and more groups, a tree that ends
    before L = 16"""
    _same(ctx, name)


@pytest.mark.parametrize("name", C.GROUPS["wide"])
def test_wide_nodes(ctx, name):
    """k = 64, 65, 256: as many clusters as lanes and more, 255 seeding rounds on the root"""
    _same(ctx, name)


@pytest.mark.parametrize("name", C.GROUPS["far_tied"])
def test_distances_of_256_and_low_entropy_rows(ctx, name):
    _same(ctx, name)


@pytest.mark.parametrize("name", C.GROUPS["draws"])
def test_edges_of_the_draws(ctx, name):
    """a cut of 0.0 drawn again on the device, a cut equal to the distance sum, the first centre on row n - 1 and row 0; three of
    the seeds are 2^63 and more"""
    _same(ctx, name)


@pytest.mark.parametrize("name", C.GROUPS["documents"])
def test_hundreds_of_documents_and_more_documents_than_rows(ctx, name):
    _same(ctx, name)


@pytest.mark.parametrize("name", C.GROUPS["scale"])
def test_scale(ctx, name):
    """65536 words and more behind the word sort; more than 1024 tiles under the prefix sum"""
    _same(ctx, name)


# ---- life cycle ------------------------------------------------------------------------------------------------------------
def _trainer(ctx, name, max_iters=None):
    docs, k, L, weighting, seed, mi = C.case(name)
    parts = [np.asarray(d, np.uint8).reshape(-1, 32) for d in docs]
    return bow_train.BowTrainer(ctx, np.concatenate(parts), bow_train.doc_offsets(parts), k, L, weighting, seed,
                                mi if max_iters is None else max_iters)


def _result(t, stats):
    return (t.export(), stats) + t.download()


def test_run_twice_on_one_trainer(ctx):
    name = "documents_499_cuts_tfidf"
    t = _trainer(ctx, name)
    a = _result(t, t.run())
    b = _result(t, t.run())
    t.close()
    _assert_same(a, C.expect(name)[0], "the first run")
    _assert_same(b, C.expect(name)[0], "the second run")
    assert a[0].nodes.tobytes() == b[0].nodes.tobytes() and a[0].words.tobytes() == b[0].words.tobytes() and a[1] == b[1]


def test_two_trainers_alive_on_one_context(ctx):
    """A and B created, B run, A run, then both exported: each is what a lone trainer gives"""
    na, nb = "alternating_flipped", "low_entropy_k10_L3"
    ta, tb = _trainer(ctx, na), _trainer(ctx, nb)
    sb = tb.run()
    sa = ta.run()
    a, b = _result(ta, sa), _result(tb, sb)
    ta.close()
    _assert_same(b, C.expect(nb)[0], "B, after A was closed")
    tb.close()
    _assert_same(a, C.expect(na)[0], "A")


def test_max_iters_zero_is_the_default_of_1000(ctx):
    name = "deep_k3_L8_tfidf"
    assert C.case(name)[5] == bow_train.DEFAULT_MAX_ITERS == 1000
    t = _trainer(ctx, name, max_iters=0)
    got = _result(t, t.run())
    t.close()
    _assert_same(got, C.expect(name)[0], "max_iters = 0")


# ---- refusals --------------------------------------------------------------------------------------------------------------
def _still_trains(ctx):
    _same(ctx, "draw_first_is_row_0")


def _code(call):
    with pytest.raises(PlslamError) as e:
        call()
    return e.value.code


def test_sizes_export_and_download_before_run_are_refused(ctx):
    t = _trainer(ctx, "draw_first_is_row_0")
    L = t._L
    n, w = C_.c_int32(-7), C_.c_int32(-7)
    nodes, words = np.zeros(64, bow.BOW_NODE_DTYPE), np.zeros(64, bow.BOW_WORD_DTYPE)
    leaf, word = np.full(300, -7, np.int32), np.full(300, -7, np.int32)
    assert L.plslam_bow_train_sizes(t.handle, C_.byref(n), C_.byref(w)) == EINVAL and (n.value, w.value) == (-7, -7)
    assert L.plslam_bow_train_export(t.handle, _p(nodes), _p(words)) == EINVAL and not nodes.tobytes().strip(b"\0")
    assert L.plslam_bow_train_download(t.handle, _p(leaf), _p(word)) == EINVAL and (leaf == -7).all() and (word == -7).all()
    # the wrappers raise on it too.  (export() asks sizes() first, so its line shows the refusal of sizes again: the entry
    # points plslam_bow_train_export and _download themselves are the raw calls above)
    assert _code(t.sizes) == EINVAL and _code(t.export) == EINVAL and _code(t.download) == EINVAL
    got = _result(t, t.run())                                      # the refused trainer itself still trains
    t.close()
    _assert_same(got, C.expect("draw_first_is_row_0")[0])
    _still_trains(ctx)


def test_k_and_L_beyond_the_headers_limits_are_refused(ctx):
    d = np.zeros((4, 32), np.uint8)
    assert (bow_train.MAX_K, bow_train.MAX_L) == (256, 16)
    assert _code(lambda: bow_train.BowTrainer(ctx, d, [0, 4], 257, 2)) == ERANGE
    _still_trains(ctx)
    assert _code(lambda: bow_train.BowTrainer(ctx, d, [0, 4], 2, 17)) == ERANGE
    _still_trains(ctx)


def test_the_device_pointer_form_refuses_a_misaligned_block_and_too_many_rows(ctx):
    """desc + 8 is not 16-byte aligned: EINVAL; n_total = MAX_N + 1: ERANGE, checked before anything is reserved"""
    import torch
    dd = torch.zeros(64 * 32 + 64, dtype=torch.uint8, device="cuda")
    doff = torch.tensor([0, 64], dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    assert dd.data_ptr() % 16 == 0
    mk = lambda p, n: bow_train.BowTrainer(ctx, p, doff.data_ptr(), 3, 2, T.IDF, 1, dev=True, n_docs=1, n_total=n)
    assert _code(lambda: mk(dd.data_ptr() + 8, 64)) == EINVAL
    _still_trains(ctx)
    assert _code(lambda: mk(dd.data_ptr(), bow_train.MAX_N + 1)) == ERANGE
    _still_trains(ctx)
    t = mk(dd.data_ptr(), 64)                                      # the same block, aligned and of its true size, is taken
    assert t.run()["n_words"] == 1                                 # 64 equal rows: one centre, one word
    t.close()
