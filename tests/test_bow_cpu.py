"""CPU tests of the bag-of-words layer: the restatement (tests/dbow_ref.py) against the reference's own FORB::distance, the
vocabulary file loader, the synthetic vocabularies, and the C++ shim compiling against the C ABI."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import plslam_amd
from plslam_amd import bow
from tests import dbow_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_restated_distance_is_the_references_forb_distance(oracle):
    ref = oracle.ref_lib()
    if ref is None:
        pytest.skip("oracle/_ref was not built (no reference tree on this machine)")
    rng = np.random.default_rng(3)
    a = rng.integers(0, 256, (500, 32), dtype=np.uint8)
    b = rng.integers(0, 256, (500, 32), dtype=np.uint8)
    b[:50] = a[:50]
    b[50:100] = ~a[50:100]
    for x, y in zip(a, b):
        assert R.forb_distance(bytes(x), bytes(y)) == ref.ref_forb_distance(x.ctypes.data, y.ctypes.data)


def _same_vocab(a, b):
    assert (a.k, a.L, a.scoring_type, a.weighting_type) == (b.k, b.L, b.scoring_type, b.weighting_type)
    assert np.array_equal(a.nodes["node_id"], b.nodes["node_id"]) and np.array_equal(a.nodes["parent_id"], b.nodes["parent_id"])
    assert np.array_equal(a.nodes["weight"].view(np.uint64), b.nodes["weight"].view(np.uint64))
    assert np.array_equal(a.nodes["descriptor"], b.nodes["descriptor"]) and np.array_equal(a.words, b.words)


@pytest.mark.parametrize("suffix", [".yml", ".yml.gz"])
def test_vocabulary_file_round_trip(tmp_path, suffix):
    v = bow.synth_vocabulary(np.random.default_rng(1), k=5, L=3, weighting=R.IDF, irregular=True, shuffle_ids=True,
                             permute_words=True, stop_frac=0.2)
    v.nodes["weight"][::7] = np.random.default_rng(2).normal(0, 1e-300, v.nodes.shape[0])[::7]   # subnormal-ish values round trip
    p = str(tmp_path / ("voc" + suffix))
    bow.save_vocabulary(p, v)
    _same_vocab(bow.load_vocabulary(p), v)


def test_loader_reads_the_opencv_yaml_layout(tmp_path):
    """The layout cv::FileStorage gives TemplatedVocabulary::save (:1340-1435): flow maps, weights as OpenCV prints them."""
    d = " ".join(str(i) for i in range(32)) + " "
    text = ("%YAML:1.0\n---\nvocabulary:\n   k: 2\n   L: 2\n   scoringType: 0\n   weightingType: 0\n   nodes:\n"
            f"      - {{ nodeId:2, parentId:0, weight:0., descriptor:\"{d}\" }}\n"
            f"      - {{ nodeId:1, parentId:0, weight:1.5000000000000000e+00,\n          descriptor:\"{d}\" }}\n"
            f"      - {{ nodeId:3, parentId:2, weight:.Inf, descriptor:\"{d}\" }}\n"
            "   words:\n      - { wordId:0, nodeId:1 }\n      - { wordId:1, nodeId:3 }\n")
    p = tmp_path / "v.yml"
    p.write_text(text)
    v = bow.load_vocabulary(str(p))
    assert (v.k, v.L, v.scoring_type, v.weighting_type) == (2, 2, 0, 0)
    assert list(v.nodes["node_id"]) == [2, 1, 3] and list(v.nodes["parent_id"]) == [0, 0, 2]
    assert v.nodes["weight"][1] == 1.5 and np.isinf(v.nodes["weight"][2])
    assert list(v.nodes["descriptor"][0]) == list(range(32))
    assert [tuple(w) for w in v.words] == [(0, 1), (1, 3)]


def _children(v):
    ch = {}
    for r in v.nodes:
        ch.setdefault(int(r["parent_id"]), []).append(int(r["node_id"]))
    return ch


def test_synthetic_vocabulary_full_size():
    v = bow.synth_vocabulary(np.random.default_rng(0), k=10, L=6)
    assert v.nodes.shape[0] == sum(10 ** i for i in range(1, 7)) and v.words.shape[0] == 10 ** 6
    assert np.array_equal(np.sort(v.nodes["node_id"]), np.arange(1, v.nodes.shape[0] + 1))
    assert np.array_equal(v.words["word_id"], np.arange(10 ** 6))
    # save()'s order: the children of a parent are consecutive records
    pid = v.nodes["parent_id"]
    assert np.count_nonzero(pid[1:] != pid[:-1]) + 1 == len(np.unique(pid))


def test_synthetic_vocabulary_irregular_properties():
    v = bow.synth_vocabulary(np.random.default_rng(4), k=6, L=5, irregular=True, shuffle_ids=True, permute_words=True,
                             stop_frac=0.3)
    ch = _children(v)
    assert all(1 <= len(c) <= 6 for c in ch.values())
    leaves = set(v.nodes["node_id"].tolist()) - set(ch)
    assert set(v.words["node_id"].tolist()) == leaves
    depth = {0: 0}
    for r in v.nodes:                                             # parents precede their children in save()'s order
        depth[int(r["node_id"])] = depth[int(r["parent_id"])] + 1
    assert len({depth[n] for n in leaves}) > 1                    # leaves at several depths
    assert any(c != sorted(c) for c in ch.values())               # children-list order differs from id order
    w = dict(zip(v.nodes["node_id"].tolist(), v.nodes["weight"].tolist()))
    stopped = sum(w[n] == 0.0 for n in leaves)
    assert 0 < stopped < len(leaves)
    assert sorted(v.words["word_id"].tolist()) == list(range(len(leaves)))


def test_restatement_basics():
    v = bow.synth_vocabulary(np.random.default_rng(5), k=4, L=3)
    rv = R.Vocab(v)
    d = bow.near_leaf_descriptors(np.random.default_rng(6), v, 40)
    bv, per = rv.transform(d)
    assert len(per) == 40 and 0 < len(bv) <= 40
    assert abs(sum(bv.values()) - 1.0) < 1e-12
    assert R.l1_score(bv, bv) == pytest.approx(1.0) and R.l1_score({}, bv) == 0.0
    assert np.signbit(R.l1_score({}, bv))                         # -0.0 / 2.0
    assert np.isnan(R.pl_combine(0.5, 0.5, 0, 0, 1.0, 1.0))       # 0/0 -> NaN, as IEEE gives it


def test_bow_shim_compiles_against_the_abi(tmp_path):
    """CPU: plslam_amd/host/dbow_voc.hpp and the shim test compile and link against the C-ABI library (no device needed)."""
    exe = str(tmp_path / "test_bow_shim")
    subprocess.run([shutil.which("g++") or "g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror",
                    os.path.join(ROOT, "tests", "cpp", "test_bow_shim.cpp"), "-I" + os.path.join(ROOT, "include"),
                    "-L" + os.path.dirname(plslam_amd.LIB_PATH), "-lplslam_hip", "-Wl,-rpath," + os.path.dirname(plslam_amd.LIB_PATH),
                    "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib", "-lamdhip64", "-o", exe], check=True)
