"""Builds and runs a C++ client of PlslamBow::train (plslam_amd/host/dbow_voc.hpp) on the GPU and compares what it exports with
the Python route (plslam_amd.bow_train) on the same documents, byte for byte."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import plslam_amd
from plslam_amd import bow, bow_train
from tests import bow_train_ref as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _compile(tmp):
    exe = os.path.join(tmp, "test_bow_train_shim")
    lib = os.path.dirname(plslam_amd.LIB_PATH)
    subprocess.run([shutil.which("g++") or "g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror",
                    os.path.join(ROOT, "tests", "cpp", "test_bow_train_shim.cpp"), "-I" + os.path.join(ROOT, "include"), "-L" + lib,
                    "-lplslam_hip", "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib", "-lamdhip64", "-o", exe],
                   check=True)
    return exe


@pytest.mark.gpu
@pytest.mark.parametrize("case", [(10, 3, bow.BOW_TF_IDF, 0, "uniform"), (3, 4, bow.BOW_BINARY, 2, "uniform"),
                                  (4, 3, bow.BOW_IDF, 0, "clustered")])
def test_shim_train_exports_what_the_python_route_exports(ctx, tmp_path, case):
    k, L, weighting, max_iters, kind = case
    rng = np.random.default_rng(40 + k)
    docs = T.uniform_docs(rng) if kind == "uniform" else T.clustered_docs(rng, 4, 150, 6, 15)
    docs.insert(2, docs[0][:0])                                     # an empty document in the middle
    seed = 2 ** 63 + 12345                                          # a seed beyond int64
    off = bow_train.doc_offsets(docs)
    fx, out = str(tmp_path / "train.bin"), str(tmp_path / "out.bin")
    with open(fx, "wb") as f:
        f.write(np.array([k, L, weighting, max_iters, len(docs)], np.int32).tobytes())
        f.write(np.array([seed], np.uint64).tobytes())
        f.write(off.tobytes())
        f.write(np.ascontiguousarray(np.concatenate(docs)).tobytes())
    res = subprocess.run([_compile(str(tmp_path)), fx, out], capture_output=True, text=True, timeout=300)
    print(res.stdout[-2000:], res.stderr[-2000:])
    assert res.returncode == 0 and "all checks passed" in res.stdout, res.stdout[-2000:]
    voc, stats = bow_train.train_vocabulary(ctx, docs, k, L, weighting, seed, max_iters or bow_train.DEFAULT_MAX_ITERS)
    raw = open(out, "rb").read()
    st = np.frombuffer(raw[:48], np.int64)
    assert st.tolist() == [stats[n] for n in ("n_nodes", "n_words", "lloyd_rounds", "lloyd_rounds_max", "empty_groups", "capped_nodes")]
    nb = voc.nodes.shape[0] * bow.BOW_NODE_DTYPE.itemsize
    assert raw[48:48 + nb] == voc.nodes.tobytes() and raw[48 + nb:] == voc.words.tobytes()
    if kind == "clustered":
        assert stats["empty_groups"] > 0
    if max_iters:
        assert stats["capped_nodes"] > 0
