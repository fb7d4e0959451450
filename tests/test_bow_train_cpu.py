"""The vocabulary training without a GPU: the restatement (tests/bow_train_ref.py) against the reference's own
TemplatedVocabulary::create -- live where oracle/_ref carries the DBoW2 wrapper, and against its recorded outputs
(tests/golden/bow_train_golden.npz) everywhere --, the draw function of plslam_amd/csrc/bow_train_draw.h against its Python
statement, the pure host planner as a stand-alone program (plain and under the sanitizers; nothing is loaded into Python), and
include/plslam_bow_train.h held to what tests/test_abi.py asks of include/plslam_hip.h.  Every comparison is exact."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import plslam_amd
from plslam_amd import bow_train
from tests import bow_train_ref as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "bow_train_golden.npz")
INC = ["-I" + os.path.join(ROOT, "plslam_amd", "csrc"), "-I" + os.path.join(ROOT, "include")]


# ---- the restatement against the reference -------------------------------------------------------------------------------
def _ref(oracle):
    if oracle.ref_lib() is None or not hasattr(oracle.ref_lib(), "ref_dbow_train"):
        pytest.skip("oracle/_ref was not built with the DBoW2 wrapper (no reference tree on this machine)")
    return oracle


def _against_the_reference(O, make_docs, k, L, weighting, seed0):
    """The restatement first: an input on which it sees an empty group or a capped node is replaced by another seed and never
    reaches the reference (which would read a released matrix and take the process down)."""
    found = T.clean_input(make_docs, k, L, weighting, seed0)
    if found is None:
        pytest.fail("no input without an empty group in 8 seeds")
    docs, seed, mine = found
    assert mine["stats"]["empty_groups"] == 0 and mine["stats"]["capped_nodes"] == 0
    nodes, words = T.reference_records(O, docs, k, L, weighting, seed)
    assert T.same_records(mine["nodes"], mine["words"], nodes, words), (k, L, weighting, seed)
    return mine


@pytest.mark.parametrize("weighting", T.WEIGHTINGS)
@pytest.mark.parametrize("L", T.UNIFORM_L)
@pytest.mark.parametrize("k", T.UNIFORM_K)
def test_restatement_is_the_references_create_on_uniform_documents(oracle, k, L, weighting):
    """five documents of 50-400 uniform random descriptors, docs[0][:20] appended to each; records and weights as uint64"""
    _against_the_reference(_ref(oracle), T.uniform_docs, k, L, weighting, T.uniform_seed0(k, L, weighting))


@pytest.mark.parametrize("weighting", T.WEIGHTINGS)
@pytest.mark.parametrize("k,L", T.DUPLICATE_KL)
def test_restatement_is_the_references_create_on_heavy_duplicates(oracle, k, L, weighting):
    """30 distinct descriptors repeated up to 12 times: nodes with fewer distinct rows than k stop seeding early (dist_sum == 0),
    and trivial nodes hold duplicates, where the descent's word is not the training partition's leaf"""
    mine = _against_the_reference(_ref(oracle), T.duplicate_docs, k, L, weighting, T.duplicate_seed0(k, L, weighting))
    leaf_word = {int(n): int(w) for w, n in zip(mine["words"]["word_id"], mine["words"]["node_id"])}
    if k == 10:
        assert any(leaf_word[int(l)] != int(w) for l, w in zip(mine["leaf"], mine["word"]))     # the two do differ here


def test_restatement_reproduces_the_recorded_reference_outputs():
    g = np.load(GOLDEN)
    assert len(g["cases"]) >= 3
    for name in g["cases"].tolist():
        k, L, weighting, seed = (int(x) for x in g[f"{name}__params"])
        off = g[f"{name}__off"]
        docs = [g[f"{name}__desc"][a:b] for a, b in zip(off[:-1], off[1:])]
        mine = T.train(docs, k, L, weighting, T.LibcDraws(seed))
        assert mine["stats"]["empty_groups"] == 0 and mine["stats"]["capped_nodes"] == 0
        for f, key in (("node_id", "node_id"), ("parent_id", "parent_id"), ("descriptor", "descriptor")):
            assert np.array_equal(mine["nodes"][f], g[f"{name}__{key}"]), (name, f)
        assert np.array_equal(mine["nodes"]["weight"].view(np.uint64), g[f"{name}__weight_bits"]), name
        assert np.array_equal(mine["words"]["word_id"], g[f"{name}__word_id"]), name
        assert np.array_equal(mine["words"]["node_id"], g[f"{name}__word_node"]), name


def test_departures_are_counted_by_the_restatement():
    """clustered inputs run groups empty; max_iters 1 and 2 cap nodes; the counter draws do not depend on the walk's order"""
    rs, k, L, weighting, seed = T.DEPARTURE_CLUSTERED
    docs = T.clustered_docs(np.random.default_rng(rs), 4, 150, 6, 15)
    a = T.train(docs, k, L, weighting, T.CounterDraws(seed))
    assert a["stats"]["empty_groups"] > 0 and a["stats"]["capped_nodes"] == 0
    rs, ck, cL, cw, cseed, caps = T.DEPARTURE_CAPPED
    u = T.uniform_docs(np.random.default_rng(rs))
    for cap in caps:
        s = T.train(u, ck, cL, cw, T.CounterDraws(cseed), cap)["stats"]
        assert s["capped_nodes"] > 0 and s["rounds_max"] == cap
    b = T.train(docs, k, L, weighting, T.CounterDraws(seed))
    assert a["nodes"].tobytes() == b["nodes"].tobytes() and a["stats"] == b["stats"]


# ---- the draw function -----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def plan_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("bow_train_plan") / "test_bow_train_plan")
    subprocess.run([shutil.which("g++") or "g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror",
                    os.path.join(ROOT, "tests", "cpp", "test_bow_train_plan.cpp")] + INC + ["-o", exe], check=True)
    return exe


def test_header_draw_function_equals_the_python_statement(plan_exe):
    rng = np.random.default_rng(7)
    tuples = []
    for i in range(1000):
        seed = int(rng.integers(0, 2 ** 64, dtype=np.uint64)) if i % 3 else i
        path = [int(c) for c in rng.integers(0, 256, int(rng.integers(0, 7)))]
        tuples.append((seed, path, int(rng.integers(0, 256)), int(rng.integers(0, 5)) if i % 5 else int(rng.integers(0, 2 ** 32))))
    text = "".join(f"{s} {len(p)} {' '.join(map(str, p))} {j} {t}\n" for s, p, j, t in tuples)
    out = subprocess.run([plan_exe, "draws"], input=text, capture_output=True, text=True, check=True).stdout.split()
    assert len(out) == 2000
    for i, (seed, path, j, t) in enumerate(tuples):
        key = T.root_key(seed)
        for c in path:
            key = T.child_key(key, c)
        assert (int(out[2 * i]), int(out[2 * i + 1])) == (key, T.counter_draw(key, j, t)), (seed, path, j, t)


def test_draw_function_known_answers():
    assert T.mix64(0) == 0 and T.mix64(1) == 0x5692161D100B05E5          # the splitmix64 finaliser
    assert T.root_key(0) == 0 and T.child_key(0, 0) == T.mix64(1) and T.child_key(5, 2) == T.mix64(8)
    assert T.counter_draw(0, 0, 0) == T.mix64(0x9E3779B97F4A7C15) >> 33 == 1896895516
    assert T.root_key(7) == 1346066267577507604 and T.counter_draw(T.root_key(7), 3, 2) == 973660000
    key = T.root_key(12345)
    for c in (1, 0, 9):
        key = T.child_key(key, c)
    assert key == 13748142955388267063 and T.counter_draw(key, 4, 1) == 1760500959
    assert all(0 <= T.counter_draw(k, j, 0) < 2 ** 31 for k in range(50) for j in range(4))


def test_a_zero_cut_is_drawn_again():
    """the reference's do { cut_d = RandomValue(0, dist_sum); } while(cut_d == 0.0): an injected draw of 0 takes retry t = 1"""
    class ZeroFirst(T.Draws):
        asked = []

        def r(self, key, j, t):
            self.asked.append((j, t))
            return 0 if t == 0 else 1073741823

    d = ZeroFirst()
    assert d.cut(9, 2, 100.0) == (1073741823 / 2147483647.0) * 100.0 and d.asked == [(2, 0), (2, 1)]
    assert T.CounterDraws(0).first(T.root_key(3), 1) == 0


# ---- the planner, as a program ---------------------------------------------------------------------------------------------
HAND = ["check_refusals_in_the_headers_order", "check_offsets_first_nonzero_decreasing_empty_documents_and_n_zero",
        "check_dev_form_takes_n_total_and_the_alignment_and_the_largest_n", "sizes_of_a_million_rows_k_10_L_5",
        "carving_slices_on_256_bytes_in_order_and_disjoint", "geometry_blocks_tiles_and_waves",
        "tree_levels_visited_nodes_rows_slots_and_statistics", "renumbering_is_dbow2s_creation_order",
        "export_ascending_ids_parents_words_over_the_leaves_and_weights", "a_single_row_is_the_roots_one_child",
        "path_keys_and_draws_known_answers"]
SANITIZE = ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]


def _hand(exe):
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    res = {}
    for line in r.stdout.splitlines():
        if line.startswith(("PASS ", "FAIL ")):
            res[line.split(" ", 1)[1].split(":")[0]] = line
    return res, r.returncode, r.stderr


@pytest.mark.parametrize("case", HAND)
def test_bow_train_plan_hand_case(plan_exe, case):
    res = _hand(plan_exe)[0]
    assert case in res and res[case].startswith("PASS "), res.get(case, f"{case}: the driver did not run it")


def test_bow_train_plan_driver_ran_exactly_the_listed_cases(plan_exe):
    res, rc, _ = _hand(plan_exe)
    assert sorted(res) == sorted(HAND) and rc == 0


def test_bow_train_plan_clean_under_sanitizers(tmp_path):
    exe = str(tmp_path / "test_bow_train_plan_san")
    subprocess.run([shutil.which("g++") or "g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror"] + SANITIZE +
                   [os.path.join(ROOT, "tests", "cpp", "test_bow_train_plan.cpp")] + INC + ["-o", exe], check=True)
    res, rc, err = _hand(exe)
    assert rc == 0 and not err.strip(), err[-3000:]
    assert sorted(res) == sorted(HAND) and all(v.startswith("PASS ") for v in res.values())


def test_planner_headers_need_no_hip():
    csrc = os.path.join(ROOT, "plslam_amd", "csrc")
    for path in (os.path.join(csrc, "bow_train_plan.hpp"), os.path.join(csrc, "bow_train_draw.h"),
                 os.path.join(ROOT, "include", "plslam_bow_train.h")):
        with open(path) as f:
            inc = [l.split()[1].strip('<>"') for l in f if l.startswith("#include")]
        assert not [i for i in inc if i.startswith("hip/") or i == "common.hpp"], (path, inc)


# ---- include/plslam_bow_train.h to the standard of include/plslam_hip.h -----------------------------------------------------
def _header_symbols():
    src = open(os.path.join(ROOT, "include", "plslam_bow_train.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(plslam_[a-z0-9_]+)\s*\(", src)))


def test_train_header_symbols_all_exported_and_declared_exactly_once():
    syms = _header_symbols()
    assert len(syms) == 8 - 1 and "plslam_bow_train_run" in syms and "plslam_bow_train_create_dev" in syms
    lib = ctypes.CDLL(plslam_amd.LIB_PATH)
    assert not [s for s in syms if not hasattr(lib, s)]
    assert sorted(bow_train.TRAIN_PROTOTYPES) == syms                   # nothing missing, nothing extra
    from plslam_amd import _lib
    assert not set(syms) & set(_lib.PROTOTYPES) and not set(syms) & set(_lib.HEADER_PROTOTYPES)
    src = open(os.path.join(ROOT, "plslam_amd", "bow_train.py")).read()
    for s in syms:
        assert len(re.findall(r'"%s"\s*:' % s, src)) == 1, s
    L = bow_train._lib()
    for name, (argtypes, restype) in bow_train.TRAIN_PROTOTYPES.items():
        f = getattr(L, name)
        assert list(f.argtypes) == list(argtypes) and f.restype is restype, name


def test_train_header_is_plain_c(tmp_path):
    src = tmp_path / "abi.c"
    src.write_text('#include "plslam_bow_train.h"\nint main(void) { return (int)sizeof(plslam_bow_train_params) - 32; }\n')
    for cmd in (["gcc", "-std=c99"], ["g++", "-std=c++11", "-x", "c++"]):
        r = subprocess.run(cmd + ["-Wall", "-Wextra", "-pedantic", "-Werror", "-I" + os.path.join(ROOT, "include"), "-fsyntax-only",
                                  str(src)], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]


def test_train_structs_have_the_header_layout(tmp_path):
    """sizeof and every offsetof of the two records, from a C program, against the ctypes structures"""
    fields = {"plslam_bow_train_params": bow_train.BowTrainParams, "plslam_bow_train_stats": bow_train.BowTrainStats}
    body = "".join(f'printf("{s} %zu\\n", sizeof({s}));\n' + "".join(f'printf("{s}.{n} %zu\\n", offsetof({s}, {n}));\n' for n, _ in c._fields_)
                   for s, c in fields.items())
    src = tmp_path / "lay.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "plslam_bow_train.h"\nint main(void) {\n' + body + "return 0; }\n")
    exe = str(tmp_path / "lay")
    subprocess.run(["gcc", "-std=c99", "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe], check=True)
    got = dict(ln.split() for ln in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.splitlines())
    for s, c in fields.items():
        assert int(got[s]) == ctypes.sizeof(c)
        for n, _ in c._fields_:
            assert int(got[f"{s}.{n}"]) == getattr(c, n).offset, (s, n)
    assert ctypes.sizeof(bow_train.BowTrainParams) == 32 and ctypes.sizeof(bow_train.BowTrainStats) == 40


def test_the_training_source_is_built_and_the_first_headers_surface_is_untouched():
    from plslam_amd import build as B
    assert "bow_train.hip" in B.SOURCES
    for h in ("bow_train_plan.hpp", "bow_train_draw.h", "plslam_bow_train.h"):
        assert any(p.endswith(os.sep + h) for p in B.HEADERS), h
    assert len(plslam_amd.ABI_SYMBOLS) == 153 and not [s for s in plslam_amd.ABI_SYMBOLS if "bow_train" in s]
    assert "bow_train" not in plslam_amd.__all__ and len(plslam_amd.__all__) == 25
    assert (bow_train.MAX_N, bow_train.MAX_K, bow_train.MAX_L, bow_train.DEFAULT_MAX_ITERS) == (1 << 24, 256, 16, 1000)
    hdr = open(os.path.join(ROOT, "include", "plslam_bow_train.h")).read()
    for name, v in (("MAX_N", 1 << 24), ("MAX_K", 256), ("MAX_L", 16), ("DEFAULT_MAX_ITERS", 1000)):
        assert re.search(r"#define PLSLAM_BOW_TRAIN_%s %d\b" % (name, v), hdr), name
