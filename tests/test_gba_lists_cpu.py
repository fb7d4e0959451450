"""The host-built lists of the global bundle adjustment (plslam_amd/csrc/gba_lists.hpp) without a GPU: tests/cpp/test_gba_lists.cpp
is compiled with g++ alone (no HIP header, no library).  Its hand cases run once, every case one test here; its dump mode prints
the real lists for every input of tests/gba_cases.py, compared with tests/test_gba_cpu.py::plan_layout (the restatement of the
planner's comment) and with the lists' own definitions.  The same program built with the address and undefined-behaviour
sanitizers runs stand-alone and must come out clean."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import gba_cases
from test_gba_cpu import plan_layout

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HAND = ["one_keyframe_no_observation", "landmark_seen_by_keyframe_0_only", "chunk_boundaries",
        "refuse_point_landmark_index_past_the_end", "refuse_point_landmark_index_negative", "refuse_line_landmark_index_past_the_end",
        "refuse_point_local_keyframe_below_minus_one", "refuse_line_local_keyframe_below_minus_one",
        "refuse_point_local_keyframe_past_the_end", "refuse_point_map_keyframe_out_of_range",
        "refuse_point_local_keyframe_is_not_its_map_keyframe", "refuse_line_local_keyframe_is_not_its_map_keyframe",
        "refuse_kf_list_out_of_range"]
SANITIZE = ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]
INPUTS = dict(gba_cases.INPUTS, **gba_cases.DEGENERATE)


def _build(exe, extra):
    subprocess.run([shutil.which("g++") or "g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror"] + extra +
                   [os.path.join(ROOT, "tests", "cpp", "test_gba_lists.cpp"), "-I" + os.path.join(ROOT, "plslam_amd", "csrc"),
                    "-I" + os.path.join(ROOT, "include"), "-o", exe], check=True)
    return exe


def _hand(exe):
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    res = dict(line.split(" ", 1)[::-1] for line in r.stdout.splitlines() if line.startswith(("PASS ", "FAIL ")))
    return {k.split(":")[0]: (v, k) for k, v in res.items()}, r.returncode, r.stderr


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return _build(str(tmp_path_factory.mktemp("gba_lists") / "test_gba_lists"), [])


@pytest.fixture(scope="module")
def hand_results(exe):
    return _hand(exe)


@pytest.mark.parametrize("case", HAND)
def test_gba_lists_hand_case(hand_results, case):
    res = hand_results[0]
    assert case in res, f"{case}: the driver did not run it"
    assert res[case][0] == "PASS", res[case][1]


def test_gba_lists_driver_ran_every_case(hand_results):
    res, rc, _ = hand_results
    assert sorted(res) == sorted(HAND)
    assert rc == (0 if all(v[0] == "PASS" for v in res.values()) else 1)


def _write_case(path, m):
    pt, ls = np.asarray(m["pt_obs"]).reshape(-1, 6), np.asarray(m["ls_obs"]).reshape(-1, 6)
    with open(path, "w") as f:
        f.write(f"{m['n_map_kf']} {len(m['kf_list'])} {m['npt']} {m['nls']} {len(pt)} {len(ls)}\n")
        f.write(" ".join(str(int(v)) for v in m["kf_list"]) + "\n")
        for rows in (pt, ls):
            f.write("\n".join(" ".join(str(int(v)) for v in row) for row in rows) + "\n")


def _dump(exe, path):
    r = subprocess.run([exe, "--dump", path], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and not r.stderr.strip(), r.stderr[-3000:]
    out = {}
    for line in r.stdout.splitlines():
        key, *vals = line.split()
        out[key] = np.array([int(v) for v in vals], np.int64)
    return out


def real_layout(d):
    """plan_layout's dict from the real lists: {(k1, k2): (point pairs, line pairs, [chunk sizes])}"""
    blks, chks = d["blks"].reshape(-1, 4), d["chks"].reshape(-1, 4)
    out = {}
    for b, (k1, k2, c0, c1) in enumerate(blks):
        c = chks[c0:c1]
        assert (c[:, 0] == b).all() and (np.diff(c[:, 1]) >= 0).all()              # the block's own; points before lines
        out[(int(k1), int(k2))] = (int(c[c[:, 1] == 0, 3].sum()), int(c[c[:, 1] == 1, 3].sum()), c[:, 3].tolist())
    return out


def _check_lists(m, d):
    assert d["rc"][0] == 0
    lay = plan_layout(m)
    got = real_layout(d)
    assert list(got) == sorted(got) == list(lay)                # the blocks, in (k1, k2) order
    assert got == lay                                           # per-kind pair counts and chunk sizes
    pt, ls = np.asarray(m["pt_obs"]).reshape(-1, 6), np.asarray(m["ls_obs"]).reshape(-1, 6)
    n_map = m["n_map_kf"]
    assert np.array_equal(d["plm"], pt[:, 1]) and np.array_equal(d["pkf"], pt[:, 4])
    assert np.array_equal(d["pslot"], np.where(pt[:, 4] >= 0, n_map + pt[:, 4], pt[:, 3]))
    assert np.array_equal(d["llm"], ls[:, 1]) and np.array_equal(d["lkf"], ls[:, 4]) and np.array_equal(d["lslot"], ls[:, 3])
    # the four CSR lists: the observations by optimised keyframes, stable
    for ptr, ids, key, kf, n in (("lpp", "lpo", pt[:, 1], pt[:, 4], m["npt"]), ("llp", "llo", ls[:, 1], ls[:, 4], m["nls"]),
                                 ("kpp", "kpo", pt[:, 4], pt[:, 4], len(m["kf_list"])),
                                 ("klp", "klo", ls[:, 4], ls[:, 4], len(m["kf_list"]))):
        sel = np.flatnonzero(kf >= 0)
        assert np.array_equal(d[ids], sel[np.argsort(key[sel], kind="stable")])
        assert np.array_equal(d[ptr], np.concatenate([[0], np.cumsum(np.bincount(key[sel], minlength=n))]))
    # chunks tile the pair list; a pair lies in its block with kf(o1) >= kf(o2); pairs of one kind in a block are in landmark order
    blks, chks, pairs = d["blks"].reshape(-1, 4), d["chks"].reshape(-1, 4), d["pairs"].reshape(-1, 2)
    assert np.array_equal(chks[:, 2], np.concatenate([[0], np.cumsum(chks[:, 3])[:-1]])) and chks[:, 3].sum() == len(pairs)
    assert ((chks[:, 3] >= 1) & (chks[:, 3] <= 64)).all()
    for b, (k1, k2, c0, c1) in enumerate(blks):
        for line in (0, 1):
            c = chks[c0:c1][chks[c0:c1, 1] == line]
            if not len(c):
                continue
            q = pairs[c[0, 2]:c[-1, 2] + c[-1, 3]]
            lm, kf = (d["llm"], d["lkf"]) if line else (d["plm"], d["pkf"])
            assert (kf[q[:, 0]] == k1).all() and (kf[q[:, 1]] == k2).all() and np.array_equal(lm[q[:, 0]], lm[q[:, 1]])
            assert (np.diff(lm[q[:, 0]]) >= 0).all()
            assert (c[:-1, 3] == 64).all()                      # only the last chunk of a kind is ragged


@pytest.mark.parametrize("name", list(INPUTS))
def test_gba_lists_of_a_device_test_input(exe, tmp_path, name):
    m = INPUTS[name]()
    path = str(tmp_path / "case.txt")
    _write_case(path, m)
    _check_lists(m, _dump(exe, path))


def test_chunks_blocks_hold_the_pair_counts_they_are_built_for_in_the_real_lists(exe, tmp_path):
    """tests/test_gba_cpu.py's check of gba_cases.CHUNK_BLOCKS, on the lists the planner builds"""
    path = str(tmp_path / "chunks.txt")
    _write_case(path, gba_cases.chunks())
    lay = real_layout(_dump(exe, path))
    assert {b: v[:2] for b, v in lay.items()} == gba_cases.CHUNK_BLOCKS
    assert lay[(1, 0)][2] == [63] and lay[(2, 1)][2] == [64, 1] and lay[(3, 0)][2] == [64, 64] and lay[(3, 1)][2] == [64, 64, 1]
    assert lay[(2, 0)][2] == [64, 64, 1] and lay[(3, 2)][2] == [1]
    assert lay[(0, 0)][2] == [64, 64, 64, 63, 64, 1] and lay[(3, 3)][2] == [64, 64, 64, 64, 2]


def test_gba_lists_clean_under_sanitizers(tmp_path):
    """The hand cases and the dump of the inputs with the most irregular lists, in a build of the program with the sanitizers"""
    san = _build(str(tmp_path / "test_gba_lists_san"), SANITIZE)
    res, rc, err = _hand(san)
    assert rc == 0 and not err.strip(), err[-3000:]
    assert sorted(res) == sorted(HAND) and all(v[0] == "PASS" for v in res.values())
    for name in ("chunks", "gaps", "no_point_obs"):
        m = INPUTS[name]()
        path = str(tmp_path / f"{name}.txt")
        _write_case(path, m)
        _check_lists(m, _dump(san, path))
