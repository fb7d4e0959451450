"""The host half of the loop-closure pose graph (plslam_amd/csrc/pgo_graph.hpp) without a GPU: tests/cpp/test_pgo_graph.cpp is
compiled with g++ alone (no HIP header, no library).  Its hand cases run once, every case one test here; its dump mode prints
the planner's lists for every pose-graph input of the device tests, compared entry for entry with tests/pgo_ref.py and, where
the restatement has no counterpart, with the lists' own definitions.  The same program built with the address and
undefined-behaviour sanitizers runs stand-alone and must come out clean."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from plslam_amd import pgo

import pgo_cases
import pgo_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HAND = ["two_keyframes", "null_keyframe_inside_the_range", "vinit_break_rule", "bfs_tie_by_incident_edge_order",
        "two_chains_meeting_at_vertex_0", "star_neighbours_by_degree_then_index", "refuse_lc_entry_names_a_null_keyframe",
        "refuse_lc_entry_out_of_range", "refuse_lc_entry_negative", "refuse_keyframe_0_null", "refuse_no_lc_entry",
        "refuse_lc_entry_of_one_keyframe", "refuse_no_path_to_vertex_0", "refuse_negative_max_iters", "refuse_zero_max_trials",
        "refuse_null_arguments", "refuse_more_than_4096_active_vertices"]
SANITIZE = ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]

# every pose-graph input of tests/test_gpu_pgo.py: its CASES and the other pgo.pose_graph calls, then tests/pgo_cases.py
CIRCLE = {
    "kf12": dict(n_kf=12, period=9, n_after=1),
    "P1": dict(n_kf=120),
    "kf400_2loops": dict(n_kf=400, n_loops=2, seed=4),
    "null_slots": dict(n_kf=60, null_slots=(9, 20, 33, 58), seed=6),
    "dup_lc_edge": dict(n_kf=50, extra_lc=((30, 31),), seed=7),
    "several_lc_one_optimized": dict(n_kf=80, n_loops=3, extra_lc=((5, 70),), optimized=(0,), seed=8),
    "rejections": dict(n_kf=60, lc_noise=1.0, seed=9),
    "iteration_limits": dict(n_kf=40, seed=12),
    "same_bits": dict(n_kf=120, seed=13),
    "dense_path": dict(n_kf=120, seed=14),
    "refusals_base": dict(n_kf=30, seed=15),
    "corrected_map": dict(n_kf=60, null_slots=(13, 57), n_after=4, seed=16),
    "world_frame": dict(n_kf=60, seed=6),
}
INPUTS = {name: (lambda kw=kw: pgo.pose_graph(**kw)) for name, kw in CIRCLE.items()}
INPUTS.update(pgo_cases.INPUTS)
INPUTS.update(many_loops=pgo_cases.many_loops, wide_band_window8=lambda: pgo_cases.wide_band(window=8),
              nan_pose=lambda: pgo_cases.with_nan_pose(pgo_cases.tumbling(n_kf=60, seed=35), 20),
              tumbling_corrections=lambda: pgo_cases.tumbling(n_kf=60, seed=36, n_after=4))


def _build(exe, extra):
    subprocess.run([shutil.which("g++") or "g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror"] + extra +
                   [os.path.join(ROOT, "tests", "cpp", "test_pgo_graph.cpp"), "-I" + os.path.join(ROOT, "plslam_amd", "csrc"),
                    "-I" + os.path.join(ROOT, "include"), "-o", exe], check=True)
    return exe


def _hand(exe):
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    res = dict(line.split(" ", 1)[::-1] for line in r.stdout.splitlines() if line.startswith(("PASS ", "FAIL ")))
    return {k.split(":")[0]: (v, k) for k, v in res.items()}, r.returncode, r.stderr


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return _build(str(tmp_path_factory.mktemp("pgo_graph") / "test_pgo_graph"), [])


@pytest.fixture(scope="module")
def hand_results(exe):
    return _hand(exe)


@pytest.mark.parametrize("case", HAND)
def test_pgo_graph_hand_case(hand_results, case):
    res = hand_results[0]
    assert case in res, f"{case}: the driver did not run it"
    assert res[case][0] == "PASS", res[case][1]


def test_pgo_graph_driver_ran_every_case(hand_results):
    res, rc, _ = hand_results
    assert sorted(res) == sorted(HAND)
    assert rc == (0 if all(v[0] == "PASS" for v in res.values()) else 1)


def _write_case(path, m, ess=75, cov=75):
    fg = np.asarray(m["full_graph"])
    i, j = np.nonzero(fg)
    with open(path, "w") as f:
        f.write(f"{fg.shape[0]} {len(m['lc_idx'])} {ess} {cov}\n")
        f.write(" ".join(str(int(v)) for v in m["kf_valid"]) + "\n")
        f.write(" ".join(str(int(v)) for v in np.asarray(m["lc_idx"]).reshape(-1)) + "\n")
        f.write(f"{len(i)}\n")
        f.write("\n".join(f"{a} {b} {fg[a, b]}" for a, b in zip(i, j)) + "\n")


def _dump(exe, path):
    r = subprocess.run([exe, "--dump", path], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and not r.stderr.strip(), r.stderr[-3000:]
    out = {}
    for line in r.stdout.splitlines():
        key, *vals = line.split()
        out[key] = np.array([int(v) for v in vals], np.int64)
    return out


def _check_lists(m, d):
    assert d["rc"][0] == 0
    n_map, kf_curr, nv, ne, na, N, nlvl, bw = (int(v) for v in d["counts"])
    g = pgo_ref.build_graph(m["kf_valid"], m["full_graph"], m["lc_idx"])
    vslot = d["vslot"]
    # ---- against the restatement, entry for entry: vertices, edges, the BFS tree, the active set
    assert n_map == len(m["kf_valid"]) and kf_curr == g["kf_curr"] and vslot.tolist() == g["verts"] and nv == len(vslot)
    ev, elc = d["ev"].reshape(-1, 2), d["elc"]
    assert ne == len(ev) == len(elc)
    assert [(int(vslot[x]), int(vslot[y]), int(k >= 0), int(k)) for (x, y), k in zip(ev, elc)] == g["edges"]
    order, level = pgo_ref.bfs_tree(g)
    tree, lvl_ptr = d["tree"].reshape(-1, 4), d["lvl_ptr"]
    assert [(int(vslot[v]), int(vslot[u]), int(e)) for v, u, e, _ in tree] == order
    assert all(int(f) == int(ev[e][0] == u) for _, u, e, f in tree)
    assert nlvl == len(lvl_ptr) - 1 and lvl_ptr[0] == 0 and lvl_ptr[-1] == len(tree) and (np.diff(lvl_ptr) > 0).all()
    for l in range(nlvl):
        assert all(level[int(vslot[v])] == l + 1 for v in tree[lvl_ptr[l]:lvl_ptr[l + 1], 0])
    vcol = d["vcol"]
    act = [v for v in range(nv) if vcol[v] >= 0]
    assert [int(vslot[v]) for v in act] == pgo_ref.active_vertices(g) and na == len(act) and N == 6 * na
    # ---- what has no Python counterpart: from the definitions
    ord_ = d["ord"]
    assert sorted(ord_.tolist()) == list(range(na))
    pos = np.empty(na, np.int64)
    pos[ord_] = np.arange(na)
    assert [int(vcol[v]) for v in act] == pos.tolist()          # active vertex k sits at position pos[k]
    first = np.arange(na)
    for x, y in ev:                                              # the lowest position among a block and its neighbours
        cx, cy = vcol[x], vcol[y]
        if cx >= 0 and cy >= 0:
            first[cx] = min(first[cx], cy)
            first[cy] = min(first[cy], cx)
    cs, off, reach = d["cs"], d["off"], d["reach"]
    assert len(cs) == N and np.array_equal(cs, np.repeat(6 * first, 6))
    r = np.arange(N)
    assert len(off) == N + 1 and off[0] == 0 and np.array_equal(np.diff(off), r - cs + 1)
    assert np.array_equal(reach, np.where(cs[None, :] <= r[:, None], r[None, :], -1).max(1)) and bw == (r - cs).max()
    # targets: unique, sorted by (row, col), lower triangle; their ranges tile contrib
    tg, contrib = d["tg"].reshape(-1, 4), d["contrib"]
    keys = [(int(a), int(b)) for a, b, _, _ in tg]
    assert keys == sorted(set(keys)) and all(a >= b for a, b in keys)
    assert tg[0, 2] == 0 and tg[-1, 3] == len(contrib) and np.array_equal(tg[1:, 2], tg[:-1, 3]) and (tg[:, 3] > tg[:, 2]).all()
    want = {}
    for e, (x, y) in enumerate(ev):
        ci, cj = int(vcol[x]), int(vcol[y])
        if ci >= 0:
            want[4 * e + 0] = (ci, ci)
        if cj >= 0:
            want[4 * e + 1] = (cj, cj)
        if ci >= 0 and cj >= 0:
            assert ci != cj
            want[4 * e + (2 if ci > cj else 3)] = (max(ci, cj), min(ci, cj))
    got = {}
    for a, b, c0, c1 in tg:
        codes = contrib[c0:c1]
        assert (np.diff(codes >> 2) > 0).all()                  # ascending edge order inside a target
        for c in codes:
            assert int(c) not in got
            got[int(c)] = (int(a), int(b))
    assert got == want                                           # every (edge, kind) exactly once, in its own block
    rptr, rlist = d["rptr"], d["rlist"]
    assert len(rptr) == na + 1 and rptr[0] == 0 and rptr[-1] == len(rlist)
    want_r = [[] for _ in range(na)]
    for e, (x, y) in enumerate(ev):
        for side, v in enumerate((x, y)):
            if vcol[v] >= 0:
                want_r[vcol[v]].append(2 * e + side)
    assert [rlist[rptr[p]:rptr[p + 1]].tolist() for p in range(na)] == want_r          # built in edge order: ascending
    assert all((np.diff(np.array(w) >> 1) > 0).all() for w in want_r)
    # the vertex-init rule of pgo_ref.initial_estimates
    lc = np.asarray(m["lc_idx"]).reshape(-1, 3)
    vinit = d["vinit"].reshape(-1, 2)
    for v, (slot, ident) in enumerate(vinit):
        w = -1
        for k, (a, b, _) in enumerate(lc):
            if a == vslot[v]:
                break
            if b == vslot[v]:
                w = k
                break
        assert slot == vslot[v] and ident == w


@pytest.mark.parametrize("name", list(INPUTS))
def test_pgo_graph_lists_of_a_device_test_input(exe, tmp_path, name):
    m = INPUTS[name]()
    path = str(tmp_path / "case.txt")
    _write_case(path, m)
    _check_lists(m, _dump(exe, path))


def test_pgo_graph_clean_under_sanitizers(tmp_path):
    """The hand cases and the dump of the widest inputs, in a build of the program with the sanitizers: a program of its own."""
    san = _build(str(tmp_path / "test_pgo_graph_san"), SANITIZE)
    res, rc, err = _hand(san)
    assert rc == 0 and not err.strip(), err[-3000:]
    assert sorted(res) == sorted(HAND) and all(v[0] == "PASS" for v in res.values())
    for name in ("null_slots", "many_loops", "near_5e-6"):
        m = INPUTS[name]()
        path = str(tmp_path / f"{name}.txt")
        _write_case(path, m)
        _check_lists(m, _dump(san, path))
