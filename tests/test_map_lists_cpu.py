"""CPU tests of the map-lists feature's checker and generators: the replay of the event records (tests/map_lists_ref.py) proves
its own ordering on every case of both case tables; the generators are seeded; the clustered generator really produces the ties
the "first row wins" rule needs; the numpy rule of the generators equals the oracle's; the header declares the new symbols and
the binding carries them."""
import os
import re

import numpy as np
import pytest

import lc_fuse_cases as FC
import map_insert_cases as IC
import map_lists_ref as R
import plslam_amd
from oracle import oracle as O
from plslam_amd import map_lists as ML

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("plslam_map_lists_refresh", "plslam_map_insert_carry", "plslam_lc_fuse_carry")


def _touched_ties(want, m_after):
    return sum(R.tied_landmarks(want[k]["desc"], np.asarray(m_after[k]["obs_ptr"]), np.flatnonzero(want[k]["refreshed"]).tolist()) for k in R.KINDS)


@pytest.mark.parametrize("name", sorted(IC.CASES))
def test_insert_replay_checks_itself_and_has_ties(name):
    """run_insert asserts inside the replay that the replayed obs_ptr / obs_kf are the restatement's image, for both passes"""
    r = R.run_insert(name)
    for want, m_after, out in ((r["want_a"], r["m_a"], r["out_a"]), (r["want_b"], r["m_b"], r["out_b"])):
        for k in R.KINDS:
            W = want[k]
            n, n_obs = m_after[k]["n"], m_after[k]["obs_kf"].size
            assert W["desc"].shape == (n_obs, 32) and W["dir"].shape == (n_obs, 3) and W["obs_src"].shape == (n_obs,)
            assert W["med_idx"].shape == (n,) and W["med_desc"].shape == (n, 32) and W["refreshed"].shape == (n,)
            assert (k == "lines") == ("pts" in W)
            assert int(W["refreshed"].sum()) == np.unique(out[k]["ev"][:, 0]).size
            assert (W["obs_src"] < 0).sum() == out[k]["counts"]["n_appended"]
    if name == "no_events":
        assert not r["want_a"]["points"]["refreshed"].any() and (r["want_a"]["points"]["obs_src"] == np.arange(r["m"]["points"]["obs_kf"].size)).all()
    else:
        assert _touched_ties(r["want_a"], r["m_a"]) >= 1, "no touched landmark whose winning value two rows share"
    if name.startswith("tile_events"):
        n = IC.T + int(name.rsplit("_", 1)[1])                    # the touched count at the tile's edge
        assert r["want_a"]["points"]["refreshed"].sum() == r["want_a"]["lines"]["refreshed"].sum() == r["want_b"]["points"]["refreshed"].sum() == n


@pytest.mark.parametrize("name", sorted(FC.CASES))
def test_fuse_replay_checks_itself_and_has_ties(name):
    r = R.run_fuse(name)
    if r is None:
        assert name == "level_over"
        return
    ties = _touched_ties(r["want"], r["m_a"])
    for k in R.KINDS:
        W, ev = r["want"][k], r["out"][k]["ev"]
        dead = ev[ev[:, 0] == 4][:, 2]
        assert (W["med_idx"][dead] == -1).all() and not W["med_desc"][dead].any() and (W["refreshed"][dead] == 1).all()
        assert np.array_equal(W["obs_src"], r["out"][k]["obs_src"])
    if name == "no_events":
        assert not r["want"]["points"]["refreshed"].any()
    else:
        assert ties >= 1, "no touched landmark whose winning value two rows share"
    if name in ("grown_then_fused", "nested"):                    # a D fusion that follows an A / B on the same landmark
        assert any((r["want"][k]["obs_src"][np.asarray(r["m_a"][k]["obs_ptr"])[ev_[1]]:np.asarray(r["m_a"][k]["obs_ptr"])[ev_[1] + 1]] < 0).sum() >= 1
                   for k in R.KINDS for ev_ in r["out"][k]["ev"] if ev_[0] == 4)


def test_untouched_landmarks_keep_what_the_source_stores():
    r = R.run_insert("mixed", True, True)
    for k in R.KINDS:
        W, src = r["want_a"][k], r["lists0"][k]
        same = np.flatnonzero(W["refreshed"][:src["med_idx"].size] == 0)
        lens = np.diff(r["m"][k]["obs_ptr"])
        assert same.size > 50 and np.array_equal(W["med_idx"][same], lens[same] - 1) and np.array_equal(W["med_desc"][same], src["med_desc"][same])
        true_idx, true_med = O.median_desc_batched(W["desc"], r["m_a"][k]["obs_ptr"].astype(np.int32))
        t = np.flatnonzero(W["refreshed"])
        assert np.array_equal(W["med_idx"][t], true_idx[t]) and np.array_equal(W["med_desc"][t], true_med[t])
        assert (true_idx[same] != lens[same] - 1).any()           # (the planted value is not the representative everywhere)


def test_generators_are_seeded():
    m, kf, _ = IC.CASES["mixed"]()
    _, lc = FC.CASES["three_entries"]()
    for clustered in (False, True):
        a, b, c = (ML.synthetic_lists(m, seed=s, clustered=clustered) for s in (3, 3, 4))
        ka, kb, kc = (ML.keyframe_rows(kf, seed=s, clustered=clustered) for s in (3, 3, 4))
        ta, tb, tc = (ML.tuple_rows(lc, seed=s, clustered=clustered) for s in (3, 3, 4))
        for x, y, z in ((a, b, c), (ka, kb, kc), (ta, tb, tc)):
            for k in R.KINDS:
                assert sorted(x[k]) == sorted(y[k])
                assert all(np.array_equal(x[k][f], y[k][f]) for f in x[k])
                assert not np.array_equal(x[k][next(iter(x[k]))], z[k][next(iter(x[k]))])
        assert a["points"]["desc"].shape == (m["points"]["obs_kf"].size, 32) and a["lines"]["pts"].shape == (m["lines"]["obs_kf"].size, 4)
        assert "pts" not in a["points"] and "pts1" not in ka["points"] and ka["lines"]["pts2"].shape == (kf["lines"]["P2"].shape[0], 4)
        assert ta["points"]["desc0"].shape == (lc["points"]["tuples"].shape[0], 32)
        assert np.allclose(np.linalg.norm(a["points"]["dir"], axis=1), 1.0)


def test_the_generators_rule_is_the_oracles():
    """representative() (numpy, in the product's generator module) against the oracle pinned to the reference, with empty lists,
    single observations, ties and lists on both sides of the row cache's 16"""
    from plslam_amd import synth
    rng = np.random.Generator(np.random.PCG64(12))
    for max_obs, ties in ((7, True), (7, False), (20, True)):
        d, off = synth.landmark_desc_lists(rng, 300, max_obs=max_obs, empty_frac=0.05, ties=ties)
        gi, gm = ML.representative(d, off)
        ri, rm = O.median_desc_batched(d, off)
        assert np.array_equal(gi, ri) and np.array_equal(gm[gi >= 0], rm[gi >= 0]) and not gm[gi < 0].any()
        assert (gi == -1).any() and (np.diff(off) == 1).any()


def test_header_declares_and_binding_carries_the_new_symbols():
    src = open(os.path.join(ROOT, "include", "plslam_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for s in NEW_SYMBOLS:
        assert re.search(r"\bint\s+" + s + r"\s*\(", code), s
        assert s in plslam_amd.ABI_SYMBOLS
    for t in ("plslam_map_lists_kind", "plslam_map_lists", "plslam_map_insert_rows", "plslam_lc_fuse_rows"):
        assert re.search(r"\}\s*" + t + r"\s*;", code), t
    assert re.search(r"void\*\s*stream;\s*int32_t\s*\*pt_obs_src,\s*\*ls_obs_src;\s*\}\s*plslam_map_insert_events", code)
    assert "#define PLSLAM_ABI_VERSION 5" in src
    L = plslam_amd.load()
    for s in NEW_SYMBOLS:
        assert getattr(L, s).argtypes is not None and len(getattr(L, s).argtypes) == (3 if s.endswith("refresh") else 7)
    from plslam_amd import map_insert as MI
    assert [f for f, _ in MI.MapInsertEvents._fields_][-3:] == ["stream", "pt_obs_src", "ls_obs_src"]
    assert [f for f, _ in ML.MapListsKind._fields_] == ["desc", "dir", "pts", "med_idx", "med_desc", "refreshed"]
