"""A C++ client (tests/cpp/test_lc_fuse_shim.cpp) uploads a generated map once, packs lc_idx_list / lc_pt_idxs / lc_ls_idxs and the
keyframes' features through plslam_amd/host/lc_fuse.hpp, fuses on the device and applies the records to its own containers
(full_graph, map_*_kf_idx, a per-observation list); the image, the records and the containers it ends with must be what the
sequential restatement gives."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import lc_fuse_cases as CS
import lc_fuse_ref as R
import plslam_amd

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _with_features(m, lc, seed=31):
    """the keyframes' features (values per feature of the image) and lc with its per-tuple values gathered from them, zeros where the
    keyframe has no such feature: what the client's pack() must produce"""
    rng = np.random.Generator(np.random.PCG64(seed))
    feats, out = {}, dict(lc)
    for kind, dl, dv in (("points", 3, 2), ("lines", 6, 3)):
        A, K = m[kind], lc[kind]
        nf = A["feat_idx"].size
        P, obs = rng.uniform(-3.0, 3.0, (nf, dl)) + np.tile([0.0, 0.0, 8.0], dl // 3), rng.uniform(0.0, 700.0, (nf, dv))
        feats[kind] = (P, obs)
        new = dict(K, P0=np.zeros_like(K["P0"]), obs0=np.zeros_like(K["obs0"]), P1=np.zeros_like(K["P1"]), obs1=np.zeros_like(K["obs1"]))
        ent = np.repeat(np.arange(len(lc["lc_idx"])), np.diff(K["entry_ptr"]))
        for t, (a, l0, b, l1) in enumerate(K["tuples"].tolist()):
            for side, ldx in ((0, l0), (1, l1)):
                kf = int(lc["lc_idx"][ent[t]][side])
                if 0 <= ldx < A["feat_ptr"][kf + 1] - A["feat_ptr"][kf]:
                    f = A["feat_ptr"][kf] + ldx
                    new[f"P{side}"][t], new[f"obs{side}"][t] = P[f], obs[f]
        out[kind] = new
    return feats, out


def _kf_idx(A, nk):
    """map_*_kf_idx: every valid landmark with observations under its first observer (where that is a slot of the map)"""
    lists = [[] for _ in range(nk)]
    for x in range(A["n"]):
        if A["valid"][x] and A["obs_ptr"][x + 1] > A["obs_ptr"][x] and 0 <= A["obs_kf"][A["obs_ptr"][x]] < nk:
            lists[A["obs_kf"][A["obs_ptr"][x]]].append(x)
    return lists


def test_cpp_client_fuses_a_loop_closure(ctx, tmp_path):
    lib = os.path.dirname(plslam_amd.LIB_PATH)
    exe = str(tmp_path / "test_lc_fuse_shim")
    subprocess.run([shutil.which("g++") or "g++", "-O2", "-std=c++17", "-D__HIP_PLATFORM_AMD__",
                    os.path.join(ROOT, "tests", "cpp", "test_lc_fuse_shim.cpp"), "-I" + os.path.join(ROOT, "include"),
                    "-I/opt/rocm/include", "-L" + lib, "-lplslam_hip", "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib",
                    "-L/opt/rocm/lib", "-lamdhip64", "-o", exe], check=True)
    m, lc0 = CS.CASES["mixed"]()
    feats, lc = _with_features(m, lc0)
    m2, out = R.fuse(m, lc)
    nk = m["n_map_kf"]

    def put(name, a, dt):
        np.ascontiguousarray(a, dt).tofile(str(tmp_path / f"{name}.bin"))
    put("lc_idx", lc["lc_idx"], np.int32)
    put("T_kf_w", lc["T_kf_w"], np.float64)
    put("kf_valid", m["kf_valid"], np.uint8)
    put("x_kf_w", m["x_kf_w"], np.float64)
    before = {}
    for kind, tag in (("points", "pt"), ("lines", "ls")):
        for f in ("valid", "inlier", "X", "obs_ptr", "obs_kf", "obs_val", "feat_ptr", "feat_idx"):
            put(f"{tag}_{f}", m[kind][f], m[kind][f].dtype)
        put(f"{tag}_tuples", lc[kind]["tuples"], np.int32)
        put(f"{tag}_entry_ptr", lc[kind]["entry_ptr"], np.int32)
        put(f"{tag}_feat_P", feats[kind][0], np.float64)
        put(f"{tag}_feat_obs", feats[kind][1], np.float64)
        before[kind] = _kf_idx(m[kind], nk)
        put(f"{tag}_kf_idx_ptr", np.concatenate([[0], np.cumsum([len(x) for x in before[kind]])]), np.int32)
        put(f"{tag}_kf_idx", [v for x in before[kind] for v in x], np.int32)
    r = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr

    def got(name, dt):
        return np.fromfile(str(tmp_path / f"out_{name}.bin"), dt)
    names = ("n_a", "n_b", "n_c", "n_d", "n_new", "n_dead", "n_skipped")
    assert got("counts", np.int32).tolist() == [out[k]["counts"][c] for k in ("points", "lines") for c in names]
    assert out["points"]["counts"]["n_skipped"] > 20 and out["points"]["counts"]["n_d"] > 10
    assert np.array_equal(got("full_graph", np.int32).reshape(nk, nk), 1 + out["graph_delta"])
    for kind, tag in (("points", "pt"), ("lines", "ls")):
        o = out[kind]
        assert np.array_equal(got(f"{tag}_ev", np.int32), o["ev"].ravel()), kind
        assert np.array_equal(got(f"{tag}_dir", np.uint64), o["dir"].ravel().view(np.uint64)), kind
        assert np.array_equal(got(f"{tag}_obs_src", np.int32), o["obs_src"]), kind
        # the containers, from the restatement's records: a new landmark under kf_prev, a fused one out of its first observer's list
        want = [list(x) for x in before[kind]]
        for code, keep, dead, anchor, _, _ in o["ev"].tolist():
            if code == 3:
                want[anchor].append(keep)
            elif code == 4 and 0 <= anchor < nk and dead in want[anchor]:
                want[anchor].remove(dead)
        p, v = got(f"{tag}_kf_idx_ptr", np.int32), got(f"{tag}_kf_idx", np.int32)
        assert [v[p[i]:p[i + 1]].tolist() for i in range(nk)] == want, kind
        dead = o["ev"][o["ev"][:, 0] == 4, 2]
        assert not np.isin(dead, v).any() and np.isin(o["ev"][o["ev"][:, 0] == 3, 1], v).all()
        for f in ("valid", "inlier", "X", "obs_ptr", "obs_kf", "obs_val", "feat_ptr", "feat_idx"):
            w = np.ascontiguousarray(m2[kind][f]).ravel()
            g = got(f"{tag}_{f}", w.dtype)
            assert g.shape == w.shape, (kind, f, g.shape, w.shape)
            assert np.array_equal(g.view(np.uint64) if w.dtype == np.float64 else g, w.view(np.uint64) if w.dtype == np.float64 else w), (kind, f)
    src = out["points"]["obs_src"]
    assert np.array_equal(got("pt_list", np.int32), np.where(src >= 0, 1000 + src, -1 - src))
    assert np.array_equal(got("kf_valid", np.uint8), m2["kf_valid"])
    assert np.array_equal(got("x_kf_w", np.uint64), m2["x_kf_w"].ravel().view(np.uint64))
