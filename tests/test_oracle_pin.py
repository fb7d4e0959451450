"""CPU tests that PIN THE ORACLE (no GPU): distance against the reference's own in-tree popcount
code (oracle/_ref), kNN-2 / ratio / mutual against an independent numpy formulation and the
committed golden vectors, LBA rows against finite differences and a literal numpy restatement.

Parity status: the reference holds no tests for this path and its matcher arithmetic is in
OpenCV/stvo-pl (absent) -> tie order / ratio / mutual are "parity unpinned" (SURVEY.md 8c).  What the reference
tree itself can pin is pinned: the distance (its two popcount implementations) and the two nearest DISTANCES per
query (its in-tree exact kNN search, BinaryDescriptorMatcher::knnMatch, live through oracle/_ref and as committed
outputs in tests/golden/ref_knn_golden.npz).
"""
import os

import numpy as np
import pytest
from hypothesis import given, settings, strategies as st

from oracle import oracle as O
from plslam_amd import synth

GOLD = os.path.join(os.path.dirname(__file__), "golden", "match_golden.npz")


def _rng(seed=0):
    return np.random.Generator(np.random.PCG64(seed))


# The reference's outputs for the pinning tests below, recorded from oracle/_ref by tests/golden/make_ref_calls_golden.py:
# where oracle/_ref was never built (no reference tree at build time) the tests check the oracle against these; where it was,
# the live outputs are checked against them too.
REF_CALLS = os.path.join(os.path.dirname(__file__), "golden", "ref_calls_golden.npz")
_REF_CALLS = None


def _encode(v, key, out):
    if isinstance(v, tuple):
        out[key + "/tuple"] = np.array(len(v))
        for i, x in enumerate(v):
            _encode(x, f"{key}/{i}", out)
    elif isinstance(v, np.ndarray):
        out[key] = v
    else:
        out[key + "/scalar"] = np.array(v)


def _decode(key, g):
    if key + "/tuple" in g:
        return tuple(_decode(f"{key}/{i}", g) for i in range(int(g[key + "/tuple"])))
    if key + "/scalar" in g:
        return g[key + "/scalar"].item()
    return g[key]


def _equal(a, b):
    if isinstance(a, tuple):
        return isinstance(b, tuple) and len(a) == len(b) and all(_equal(x, y) for x, y in zip(a, b))
    if isinstance(a, np.ndarray):
        return isinstance(b, np.ndarray) and a.dtype == b.dtype and a.shape == b.shape and \
            np.array_equal(a.view(np.uint8), b.view(np.uint8))
    return a == b


def _reference(key, live, same=None):
    """The reference's output of one case: live() (None without oracle/_ref), else the recorded one.  `same(live, recorded)`
    says what must agree between the two (default: everything, bit for bit)."""
    global _REF_CALLS
    if _REF_CALLS is None:
        _REF_CALLS = dict(np.load(REF_CALLS)) if os.path.exists(REF_CALLS) else {}
    got = live()
    rec_dir = os.environ.get("PLSLAM_RECORD_REF_CALLS")
    if rec_dir and got is not None:                  # make_ref_calls_golden.py: record instead of compare
        enc = {}
        _encode(got, key, enc)
        np.savez(os.path.join(rec_dir, key.replace("/", "__") + ".npz"), **enc)
        return got
    assert key in _REF_CALLS or key + "/tuple" in _REF_CALLS or key + "/scalar" in _REF_CALLS, \
        f"{key}: no recorded reference output in {REF_CALLS} (make_ref_calls_golden.py)"
    rec = _decode(key, _REF_CALLS)
    if got is not None:
        assert (same or _equal)(got, rec), f"{key}: the reference's live output differs from the recorded one"
    return rec


# ---------------------------------------------------------------- distance ----------------
def test_distance_known_answers():
    z = np.zeros(32, np.uint8)
    o = np.full(32, 0xFF, np.uint8)
    one = z.copy()
    one[17] = 0x10
    for v in ("popcnt32", "swar", "lut"):
        assert O.hamming256(z, z, v) == 0
        assert O.hamming256(z, o, v) == 256
        assert O.hamming256(z, one, v) == 1
        assert O.hamming256(o, one, v) == 255
        assert O.hamming256(np.full(32, 0xAA, np.uint8), np.full(32, 0x55, np.uint8), v) == 256


def test_distance_three_restatements_agree():
    r = _rng(1)
    a, b = synth.random_desc(r, 500), synth.random_desc(r, 500)
    for i in range(500):
        d = O.hamming256(a[i], b[i])
        assert d == O.hamming256(a[i], b[i], "swar") == O.hamming256(a[i], b[i], "lut")
        assert d == int(np.bitwise_count(a[i] ^ b[i]).sum())


def test_distance_pinned_to_reference_code():
    """oracle/_ref = the reference's bitops_custom.hpp:83-96 and FORB.cpp:78-101 compiled as is."""
    r = _rng(2)
    a, b = synth.random_desc(r, 400), synth.random_desc(r, 400)
    a[0] = 0
    b[0] = 0xFF

    def live():
        ref = O.ref_lib()
        if ref is None:
            return None
        return np.array([[ref.ref_ld_match(a[i].ctypes.data, b[i].ctypes.data, 32),
                          ref.ref_forb_distance(a[i].ctypes.data, b[i].ctypes.data)] for i in range(400)], np.int32)
    R = _reference("distance", live)
    for i in range(400):
        d = O.hamming256(a[i], b[i])
        assert d == R[i, 0]
        assert d == R[i, 1]


def _untied(D, k=2):
    """Rows whose k nearest are decided by distance alone (all k + 1 smallest distances distinct)."""
    srt = np.sort(D, axis=1)
    if D.shape[1] <= k:
        return np.all(np.diff(srt[:, :k], axis=1) > 0, axis=1)
    return np.all(np.diff(srt[:, :k + 1], axis=1) > 0, axis=1)


@pytest.mark.parametrize("nq,nt,kind,seed", [(300, 280, "plain", 0), (257, 511, "plain", 1), (1500, 1500, "planted", 2),
                                             (200, 220, "ties", 3), (64, 2, "plain", 4), (3, 700, "planted", 5)])
def test_knn2_distances_pinned_to_reference_mih_search(nq, nt, kind, seed):
    """oracle/_ref also holds the reference's in-tree EXACT kNN (BinaryDescriptorMatcher::knnMatch,
    binary_descriptor_matcher.cpp:258-335, compiled as is): the oracle's two nearest distances must be the same for
    every query, and wherever distance alone decides (no tie among the three nearest) so must the indices."""
    r = _rng(900 + seed)
    if kind == "ties":
        q, t = synth.tie_stress_desc(r, nq), synth.tie_stress_desc(r, nt)
    else:
        q, t = synth.random_desc(r, nq), synth.random_desc(r, nt)
        if kind == "planted":
            m = min(nq, nt)
            t[:m] = synth.noisy_copy(r, q[:m])[0]
    # (which of several equally distant rows the engine names varies between its runs: only the distances must agree)
    ridx, rdist = _reference(f"mih_knn/{seed}", lambda: O.ref_mih_knn(q, t, 2), same=lambda a, b: np.array_equal(a[1], b[1]))
    idx, dist = O.knn2(q, t)
    assert np.array_equal(dist, rdist)
    D = np.bitwise_count(q[:, None, :] ^ t[None, :, :]).sum(-1).astype(np.int32)
    # the reference's indices carry its distances -- except on tiny train sets (< ~6 rows), where its engine returns
    # repeated or out-of-range trainIdx values (result array allocated uninitialised); the distances are right
    if nt < 8:
        return
    assert np.array_equal(np.take_along_axis(D, ridx, 1), rdist)
    u = _untied(D)
    assert u.sum() > 0 or kind == "ties"
    assert np.array_equal(idx[u], ridx[u])


def test_knn2_against_committed_reference_outputs():
    """tests/golden/ref_knn_golden.npz = outputs of the reference's own knnMatch (make_ref_knn_golden.py); checked
    without oracle/_ref, so it also runs where /root/reference never existed."""
    g = np.load(os.path.join(os.path.dirname(__file__), "golden", "ref_knn_golden.npz"))
    for name in g["names"]:
        q, t = g[f"{name}/q"], g[f"{name}/t"]
        idx, dist = O.knn2(q, t)
        assert np.array_equal(dist, g[f"{name}/k2_dist"]), name
        assert np.array_equal(g[f"{name}/k3_dist"][:, :2], g[f"{name}/k2_dist"]), name
        D = np.bitwise_count(q[:, None, :] ^ t[None, :, :]).sum(-1).astype(np.int32)
        u = _untied(D)                                   # the fixture keeps indices for exactly these queries
        assert np.array_equal(u, np.all(g[f"{name}/k2_idx"] >= 0, axis=1)), name
        assert np.array_equal(np.take_along_axis(D[u], g[f"{name}/k2_idx"][u], 1), g[f"{name}/k2_dist"][u]), name
        assert np.array_equal(idx[u], g[f"{name}/k2_idx"][u]), name
        # third nearest (k = 3): the oracle's best two are a prefix of the reference's best three
        assert np.all(g[f"{name}/k3_dist"][:, 2] >= dist[:, 1]), name


# ---------------------------------------------------------------- golden vectors ----------
def _gold_cases():
    g = np.load(GOLD)
    names = sorted({k.split("/")[0] for k in g.files})
    return g, names


def test_golden_distances_and_knn():
    g, names = _gold_cases()
    for n in names:
        q, t = g[f"{n}/q"], g[f"{n}/t"]
        assert np.array_equal(O.np_dist_matrix(q, t), g[f"{n}/dist_ref_bitops"]), n
        idx, dist = O.knn2(q, t)
        assert np.array_equal(idx, g[f"{n}/knn_idx"]), n
        assert np.array_equal(dist, g[f"{n}/knn_dist"]), n


def test_golden_match_tables():
    g, names = _gold_cases()
    for n in names:
        q, t = g[f"{n}/q"], g[f"{n}/t"]
        for nnr in (0.6, 0.75, 0.9):
            for mut in (0, 1):
                m, cnt = O.match(q, t, nnr, bool(mut))
                exp = g[f"{n}/m12_nnr{nnr}_mut{mut}"]
                assert np.array_equal(m, exp), (n, nnr, mut)
                assert cnt == int((exp >= 0).sum())


def test_ratio_boundaries_fp32():
    """d0 < d1*nnr evaluated in fp32 with ONE multiply: 9 vs 10*0.9f -> 9.0f exactly -> reject."""
    g, _ = _gold_cases()
    expect = {("9_10", 0.9): -1, ("3_4", 0.75): -1, ("75_100", 0.75): -1, ("0_0", 0.75): -1,
              ("5_5", 0.9): -1, ("89_99", 0.9): 1, ("90_100", 0.9): -1, ("6_10", 0.6): -1,
              ("59_99", 0.6): 1,
              ("60_100", 0.6): 1}   # 100*0.6f rounds UP to 60.000004f in fp32 (fp64 would reject)
    for (name, nnr), want in expect.items():
        q, t = g[f"ratio_{name}/q"], g[f"ratio_{name}/t"]
        m, _ = O.match(q, t, nnr, False)
        assert m[0] == want, (name, nnr, m)
        # same decision straight from IEEE fp32
        d0, d1 = (int(x) for x in name.split("_"))
        dec = np.float32(d0) < np.float32(d1) * np.float32(nnr)
        assert (m[0] >= 0) == bool(dec)


def test_fp32_vs_fp64_ratio_disagreements_exist_only_at_0p6():
    """for the shipped thresholds fp32 and fp64 evaluation agree on every integer pair;
    at nnr=0.6 they do not -- the implementation must be fp32."""
    d = np.arange(0, 257)
    d0, d1 = np.meshgrid(d, d, indexing="ij")
    keep = d0 <= d1
    for nnr in (0.7, 0.75, 0.8, 0.85, 0.9, 0.95):
        f32 = d0.astype(np.float32) < d1.astype(np.float32) * np.float32(nnr)
        f64 = d0.astype(np.float64) < d1.astype(np.float64) * float(nnr)
        assert np.array_equal(f32[keep], f64[keep]), nnr
    f32 = d0.astype(np.float32) < d1.astype(np.float32) * np.float32(0.6)
    f64 = d0.astype(np.float64) < d1.astype(np.float64) * 0.6
    assert (f32[keep] != f64[keep]).sum() > 0


# ---------------------------------------------------------------- kNN-2 / match -----------
@pytest.mark.parametrize("nq,nt", [(0, 5), (5, 0), (3, 1), (3, 2), (1, 1), (64, 64), (65, 129), (200, 37)])
def test_knn2_edge_sizes(nq, nt):
    r = _rng(nq * 1000 + nt)
    q, t = synth.random_desc(r, nq), synth.random_desc(r, nt)
    idx, dist = O.knn2(q, t)
    eidx, edist = O.np_knn2(q, t)
    assert np.array_equal(idx, eidx) and np.array_equal(dist, edist)
    if nt < 2:
        m, n = O.match(q, t, 0.9, False)
        assert n == 0 and (m == -1).all()


def test_knn2_ties_lowest_index_first():
    r = _rng(5)
    t = np.repeat(synth.random_desc(r, 4), 5, axis=0)      # every row appears 5 times
    q = t[::5].copy()
    idx, dist = O.knn2(q, t)
    assert np.array_equal(idx[:, 0], np.arange(4) * 5)
    assert np.array_equal(idx[:, 1], np.arange(4) * 5 + 1)  # second best = same distance, next index
    assert (dist == 0).all()
    m, n = O.match(q, t, 0.9, False)
    assert n == 0                                           # d0 == d1 == 0 -> 0 < 0 false


def test_mutual_semantics_hand_case():
    z = np.zeros((1, 32), np.uint8)

    def row(d):
        b = np.zeros(256, np.uint8)
        b[:d] = 1
        return np.packbits(b)
    # d1 = {A}, d2 = {B(=A+2 bits), C(far)}; plus in d1 a row A' closer to B than A is
    d1 = np.stack([row(10), row(4)])        # A (10 bits), A' (4 bits)
    d2 = np.stack([row(6), row(200)])       # B (6 bits), C
    m_nomut, _ = O.match(d1, d2, 0.75, False)
    assert list(m_nomut) == [0, 0]          # both prefer B (dist 4 and 2)
    m_mut, n = O.match(d1, d2, 0.75, True)
    assert list(m_mut) == [-1, 0] and n == 1  # B's best is A' (dist 2 < 4*0.75) -> A is dropped
    assert z.sum() == 0


@pytest.mark.parametrize("mutual", [False, True])
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_match_on_a_vector_that_already_holds_entries(seed, mutual):
    """plo_match_prior = [RECALL] stvo-pl matchNNR's `matches_12.resize(desc1.rows, -1)` when the caller's vector is the one
    matchGrid filled (src/mapHandler.cpp:271 -> :277): restated here step by step from the directed tables."""
    r = np.random.Generator(np.random.PCG64(seed))
    n1, n2 = 180, 150
    d1 = synth.random_desc(r, n1)
    d2 = synth.random_desc(r, n2)
    k = 90
    d2[:k] = d1[:k] ^ np.packbits(r.random((k, 256)) < 0.04, axis=1)         # true correspondences
    d2[k:k + 20] = d2[:20]                                                    # + duplicates: ratio test fails there
    prior = np.where(r.random(n1) < 0.5, r.integers(0, n2, n1), -1).astype(np.int32)
    m12, _ = O.match(d1, d2, 0.75, False)
    m21, _ = O.match(d2, d1, 0.75, False)
    exp = np.where(m12 >= 0, m12, prior)
    cnt = int((m12 >= 0).sum())
    if mutual:
        for i1 in range(n1):
            if exp[i1] >= 0 and m21[exp[i1]] != i1:
                exp[i1] = -1
                cnt -= 1
    got, n = O.match_prior(d1, d2, 0.75, mutual, prior)
    np.testing.assert_array_equal(got, exp)
    assert n == cnt
    assert ((m12 < 0) & (prior >= 0)).sum() > 10                              # kept entries exist in this case
    if mutual:
        assert n != (got >= 0).sum() or seed < 0                              # ... and the count is not the number of entries
    fresh, nf = O.match_prior(d1, d2, 0.75, mutual, np.full(n1, -1, np.int32))
    ref, nr = O.match(d1, d2, 0.75, mutual)
    np.testing.assert_array_equal(fresh, ref)                                 # an all -1 vector: plain match()
    assert nf == nr


@settings(max_examples=60, deadline=None)
@given(st.integers(0, 40), st.integers(0, 40), st.integers(0, 2 ** 31 - 1), st.booleans(),
       st.sampled_from([0.6, 0.75, 0.9]), st.booleans())
def test_match_property_c_vs_numpy(nq, nt, seed, ties, nnr, mutual):
    r = _rng(seed)
    gen = synth.tie_stress_desc if ties else synth.random_desc
    q, t = gen(r, nq), gen(r, nt)
    if nq and nt and not ties:
        k = min(nq, nt)
        t[:k] = q[:k] ^ np.packbits(r.random((k, 256)) < 0.05, axis=1)
    idx, dist = O.knn2(q, t)
    eidx, edist = O.np_knn2(q, t)
    assert np.array_equal(idx, eidx) and np.array_equal(dist, edist)
    m, n = O.match(q, t, nnr, mutual)
    em, en = O.np_match(q, t, nnr, mutual)
    assert np.array_equal(m, em) and n == en


def test_match_batched_and_threads_agree():
    r = _rng(9)
    sizes1, sizes2 = [30, 0, 17, 64], [25, 10, 0, 70]
    off1 = np.concatenate([[0], np.cumsum(sizes1)]).astype(np.int32)
    off2 = np.concatenate([[0], np.cumsum(sizes2)]).astype(np.int32)
    d1, d2 = synth.random_desc(r, off1[-1]), synth.random_desc(r, off2[-1])
    m, nm = O.match_batched(d1, off1, d2, off2, 0.9, True)
    m2, nm2 = O.match_batched(d1, off1, d2, off2, 0.9, True, nthreads=3)
    assert np.array_equal(m, m2) and np.array_equal(nm, nm2)
    for b in range(4):
        e, n = O.np_match(d1[off1[b]:off1[b + 1]], d2[off2[b]:off2[b + 1]], 0.9, True)
        assert np.array_equal(m[off1[b]:off1[b + 1]], e) and nm[b] == n


def test_median_descriptor_restatement():
    """src/mapFeatures.cpp:51-93 restated in python: sorted row, element int(1+0.5(n-1)), first min."""
    r = _rng(3)
    for n in (2, 3, 4, 5, 8, 11):
        base = synth.random_desc(r, 1)
        d = np.repeat(base, n, axis=0) ^ np.packbits(r.random((n, 256)) < 0.1, axis=1)
        D = O.np_dist_matrix(d, d)
        med = int(1 + 0.5 * (n - 1))
        vals = [sorted(D[i])[med] for i in range(n)]
        assert O.median_desc(d) == int(np.argmin(vals))
    assert O.median_desc(synth.random_desc(r, 1)) == 0


@pytest.mark.parametrize("seed,max_obs,ties", [(0, 8, False), (1, 8, True), (2, 40, False), (3, 3, True)])
def test_median_descriptor_batched_vs_numpy(seed, max_obs, ties):
    d, off = synth.landmark_desc_lists(_rng(60 + seed), 300, max_obs=max_obs, empty_frac=0.05, ties=ties)
    idx, md = O.median_desc_batched(d, off)
    for l in range(300):
        lst = d[off[l]:off[l + 1]]
        if lst.shape[0] == 0:
            assert idx[l] == -1 and not md[l].any()
            continue
        assert idx[l] == O.np_median_desc(lst) == O.median_desc(lst)
        np.testing.assert_array_equal(md[l], lst[idx[l]])
    if ties:
        # tie stress really produces rows with equal medians (first row must win)
        assert any(len(set(map(bytes, d[off[l]:off[l + 1]]))) < off[l + 1] - off[l] for l in range(300))


# ---------------------------------------------------------------- SE(3) --------------------
def test_se3_helpers():
    r = _rng(4)
    for _ in range(20):
        x = np.concatenate([r.standard_normal(3), 0.5 * r.standard_normal(3)])
        T = O.expmap_se3(x)
        assert np.allclose(T, synth.se3_exp(x), atol=1e-14)
        assert np.allclose(T[:3, :3] @ T[:3, :3].T, np.eye(3), atol=1e-12)
        assert np.allclose(O.inverse_se3(T) @ T, np.eye(4), atol=1e-12)
        assert np.allclose(O.logmap_se3(T), x, atol=1e-9)
    assert np.allclose(O.expmap_se3(np.array([1, 2, 3, 0, 0, 0.0])), synth.se3_exp([1, 2, 3, 0, 0, 0]))


# ---------------------------------------------------------------- LBA rows ------------------
def _np_point_row(K, th, T, X, uv):
    """Independent numpy restatement of src/mapHandler.cpp:1368-1407."""
    Ti = np.linalg.inv(T.reshape(4, 4))
    R, t = Ti[:3, :3], Ti[:3, 3]
    g = R @ X + t
    p = np.array([K["cx"] + K["fx"] * g[0] / g[2], K["cy"] + K["fy"] * g[1] / g[2]])
    e = uv - p
    r = np.linalg.norm(e)
    k = 1.0 / max(th, g[2] ** 2)
    a, b = K["fx"] * e[0], K["fy"] * e[1]
    gx, gy, gz = g
    Jc = k * np.array([a * gz, b * gz, -(a * gx + b * gy), -(a * gx * gy + b * gy * gy + b * gz * gz),
                       a * gx * gx + a * gz * gz + b * gx * gy, b * gx * gz - a * gy * gz])
    return Jc / max(th, r), (Jc[:3] @ R) / max(th, r), r, 1.0 / (1.0 + r * r)


def test_point_rows_vs_numpy_restatement():
    lm = synth.local_map(n_kf=5, n_pt=300, n_ls=0, obs_per_lm=3)
    cam = O.make_cam(**synth.EUROC)
    Jp, Jl, r, w = O.lba_point_rows(cam, 1e-7, lm["T_kf_w"], lm["Xw"], lm["obs_uv"], lm["pt_lm"], lm["pt_kf"])
    for o in range(0, 900, 7):
        eJp, eJl, er, ew = _np_point_row(synth.EUROC, 1e-7, lm["T_kf_w"][lm["pt_kf"][o]],
                                         lm["Xw"][lm["pt_lm"][o]], lm["obs_uv"][o])
        assert np.allclose(Jp[o], eJp, rtol=1e-9) and np.allclose(Jl[o], eJl, rtol=1e-9)
        assert np.isclose(r[o], er, rtol=1e-12) and np.isclose(w[o], ew, rtol=1e-12)


def test_point_rows_finite_differences():
    """Pins the [RECALL] helpers: J_lm == -dr/dXw, J_pose == -dr/d(delta) under the reference's
    update rule T <- T * inverse(expmap(delta)) (src/mapHandler.cpp:1563), tangent order [t, w]."""
    lm = synth.local_map(n_kf=3, n_pt=40, n_ls=0, obs_per_lm=2, noise_px=3.0)
    cam = O.make_cam(**synth.EUROC)
    args = (lm["T_kf_w"], lm["Xw"], lm["obs_uv"], lm["pt_lm"], lm["pt_kf"])
    Jp, Jl, r, _ = O.lba_point_rows(cam, 1e-7, *args)
    h = 1e-6
    for o in range(0, 80, 5):
        l, k = lm["pt_lm"][o], lm["pt_kf"][o]
        for j in range(3):
            Xp, Xm = lm["Xw"].copy(), lm["Xw"].copy()
            Xp[l, j] += h
            Xm[l, j] -= h
            rp = O.lba_point_rows(cam, 1e-7, lm["T_kf_w"], Xp, *args[2:])[2][o]
            rm = O.lba_point_rows(cam, 1e-7, lm["T_kf_w"], Xm, *args[2:])[2][o]
            assert np.isclose(Jl[o, j], -(rp - rm) / (2 * h), rtol=2e-4, atol=1e-6)
        for j in range(6):
            d = np.zeros(6)
            d[j] = h
            Tp, Tm = lm["T_kf_w"].copy(), lm["T_kf_w"].copy()
            T0 = lm["T_kf_w"][k].reshape(4, 4)
            Tp[k] = (T0 @ O.inverse_se3(O.expmap_se3(d))).reshape(16)
            Tm[k] = (T0 @ O.inverse_se3(O.expmap_se3(-d))).reshape(16)
            rp = O.lba_point_rows(cam, 1e-7, Tp, *args[1:])[2][o]
            rm = O.lba_point_rows(cam, 1e-7, Tm, *args[1:])[2][o]
            assert np.isclose(Jp[o, j], -(rp - rm) / (2 * h), rtol=2e-4, atol=1e-5)


def _np_line_row(K, th, T, P, Q, l):
    Ti = np.linalg.inv(T.reshape(4, 4))
    R, t = Ti[:3, :3], Ti[:3, 3]

    def proj(g):
        return np.array([K["cx"] + K["fx"] * g[0] / g[2], K["cy"] + K["fy"] * g[1] / g[2]])
    Pc, Qc = R @ P + t, R @ Q + t
    p, q = proj(Pc), proj(Qc)
    e0, e1 = l[0] * p[0] + l[1] * p[1] + l[2], l[0] * q[0] + l[1] * q[1] + l[2]
    r = np.hypot(e0, e1)
    a, b = K["fx"] * e0, K["fy"] * e1          # sic (:1469-1472)

    def j6(g):
        k = 1.0 / max(th, g[2] ** 2)
        gx, gy, gz = g
        return k * np.array([a * gz, b * gz, -(a * gx + b * gy), -(a * gx * gy + b * gy * gy + b * gz * gz),
                             a * gx * gx + a * gz * gz + b * gx * gy, b * gx * gz - a * gy * gz])
    JP, JQ = j6(Pc), j6(Qc)
    den = max(th, r)
    return (JP * e0 + JQ * e1) / den, np.concatenate([(JP[:3] @ R) * e0 / den, (JQ[:3] @ R) * e1 / den]), \
        r, 1.0 / (1.0 + r * r)


def test_line_rows_vs_numpy_restatement_and_compat():
    lm = synth.local_map(n_kf=5, n_pt=0, n_ls=120, obs_per_lm=3)
    cam = O.make_cam(**synth.EUROC)
    Jp, Jl, r, w = O.lba_line_rows(cam, 1e-7, lm["T_kf_w"], lm["Lw"], lm["l_obs"], lm["ls_lm"], lm["ls_kf"])
    cJp, cJl, cr, cw = O.lba_line_rows(cam, 1e-3, lm["T_kf_w"], lm["Lw"], lm["l_obs"], lm["ls_lm"],
                                       lm["ls_kf"], compat_iter_pass=True)
    flat = lm["Lw"].reshape(-1)
    for o in range(0, 360, 5):
        T = lm["T_kf_w"][lm["ls_kf"][o]]
        L = lm["Lw"][lm["ls_lm"][o]]
        e = _np_line_row(synth.EUROC, 1e-7, T, L[:3], L[3:], lm["l_obs"][o])
        for got, exp in zip((Jp[o], Jl[o], r[o], w[o]), e):
            assert np.allclose(got, exp, rtol=1e-9, atol=1e-300)
        # iteration-pass quirk (:1678-1679): P = Q = X[3*lm_loc .. +3]; threshold is the literal 1e-7
        Pq = flat[3 * lm["ls_lm"][o]: 3 * lm["ls_lm"][o] + 3]
        e = _np_line_row(synth.EUROC, 1e-7, T, Pq, Pq, lm["l_obs"][o])
        for got, exp in zip((cJp[o], cJl[o], cr[o], cw[o]), e):
            assert np.allclose(got, exp, rtol=1e-9, atol=1e-300)


def test_rows_degenerate_thresholds():
    """z^2 < homog_th and r < homog_th branches (:1383, :1398)."""
    cam = O.make_cam(**synth.EUROC)
    T = np.eye(4).reshape(1, 16)
    X = np.array([[0.0, 0.0, 1e-5], [0.1, -0.2, 5.0]])
    uv_exact = np.array([[synth.EUROC["cx"], synth.EUROC["cy"]],
                         [synth.EUROC["cx"] + synth.EUROC["fx"] * 0.1 / 5.0,
                          synth.EUROC["cy"] + synth.EUROC["fy"] * -0.2 / 5.0]])
    Jp, Jl, r, w = O.lba_point_rows(cam, 1e-7, T, X, uv_exact, [0, 1], [0, 0])
    assert r[0] == 0.0 and w[0] == 1.0 and np.all(np.isfinite(Jp)) and np.all(np.isfinite(Jl))
    assert abs(r[1]) < 1e-12 and np.all(Jp[1] == Jp[1])


def test_accumulate_matches_numpy():
    lm = synth.local_map(n_kf=4, n_pt=30, n_ls=10, obs_per_lm=3)
    cam = O.make_cam(**synth.EUROC)
    nkf, npt, nls = 3, 30, 10                     # KF 0 is not optimised: kf_loc = slot-1 (or -1)
    kf_loc_p = lm["pt_kf"] - 1
    kf_loc_l = lm["ls_kf"] - 1
    rows_p = O.lba_point_rows(cam, 1e-7, lm["T_kf_w"], lm["Xw"], lm["obs_uv"], lm["pt_lm"], lm["pt_kf"])
    rows_l = O.lba_line_rows(cam, 1e-7, lm["T_kf_w"], lm["Lw"], lm["l_obs"], lm["ls_lm"], lm["ls_kf"])
    H, g, e1 = O.lba_accumulate("points", nkf, npt, nls, lm["pt_lm"], kf_loc_p, *rows_p)
    H, g, e2 = O.lba_accumulate("lines", nkf, npt, nls, lm["ls_lm"], kf_loc_l, *rows_l, H=H, g=g)
    N = 6 * nkf + 3 * npt + 6 * nls
    He, ge, ee = np.zeros((N, N)), np.zeros(N), 0.0
    for (Jp, Jl, r, w), lmi, kfl, base, dl in ((rows_p, lm["pt_lm"], kf_loc_p, 6 * nkf, 3),
                                                (rows_l, lm["ls_lm"], kf_loc_l, 6 * nkf + 3 * npt, 6)):
        for o in range(len(r)):
            J = np.zeros(N)
            J[base + dl * lmi[o]: base + dl * lmi[o] + dl] = Jl[o]
            if kfl[o] >= 0:
                J[6 * kfl[o]: 6 * kfl[o] + 6] = Jp[o]
            He += np.outer(J, J) * w[o]
            ge += J * r[o] * w[o]
            ee += r[o] * r[o] * w[o]
    assert np.allclose(H, He, rtol=1e-10, atol=1e-12) and np.allclose(g, ge, rtol=1e-10, atol=1e-12)
    assert np.isclose(e1 + e2, ee, rtol=1e-12)
    assert np.allclose(H, H.T)


# ---------------------------------------------------------------- gates ---------------------
def test_gates_against_numpy():
    r = _rng(8)
    K = synth.EUROC
    cam = O.make_cam(**K)
    Twf = np.linalg.inv(synth.se3_exp([0.1, -0.05, 0.3, 0.01, 0.02, -0.01]))
    X = np.stack([r.uniform(-3, 3, 200), r.uniform(-2, 2, 200), r.uniform(-1, 20, 200)], 1)
    Xc = X @ Twf[:3, :3].T + Twf[:3, 3]
    with np.errstate(divide="ignore", invalid="ignore"):
        uv = np.stack([K["cx"] + K["fx"] * Xc[:, 0] / Xc[:, 2], K["cy"] + K["fy"] * Xc[:, 1] / Xc[:, 2]], 1)
    vis = O.map_point_visible(cam, Twf, X)
    exp = (uv[:, 0] > 0) & (uv[:, 0] < K["width"]) & (uv[:, 1] > 0) & (uv[:, 1] < K["height"]) & (Xc[:, 2] > 0)
    assert np.array_equal(vis.astype(bool), exp)
    pl = uv[::-1].copy() + r.normal(0, 0.7, uv.shape)
    m12 = np.arange(199, -1, -1, dtype=np.int32)
    m12[::7] = -1
    mask, n = O.map2kf_point_gate(cam, Twf, X, m12, pl, 1.0)
    e = np.zeros(200, bool)
    ok = m12 >= 0
    e[ok] = np.linalg.norm(uv[ok] - pl[m12[ok]], axis=1) < 1.0
    assert np.array_equal(mask.astype(bool), e) and n == e.sum()
    # lines: signed test (:729) -- a large NEGATIVE error passes
    Lw = np.concatenate([X, X + 0.5], 1)
    le = r.normal(0, 1, (200, 3))
    le /= np.linalg.norm(le[:, :2], axis=1, keepdims=True)
    mask, n = O.map2kf_line_gate(cam, Twf, Lw, m12, le, 1.0)
    Ec = Lw[:, 3:] @ Twf[:3, :3].T + Twf[:3, 3]
    with np.errstate(divide="ignore", invalid="ignore"):
        euv = np.stack([K["cx"] + K["fx"] * Ec[:, 0] / Ec[:, 2], K["cy"] + K["fy"] * Ec[:, 1] / Ec[:, 2]], 1)
        l = le[np.clip(m12, 0, None)]
        e0 = l[:, 0] * uv[:, 0] + l[:, 1] * uv[:, 1] + l[:, 2]
        e1 = l[:, 0] * euv[:, 0] + l[:, 1] * euv[:, 1] + l[:, 2]
    e = ok & (e0 < 1.0) & (e1 < 1.0)
    assert np.array_equal(mask.astype(bool), e) and n == e.sum()
    assert (e & ((e0 < -5) | (e1 < -5))).any()   # the signed quirk is exercised


# ---------------------------------------------------------------- committed LBA goldens -----
LBA_GOLD = os.path.join(os.path.dirname(__file__), "golden", "lba_golden.npz")


def test_lba_golden_matches_oracle():
    """The committed fixtures (tests/golden/make_lba_golden.py) are what the oracle produces today."""
    g = np.load(LBA_GOLD)
    cam = O.make_cam(**synth.EUROC)
    lm = {k[4:]: g[k] for k in g.files if k.startswith("map/")}
    rows = O.lba_point_rows(cam, 1e-7, lm["T_kf_w"], lm["Xw"], lm["obs_uv"], lm["pt_lm"], lm["pt_kf"])
    for nm, a in zip(("J_pose", "J_lm", "r", "w"), rows):
        assert np.array_equal(a, g[f"rows/pt/{nm}"])
    rows = O.lba_line_rows(cam, 1e-3, lm["T_kf_w"], lm["Lw"], lm["l_obs"], lm["ls_lm"], lm["ls_kf"], compat_iter_pass=True)
    for nm, a in zip(("J_pose", "J_lm", "r", "w"), rows):
        assert np.array_equal(a, g[f"rows/ls_compat/{nm}"])
    for kind in ("points", "lines"):
        s = {k.split("/")[2]: g[k] for k in g.files if k.startswith(f"drv/{kind}/")}
        m, n = O.map2kf_match(kind, cam, s["Twf"], s["LM"], s["med"], s["cand"], s["kf_desc"], s["kf_feat"], s["kf_idx"],
                              0.9, True, 1.0, 10)
        assert np.array_equal(m, s["map_to_kf"]) and n == int(s["n"][0])


# ---------------------------------------------------------------- LBD binarisation ---------
REF_LBD_SRC = "/root/reference/3rdparty/line_descriptor/src/binary_descriptor_custom.cpp"
LBD_GOLD = os.path.join(os.path.dirname(__file__), "golden", "lbd_golden.npz")


def test_lbd_pair_table_structure():
    pr = O.lbd_pairs()
    assert pr.shape == (32, 2)
    rule = [(a, b) for a in range(9) for b in range(a + 1, 9) if not (a <= 1 and b >= 7)]
    assert [tuple(x) for x in pr.tolist()] == rule


def test_lbd_pair_table_pinned_to_reference_source():
    """Parses combinations[32][2] out of the reference's own source text (this container only)."""
    if not os.path.exists(REF_LBD_SRC):
        pytest.skip("/root/reference not present")
    import re
    txt = open(REF_LBD_SRC).read()
    m = re.search(r"combinations\[32\]\[2\]\s*=\s*\{(.*?)\};", txt, re.S)
    assert m, "combinations table not found"
    ref = [(int(a), int(b)) for a, b in re.findall(r"\{\s*(\d+)\s*,\s*(\d+)\s*\}", m.group(1))]
    assert len(ref) == 32
    assert ref == [tuple(x) for x in O.lbd_pairs().tolist()]
    # the conversion itself: strict '>' and weight 2^i, as the source states
    body = re.search(r"BinaryDescriptor::binaryConversion\(.*?\)\s*\{(.*?)return result", txt, re.S).group(1)
    assert "f1[i] > f2[i]" in body and "get2Pow( i )" in body
    assert "NUM_OF_BANDS 9" in txt


def test_lbd_binary_conversion_known_answers():
    f1 = np.array([1, 0, 1, 0, 1, 0, 1, 0], np.float32)
    f0 = np.zeros(8, np.float32)
    bc = lambda a, b: int(O.lib().plo_lbd_binary_conversion(a.ctypes.data, b.ctypes.data))
    assert bc(f1, f0) == 0b01010101
    assert bc(f0, f1) == 0
    assert bc(1 - f1, f1) == 0b10101010
    assert bc(f1, f1) == 0                                   # equality is not '>'
    e = np.zeros(8, np.float32)
    e[7] = 1
    assert bc(e, f0) == 128
    nan = np.full(8, np.nan, np.float32)
    assert bc(nan, f0) == 0 and bc(f0, nan) == 0             # unordered compares are false
    assert bc(np.full(8, np.inf, np.float32), np.full(8, 3.0e38, np.float32)) == 255
    assert bc(np.zeros(8, np.float32), np.full(8, -0.0, np.float32)) == 0   # +0 > -0 is false


@pytest.mark.parametrize("n,levels", [(0, 0), (1, 0), (31, 4), (32, 0), (33, 16), (1000, 8)])
def test_lbd_binarise_c_vs_numpy(n, levels):
    f = synth.lbd_float(_rng(40 + n), n, levels)
    got = O.lbd_binarise(f)
    assert got.shape == (n, 32)
    np.testing.assert_array_equal(got, O.np_lbd_binarise(f))
    if n >= 1000 and levels:
        # quantised rows really exercise the tie rule
        assert (f.reshape(n, 9, 8)[:, 0] == f.reshape(n, 9, 8)[:, 1]).any()


def test_lbd_golden_matches_oracle():
    g = np.load(LBD_GOLD)
    np.testing.assert_array_equal(O.lbd_binarise(g["lbd_f32"]), g["desc_u8"])
    np.testing.assert_array_equal(O.np_lbd_binarise(g["lbd_f32"]), g["desc_u8"])


# ---------------------------------------------------------------- LBD pinned to reference code ----
@pytest.mark.parametrize("width,height,n,wob,seed", [(320, 240, 300, 7, 0), (752, 480, 400, 7, 1), (200, 100, 200, 5, 2),
                                                     (640, 480, 200, 9, 3)])
def test_lbd_compute_pinned_to_reference_code(width, height, n, wob, seed):
    """oracle/_ref holds the reference's own BinaryDescriptor::computeLBD (binary_descriptor_custom.cpp:1026-1372,
    compiled from where it lies; oracle/ref_wrap_lbd.cpp hands it the gradient images computeSobel would have left in
    dxImg_vector / dyImg_vector).  The oracle's restatement must reproduce its 72 floats per line BIT FOR BIT --
    segments reaching past the image border (clamping) and three band widths included."""
    r = _rng(7000 + seed)
    dx, dy = synth.gradient_images(r, width, height)
    lines = synth.lbd_lines(r, n, width, height, dtype=O.LBD_LINE_DTYPE)
    ref = _reference(f"lbd_compute/{seed}", lambda: O.ref_lbd_compute(dx, dy, lines, wob))
    got = O.lbd_compute(dx, dy, lines, wob)
    assert not np.isnan(ref).any()
    assert np.array_equal(got.view(np.uint32), ref.view(np.uint32))
    # and the 32-byte binary rows built from them (computeImpl :653-668) follow
    assert np.array_equal(O.lbd_binarise(got), O.lbd_binarise(ref))


def test_lbd_tables_and_binary_conversion_pinned_to_reference_code():
    """The constructor's Gaussian weight tables (:217-259) and binaryConversion (:401-412) of the compiled reference."""
    for wob in (3, 5, 7, 9, 12):
        cl, cg = O.lbd_gauss_tables(wob)
        rl, rg = _reference(f"lbd_gauss_tables/{wob}", lambda: O.ref_lbd_gauss_tables(wob))
        assert np.array_equal(cl, rl) and np.array_equal(cg, rg)
    r = _rng(7100)
    f = r.integers(0, 4, (500, 2, 8)).astype(np.float32)     # small integers: plenty of equal pairs (strict >)
    f1, f2 = np.ascontiguousarray(f[:, 0]), np.ascontiguousarray(f[:, 1])
    live = lambda: (None if O.ref_lbd_gauss_tables(7) is None else                            # noqa: E731
                    np.array([O.ref_lbd_binary_conversion(f1[i], f2[i]) for i in range(500)], np.int32))
    R = _reference("lbd_binary_conversion", live)
    for i in range(500):
        assert int(O.lib().plo_lbd_binary_conversion(f1[i].ctypes.data, f2[i].ctypes.data)) == R[i]


# ---------------------------------------------------------------- median descriptor pinned to reference code ----
def test_median_descriptor_pinned_to_reference_code():
    """oracle/_ref holds the reference's own MapPoint / MapLine::updateAverageDescDir (src/mapFeatures.cpp:51-93,
    :121-163; mapFeatures.cpp compiled from where it lies against cv:: / Eigen stand-ins).  The landmark is built the
    way the map builds it -- first observation through the constructor, the rest through add*Observation -- and the
    observation that ends up as med_desc must be the one the oracle (and the kernel, test_gpu_median_desc.py) names:
    1 .. 13 observations, tie-heavy rows, duplicated observations (first minimum wins)."""
    cases = []
    for seed in range(400):
        r = _rng(8000 + seed)
        n = int(r.integers(1, 14))
        d = synth.tie_stress_desc(r, n) if seed % 3 == 0 else synth.random_desc(r, n)
        if seed % 5 == 0 and n > 2:
            d[int(r.integers(1, n))] = d[0]
        cases.append(d)
    live = lambda: (None if O.ref_median_desc(np.zeros((1, 32), np.uint8)) is None else              # noqa: E731
                    np.array([[O.ref_median_desc(d, "point"), O.ref_median_desc(d, "line")] for d in cases], np.int32))
    R = _reference("median_desc", live)
    for seed, d in enumerate(cases):
        exp = O.median_desc(d)
        assert R[seed, 0] == exp, (seed, len(d))
        assert R[seed, 1] == exp, (seed, len(d))


# ---------------------------------------------------------------- LBA rows + accumulation pinned to the source text ----
def _lba_oracle_Hg(cam, th, nkf, npt, nls, T, lm, kf_slot_p, kf_slot_l, kf_loc_p, kf_loc_l, compat):
    rows_p = O.lba_point_rows(cam, th, T, lm["Xw"], lm["obs_uv"], lm["pt_lm"], kf_slot_p)
    rows_l = O.lba_line_rows(cam, th, T, lm["Lw"], lm["l_obs"], lm["ls_lm"], kf_slot_l, compat_iter_pass=compat)
    H, g, e1 = O.lba_accumulate("points", nkf, npt, nls, lm["pt_lm"], kf_loc_p, *rows_p)
    H, g, e2 = O.lba_accumulate("lines", nkf, npt, nls, lm["ls_lm"], kf_loc_l, *rows_l, H=H, g=g)
    return H, g, e1 + e2


@pytest.mark.parametrize("th", [1e-7, 0.3, 30.0])
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_lba_rows_and_accumulation_pinned_to_reference_source_text(seed, th):
    """oracle/_ref compiles the reference's four local-BA observation loops TEXTUALLY (cut out of
    src/mapHandler.cpp:1358-1431, :1436-1540, :1587-1666, :1668-1772 where the file lies; Eigen spellings served by the
    plain-loop stand-in oracle/ref_shim/mini_dense.hpp, the un-vendored stvo-pl helpers restated).  H, g and err after
    the reference's loops must equal the oracle's rows + accumulation: first pass, and the iteration pass with its
    quirks (line end points both read at stride 3, the literal 1e-7, lines keep the un-updated key-frame pose while
    points take expmap(X)).  th = 0.3 puts some residual norms, th = 30 some depths (z^2) below the threshold: both std::max(homogTh, .) branches.  Tolerance 1e-11
    relative: the stand-in is not Eigen, rounding of the 3-term sums may differ in the last bit."""
    n_kf, npt, nls = 5, 40, 14
    lm = synth.local_map(n_kf=n_kf, n_pt=npt, n_ls=nls, obs_per_lm=3, seed=70 + seed, noise_px=2.0)
    cam = O.make_cam(**synth.EUROC)
    nkf = n_kf - 1                                 # KF 0 is not optimised
    kf_loc_p, kf_loc_l = lm["pt_kf"] - 1, lm["ls_kf"] - 1
    T_map = np.asarray(lm["T_kf_w"]).reshape(n_kf, 16)
    r = _rng(500 + seed)
    T_slot = np.stack([(synth.se3_exp(r.normal(0, 0.02, 6)) @ T_map[k + 1].reshape(4, 4)).reshape(16) for k in range(nkf)])
    first = O.ref_lba_accumulate(False, cam, th, nkf, T_map, T_slot, lm["Xw"], lm["Lw"], lm["pt_lm"], lm["pt_kf"], kf_loc_p,
                                 lm["obs_uv"], lm["ls_lm"], lm["ls_kf"], kf_loc_l, lm["l_obs"])
    if first is None:
        pytest.skip("oracle/_ref not built with the LBA harness (needs /root/reference at build time)")
    H, g, e = _lba_oracle_Hg(cam, th, nkf, npt, nls, T_map, lm, lm["pt_kf"], lm["ls_kf"], kf_loc_p, kf_loc_l, False)
    scale = np.abs(H).max()
    assert scale > 0 and np.abs(g).max() > 0
    np.testing.assert_allclose(first[0], H, rtol=1e-11, atol=1e-11 * scale)
    np.testing.assert_allclose(first[1], g, rtol=1e-11, atol=1e-11 * np.abs(g).max())
    assert np.isclose(first[2], e, rtol=1e-12)
    # iteration pass: points at expmap(X) for optimised slots, lines at the stored pose and with the stride-3 read
    it = O.ref_lba_accumulate(True, cam, th, nkf, T_map, T_slot, lm["Xw"], lm["Lw"], lm["pt_lm"], lm["pt_kf"], kf_loc_p,
                              lm["obs_uv"], lm["ls_lm"], lm["ls_kf"], kf_loc_l, lm["l_obs"])
    T_all = np.concatenate([T_map, T_slot])
    slot_p = np.where(kf_loc_p >= 0, n_kf + kf_loc_p, lm["pt_kf"]).astype(np.int32)
    H2, g2, e2 = _lba_oracle_Hg(cam, th, nkf, npt, nls, T_all, lm, slot_p, lm["ls_kf"], kf_loc_p, kf_loc_l, True)
    scale2 = np.abs(H2).max()
    np.testing.assert_allclose(it[0], H2, rtol=1e-11, atol=1e-11 * scale2)
    np.testing.assert_allclose(it[1], g2, rtol=1e-11, atol=1e-11 * np.abs(g2).max())
    assert np.isclose(it[2], e2, rtol=1e-12)
    assert not np.allclose(it[0], first[0], rtol=1e-6, atol=1e-6 * scale)       # the two passes really differ


@pytest.mark.parametrize("robust", [False, True])
@pytest.mark.parametrize("th", [1e-7, 0.5, 60.0])
def test_pose_gn_loops_pinned_to_reference_source_text(robust, th):
    """K17's checker against the reference's own pose-only Gauss-Newton loops, compiled textually from
    src/mapHandler.cpp:3331-3426 (computeRelativePoseGN) and :3595-3689 (computeRelativePoseRobustGN): H = H_p + H_l,
    g, e and the inlier counts of one iteration.  th = 0.5 / 60 put residual norms / depths below homogTh."""
    from test_pose_gn import scene, _args
    cam = O.make_cam(**synth.EUROC)
    for seed in (2, 3, 4):
        sc = scene(120, 40, seed=seed)
        ref = _reference(f"pose_gn/{int(robust)}/{th!r}/{seed}", lambda: O.ref_pose_gn_accumulate(robust, cam, th, *_args(sc)))
        H, g, e, n = O.pose_gn_accumulate(cam, th, *_args(sc))
        assert n == ref[3] and n[0] > 50 and n[1] > 15
        np.testing.assert_allclose(ref[0], H, rtol=1e-11, atol=1e-11 * np.abs(H).max())
        np.testing.assert_allclose(ref[1], g, rtol=1e-11, atol=1e-11 * np.abs(g).max())
        assert np.isclose(ref[2], e, rtol=1e-12)


def test_map2kf_visibility_and_gates_pinned_to_reference_source_text():
    """The loops either side of the descriptor match in matchMap2KFPoints / matchMap2KFLines, compiled textually from
    src/mapHandler.cpp:545-558, :601-629, :647-663, :716-749: which landmarks the visibility pre-filter selects (and the
    normalised projections it records for the grid search), which landmarks pass the geometric gate (points: norm of
    the pixel error; lines: the SIGNED two-end-point test) and the final `matches` count."""
    K = synth.EUROC
    cam = O.make_cam(**K)
    checked = 0
    for seed in range(4):
        r = _rng(300 + seed)
        Twf = np.linalg.inv(synth.se3_exp(r.normal(0, 0.08, 6)))
        n = 300
        X = np.stack([r.uniform(-4, 4, n), r.uniform(-3, 3, n), r.uniform(-2, 20, n)], 1)
        X[0, 2] = -Twf[2, 3] / max(abs(Twf[2, 2]), 1e-9) * np.sign(Twf[2, 2])        # a landmark at (almost) zero depth
        ref = _reference(f"map_visible/points/{seed}",
                         lambda: O.ref_map_visible("points", cam, Twf, X, 1.0 / K["width"], 1.0 / K["height"]))
        vis = O.map_point_visible(cam, Twf, X)
        assert np.array_equal(vis, ref[0]) and 20 < vis.sum() < n
        Xc = X @ Twf[:3, :3].T + Twf[:3, 3]
        uv = np.stack([K["cx"] + K["fx"] * Xc[:, 0] / Xc[:, 2], K["cy"] + K["fy"] * Xc[:, 1] / Xc[:, 2]], 1)
        sel = vis.astype(bool)
        np.testing.assert_allclose(ref[1], uv[sel] * [1.0 / K["width"], 1.0 / K["height"]], rtol=1e-12)
        Lw = np.concatenate([X, X + r.normal(0, 0.4, X.shape)], 1)
        refl = _reference(f"map_visible/lines/{seed}",
                          lambda: O.ref_map_visible("lines", cam, Twf, Lw, 1.0 / K["width"], 1.0 / K["height"]))
        visl = O.map_line_visible(cam, Twf, Lw)
        assert np.array_equal(visl, refl[0]) and 10 < visl.sum() < n
        # gates on the visible ones
        Xv, Lv = X[sel], Lw[visl.astype(bool)]
        nt = 150
        m12 = r.integers(-1, nt, len(Xv)).astype(np.int32)
        pl = np.zeros((nt, 2))
        ok = m12 >= 0
        pl[m12[ok]] = uv[sel][ok]
        pl += r.normal(0, 0.8, pl.shape)
        for th in (1.0, 2.5):
            mask, cnt = O.map2kf_point_gate(cam, Twf, Xv, m12, pl, th)
            rmask, rcnt = _reference(f"map2kf_gate/points/{seed}/{th!r}", lambda: O.ref_map2kf_gate("points", cam, Twf, Xv, m12, pl, th))
            assert np.array_equal(mask, rmask) and cnt == rcnt and 0 < cnt < ok.sum()
            checked += 1
        m12l = r.integers(-1, nt, len(Lv)).astype(np.int32)
        le = r.normal(0, 1, (nt, 3))
        le /= np.linalg.norm(le[:, :2], axis=1, keepdims=True)
        le[:, 2] *= 200.0
        for th in (1.0, 40.0):
            mask, cnt = O.map2kf_line_gate(cam, Twf, Lv, m12l, le, th)
            rmask, rcnt = _reference(f"map2kf_gate/lines/{seed}/{th!r}", lambda: O.ref_map2kf_gate("lines", cam, Twf, Lv, m12l, le, th))
            assert np.array_equal(mask, rmask) and cnt == rcnt
            checked += 1
    assert checked == 16


def test_gba_first_pass_is_the_lba_first_pass_except_for_one_transposed_block():
    """DESIGN.md claims the global-BA rows are the local-BA rows verbatim and only the accumulation is spelt differently
    (SparseMatrix::coeffRef).  Compiling the reference's own GBA loops (src/mapHandler.cpp:2124-2228, :2233-2355) shows
    the claim holds for g, err and every block of H -- EXCEPT the pose x line cross blocks, which the GBA code writes
    transposed (`H.coeffRef(idx+i,jdx+j) += Hij(i,j)` with Hij = J_line J_pose^T, :2341-2352; the local BA puts that
    product at [line rows, pose columns], :1531-1532).  A caller that wants the reference's GBA numbers therefore
    transposes the 6 x 6 W blocks of the line observations it gets from plslam_lba_assemble."""
    n_kf, npt, nls = 5, 40, 14
    lm = synth.local_map(n_kf=n_kf, n_pt=npt, n_ls=nls, obs_per_lm=3, seed=71, noise_px=2.0)
    cam = O.make_cam(**synth.EUROC)
    nkf = n_kf - 1
    kf_loc_p, kf_loc_l = lm["pt_kf"] - 1, lm["ls_kf"] - 1
    T_map = np.asarray(lm["T_kf_w"]).reshape(n_kf, 16)
    args = (cam, 1e-7, nkf, T_map, T_map[1:], lm["Xw"], lm["Lw"], lm["pt_lm"], lm["pt_kf"], kf_loc_p, lm["obs_uv"],
            lm["ls_lm"], lm["ls_kf"], kf_loc_l, lm["l_obs"])
    gba = O.ref_lba_accumulate("gba", *args)
    if gba is None:
        pytest.skip("oracle/_ref not built with the LBA harness (needs /root/reference at build time)")
    H, g, e = _lba_oracle_Hg(cam, 1e-7, nkf, npt, nls, T_map, lm, lm["pt_kf"], lm["ls_kf"], kf_loc_p, kf_loc_l, False)
    tol = 1e-11 * np.abs(H).max()
    np.testing.assert_allclose(gba[1], g, rtol=1e-11, atol=1e-11 * np.abs(g).max())
    assert np.isclose(gba[2], e, rtol=1e-12)
    base = 6 * nkf + 3 * npt
    exp = H.copy()
    for k in range(nkf):
        for l in range(nls):
            blk = H[base + 6 * l: base + 6 * l + 6, 6 * k: 6 * k + 6]          # [line rows, pose cols] = J_line J_pose^T
            exp[6 * k: 6 * k + 6, base + 6 * l: base + 6 * l + 6] = blk         # GBA: the same numbers, untransposed
            exp[base + 6 * l: base + 6 * l + 6, 6 * k: 6 * k + 6] = blk.T
    np.testing.assert_allclose(gba[0], exp, rtol=1e-11, atol=tol)
    assert not np.allclose(gba[0], H, rtol=1e-9, atol=1e-9 * np.abs(H).max())   # ... and that is a real difference


def test_lba_against_committed_reference_source_text_outputs():
    """tests/golden/lba_ref_golden.npz (H, g, err from the reference's own loops, make_lba_ref_golden.py) against the
    oracle -- runs where oracle/_ref was never built."""
    g = np.load(os.path.join(os.path.dirname(__file__), "golden", "lba_ref_golden.npz"))
    n_kf, nkf, npt, nls = (int(x) for x in g["dims"])
    cam = O.make_cam(**synth.EUROC)
    lm = {k: g[k] for k in ("Xw", "Lw", "obs_uv", "l_obs", "pt_lm", "pt_kf", "ls_lm", "ls_kf")}
    kp, kl = g["pt_kf"] - 1, g["ls_kf"] - 1
    th = float(g["th"][0])
    H, gg, e = _lba_oracle_Hg(cam, th, nkf, npt, nls, g["T_map"], lm, g["pt_kf"], g["ls_kf"], kp, kl, False)
    np.testing.assert_allclose(g["first_H"], H, rtol=1e-11, atol=1e-11 * np.abs(H).max())
    np.testing.assert_allclose(g["first_g"], gg, rtol=1e-11, atol=1e-11 * np.abs(gg).max())
    assert np.isclose(float(g["first_err"][0]), e, rtol=1e-12)
    T_all = np.concatenate([g["T_map"], g["T_slot"]])
    slot_p = np.where(kp >= 0, n_kf + kp, g["pt_kf"]).astype(np.int32)
    H, gg, e = _lba_oracle_Hg(cam, th, nkf, npt, nls, T_all, lm, slot_p, g["ls_kf"], kp, kl, True)
    np.testing.assert_allclose(g["iter_H"], H, rtol=1e-11, atol=1e-11 * np.abs(H).max())
    np.testing.assert_allclose(g["iter_g"], gg, rtol=1e-11, atol=1e-11 * np.abs(gg).max())
    assert np.isclose(float(g["iter_err"][0]), e, rtol=1e-12)


def test_visibility_gates_median_against_committed_reference_outputs():
    """tests/golden/map2kf_ref_golden.npz (outputs of the reference's own loops, make_map2kf_ref_golden.py) against the
    oracle -- runs where oracle/_ref was never built."""
    g = np.load(os.path.join(os.path.dirname(__file__), "golden", "map2kf_ref_golden.npz"))
    cam = O.make_cam(**synth.EUROC)
    vp, vl = O.map_point_visible(cam, g["Twf"], g["X"]), O.map_line_visible(cam, g["Twf"], g["Lw"])
    assert np.array_equal(vp, g["vis_p"]) and np.array_equal(vl, g["vis_l"])
    Xv, Lv = g["X"][vp.astype(bool)], g["Lw"][vl.astype(bool)]
    for k, th in enumerate(g["th_p"]):
        mask, cnt = O.map2kf_point_gate(cam, g["Twf"], Xv, g["m12p"], g["pl"], float(th))
        assert np.array_equal(mask, g[f"gate_p{k}"]) and cnt == int(g[f"count_p{k}"][0])
    for k, th in enumerate(g["th_l"]):
        mask, cnt = O.map2kf_line_gate(cam, g["Twf"], Lv, g["m12l"], g["le"], float(th))
        assert np.array_equal(mask, g[f"gate_l{k}"]) and cnt == int(g[f"count_l{k}"][0])
    idx, md = O.median_desc_batched(g["med_desc_lists"], g["med_offsets"])
    assert np.array_equal(idx, g["med_idx"])


def test_lm_loop_fixture_is_what_the_references_text_computes():
    """tests/golden/lba_lm_golden.npz (the fixture the GPU test of LbaPlanSolver::optimize is checked against) re-generated here
    from the reference's own LM text (oracle/ref_wrap_lba_lm.cpp compiles src/mapHandler.cpp:1334-1812 where it lies): same
    inputs, same trajectory, bit for bit -- and the trajectory shows the reference's quirks: a first err of +inf (the counters of
    :1541 are never incremented), lambda multiplied by lambda_k after every accepted step, a rejected step followed by a stop."""
    import importlib.util
    if O.ref_lib() is None or not hasattr(O.ref_lib(), "ref_lba_lm"):
        pytest.skip("oracle/_ref not built (no /root/reference here)")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("make_lba_lm_golden", os.path.join(root, "tests", "golden", "make_lba_lm_golden.py"))
    M = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(M)
    g = np.load(os.path.join(root, "tests", "golden", "lba_lm_golden.npz"))
    for name, args in M.CASES.items():
        p = M.problem(**args)
        for k, v in p.items():
            assert np.array_equal(np.asarray(v), g[f"{name}_{k}"]), (name, k)
        r = M.run_ref(p)
        for k, v in r.items():
            assert np.array_equal(np.asarray(v), g[f"{name}_ref_{k}"], equal_nan=True), (name, k)
        e, lam = r["err"], r["lam"]
        assert np.isinf(e[0]) and lam[1] == lam[0]
        for i in range(2, len(e)):
            assert lam[i] == (lam[i - 1] / 10.0 if (i - 1 >= 1 and e[i - 1] > e[i - 2]) else lam[i - 1] * 10.0)
    e = g["reject_ref_err"]
    assert e[2] > e[1] and int(g["reject_ref_iters"]) == 3 and float(g["reject_ref_err_last"]) == e[2]
