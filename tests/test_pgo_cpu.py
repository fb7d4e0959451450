"""CPU tests of the loop-closure correction's restatement (tests/pgo_ref.py) and generator (plslam_amd/pgo.py): the g2o maps,
the exact Jacobians, the BFS initial guess, the graph against the reference's loops and text, and the optimiser's behaviour."""
import os

import numpy as np
import pytest

from plslam_amd import pgo

import pgo_ref as R
from gba_ref import expmap_se3, inverse_se3, logmap_se3

REF_SRC = "/root/reference/src/mapHandler.cpp"


def _rand_iso(rng, scale=1.0):
    return R.se3quat_exp(np.concatenate([scale * rng.standard_normal(3), rng.standard_normal(3)]))


@pytest.mark.parametrize("rot_scale", [1.0, 1e-3, 1e-7])
def test_jacobians_equal_central_differences(rot_scale):
    rng = np.random.Generator(np.random.PCG64(1))
    for _ in range(20):
        Z, Xi, Xj = (_rand_iso(rng, rot_scale) for _ in range(3))
        Ji, Jj = R.edge_jacobians(Z, Xi, Xj)
        h = 1e-6
        for which, J in ((0, Ji), (1, Jj)):
            Jn = np.zeros((6, 6))
            for k in range(6):
                d = np.zeros(6)
                d[k] = h
                if which == 0:
                    ep = R.edge_error(Z, R.iso_mul(Xi, R.from_vector_mqt(d)), Xj)
                    em = R.edge_error(Z, R.iso_mul(Xi, R.from_vector_mqt(-d)), Xj)
                else:
                    ep = R.edge_error(Z, Xi, R.iso_mul(Xj, R.from_vector_mqt(d)))
                    em = R.edge_error(Z, Xi, R.iso_mul(Xj, R.from_vector_mqt(-d)))
                Jn[:, k] = (ep - em) / (2 * h)
            assert np.abs(J - Jn).max() <= 1e-6 * max(1.0, np.abs(J).max())


def test_exp_branches_and_the_log_quirk():
    # exp: the small-angle branch is R = I + Omega + Omega^2 (re-orthonormalised through the quaternion), V = R
    w = np.array([3e-6, -2e-6, 1e-6])
    Rs, t = R.se3quat_exp(np.concatenate([w, [1.0, 2.0, 3.0]]))
    Om = R.skew(w)
    assert np.allclose(Rs, np.eye(3) + Om + Om @ Om, atol=1e-10)
    assert np.allclose(t, (np.eye(3) + Om + Om @ Om) @ [1.0, 2.0, 3.0], atol=1e-14)
    # above the threshold: Rodrigues, and the log inverts it
    u = np.array([0.3, -0.2, 0.5, 1.0, -2.0, 0.5])
    assert np.allclose(R.se3quat_log(R.se3quat_exp(u)), u, atol=1e-13)
    # exp agrees with stvo's expmap_se3 of the reversed vector
    Rm, tm = R.se3quat_exp(R.reverse_se3(np.array([1.0, -2.0, 0.5, 0.3, -0.2, 0.5])))
    T = expmap_se3([1.0, -2.0, 0.5, 0.3, -0.2, 0.5])
    assert np.allclose(Rm, T[:3, :3], atol=1e-14) and np.allclose(tm, T[:3, 3], atol=1e-14)
    # log's first-order branch just above d = 0.99999 (theta just below acos(0.99999) ~ 4.47e-3): omega = dR / 2 is sin(theta)
    # where theta belongs, so the write-back round trip is off by ~theta^2 / 6 ~ 3e-6 relative; the exact branch is not
    th = np.arccos(0.99999) * 0.999
    u = np.array([th, 0.0, 0.0, 0.0, 1.0, 0.0])
    v = R.se3quat_log(R.se3quat_exp(u))
    rel = abs(v[0] - th) / th
    assert 1e-6 < rel < 1e-5 and rel == pytest.approx(th * th / 6, rel=1e-3)
    u2 = np.array([np.arccos(0.99999) * 1.01, 0.0, 0.0, 0.0, 1.0, 0.0])
    assert np.abs(R.se3quat_log(R.se3quat_exp(u2)) - u2).max() < 1e-12


def test_mqt_vectors():
    rng = np.random.Generator(np.random.PCG64(2))
    for _ in range(10):
        X = _rand_iso(rng)
        v = R.to_vector_mqt(X)
        Y = R.from_vector_mqt(v)
        assert np.allclose(Y[0], X[0], atol=1e-14) and np.allclose(Y[1], X[1])
    Rr, _ = R.from_vector_mqt(np.array([0, 0, 0, 0.9, 0.9, 0.0]))      # |q_xyz| > 1: the identity rotation
    assert np.array_equal(Rr, np.eye(3))


def _graph(n, edges_cov, lc):
    fg = np.zeros((n, n), np.int32)
    for i, j in edges_cov:
        fg[i, j] = fg[j, i] = 100
    return np.ones(n, np.uint8), fg, np.array(lc, np.int32).reshape(-1, 3)


def test_bfs_tree_follows_the_tie_rule():
    # 0-1-2-3 chain (|i-j| == 1 edges), covisibility 0-3 and 1-4 (4 is not consecutive to... 3-4 is), LC (0, 5)
    v, fg, lc = _graph(6, [(0, 3), (1, 4)], [[0, 5, 1]])
    g = R.build_graph(v, fg, lc)
    assert [e[:2] for e in g["edges"]] == [(0, 1), (0, 3), (1, 2), (1, 4), (2, 3), (3, 4), (4, 5), (0, 5)]
    order, level = R.bfs_tree(g)
    # from 0: its incident edges in creation order are (0,1), (0,3), (0,5) -> 1, 3, 5 at level 1; then from 1: 2, 4
    assert [(v_, u) for v_, u, _ in order] == [(1, 0), (3, 0), (5, 0), (2, 1), (4, 1)]
    assert level == {0: 0, 1: 1, 3: 1, 5: 1, 2: 2, 4: 2}
    # the edge direction decides Z or Z^-1: vertex 5 is the second end of (0, 5)
    assert [e for v_, _, e in order if v_ == 5] == [7]


def test_edges_equal_the_references_loops():
    m = pgo.pose_graph(n_kf=40, null_slots=(6, 17), seed=21, extra_lc=((3, 36),))
    g = R.build_graph(m["kf_valid"], m["full_graph"], m["lc_idx"], 75, 75)
    # :4252-4273 spelled out as the reference writes them
    kf_curr = int(m["lc_idx"][:, 1].max())
    want = []
    for i in range(0, kf_curr + 1):
        for j in range(i + 1, kf_curr + 1):
            fg = m["full_graph"][i][j]
            if m["kf_valid"][i] and m["kf_valid"][j] and (fg >= 75 or fg >= 75 or abs(i - j) == 1):
                want.append((i, j))
    want += [(int(a), int(b)) for a, b, _ in m["lc_idx"]]
    assert [e[:2] for e in g["edges"]] == want
    assert g["verts"] == [i for i in range(kf_curr + 1) if m["kf_valid"][i]]
    # near neighbours pass 75, far ones do not
    fgm = m["full_graph"]
    rows = [i for i in range(30) if m["kf_valid"][i] and m["kf_valid"][i + 1]]
    assert (fgm[rows, np.array(rows) + 1] >= 75).all() and (fgm[np.arange(30), np.arange(30) + 5] == 0).all()


def _ref_text():
    if not os.path.exists(REF_SRC):
        pytest.skip("the reference source is not on this machine")
    src = open(REF_SRC).read()
    a = src.index("bool MapHandler::loopClosureOptimizationCovGraphG2O()")
    return src[a:src.index("\n}\n", a)]


def test_the_text_the_restatement_rests_on():
    body = _ref_text()
    # the graph, :4198-4290
    assert "solver->setUserLambdaInit(1e-10);" in body
    assert "kf_prev_idx = 0;" in body
    assert "if( (*it)(1) > kf_curr_idx )" in body
    assert "if( (*it)(0) == i )\n                {\n                    is_lc_i = true;\n                    break;" in body
    assert "if( (*it)(1) == i )\n                {\n                    is_lc_j = true;\n                    break;" in body
    assert ("v_se3->setEstimate( g2o::SE3Quat::exp( reverse_se3(logmap_se3( (expmap_se3(lc_pose_list[id])) * "
            "map_keyframes[lc_idx_list[id](0)]->T_kf_w )) ) );") in body
    assert "v_se3->setEstimate( g2o::SE3Quat::exp( reverse_se3(map_keyframes[i]->x_kf_w) ) );" in body
    assert "if( i == 0 )\n                    v_se3->setFixed(true);" in body
    assert ("( full_graph[i][j] >= SlamConfig::minLMEssGraph() || full_graph[i][j] >= SlamConfig::minLMCovGraph() || "
            "abs(i-j) == 1  )") in body
    assert "Matrix4d T_ji_constraint = inverse_se3( map_keyframes[i]->T_kf_w ) * map_keyframes[j]->T_kf_w;" in body
    assert "x = reverse_se3(logmap_se3(T_ji_constraint) );" in body
    assert "x = reverse_se3( lc_pose_list[id] );" in body
    assert body.count("setInformation( Matrix6d::Identity() )") + body.count("information() = Matrix6d::Identity()") == 2
    assert ("optimizer.initializeOptimization();\n    optimizer.computeInitialGuess();\n    optimizer.computeActiveErrors();\n"
            "    optimizer.optimize(SlamConfig::maxItersPGO());") in body
    # the write-back and the map correction, :4298-4398
    assert "x = reverse_se3(Tiw_corr.log());" in body and "Tkfw = expmap_se3( x );" in body
    assert "map_keyframes[ (*kf_it) ]->x_kf_w = logmap_se3(Tkfw);" in body
    assert "Tkfw_corr = Tkfw * inverse_se3( Tkfw_prev );" in body
    assert body.count("Tkfw_corr.block(0,0,3,3) * obs_dir + Tkfw_corr.block(0,3,3,1);") == 4          # the translation on a direction
    assert body.count("Tkfw_corr.block(0,0,3,3) * dir_list_ + Tkfw_corr.block(0,3,3,1);") == 4
    assert "for( int i = kf_curr_idx + 1; i < map_keyframes.size(); i++ )" in body
    assert "map_keyframes[i]->T_kf_w = Tkfw_corr * map_keyframes[i]->T_kf_w;" in body
    later = body[body.index("for( int i = kf_curr_idx + 1; i < map_keyframes.size(); i++ )"):]
    assert "map_keyframes[i] != NULL" not in later[:later.index("map_keyframes[i]->T_kf_w = Tkfw_corr")]    # no NULL check
    assert "(*it)(2) = 0;" in body and "loopClosureFuseLandmarks();" in body


def test_a_drift_free_graph_stays_put():
    m = pgo.pose_graph(n_kf=40, drift=0.0, lc_noise=0.0, seed=22)
    m["T_kf_w"] = m["T_true"]
    m["x_kf_w"] = np.stack([logmap_se3(T) for T in m["T_true"]])
    m["lc_pose"] = np.stack([logmap_se3(inverse_se3(m["T_true"][a]) @ m["T_true"][b]) for a, b, _ in m["lc_idx"]])
    P = R.Pgo(m["kf_valid"], m["full_graph"], m["lc_idx"])
    r = P.optimize(m["T_kf_w"], m["x_kf_w"], m["lc_pose"])
    assert r["chi_initial"] < 1e-20 and r["chi_final"] < 1e-20
    T_out, _, T_corr, _ = R.write_back(P, r, m["T_kf_w"], m["x_kf_w"])
    assert np.abs(T_out - m["T_kf_w"]).max() < 1e-12


def test_a_drifted_loop_closes():
    m = pgo.pose_graph(n_kf=120, seed=23)
    P = R.Pgo(m["kf_valid"], m["full_graph"], m["lc_idx"])
    r = P.optimize(m["T_kf_w"], m["x_kf_w"], m["lc_pose"])
    T_out, _, _, _ = R.write_back(P, r, m["T_kf_w"], m["x_kf_w"])
    a, b, _ = m["lc_idx"][0]

    def loop_err(T):
        rel = inverse_se3(T[a]) @ T[b]
        return np.linalg.norm(logmap_se3(inverse_se3(expmap_se3(m["lc_pose"][0])) @ rel))

    assert loop_err(T_out) < 0.1 * loop_err(m["T_kf_w"])
    assert r["chi_final"] < 1e-2 * r["chi_initial"]
    assert r["trace"][0]["accepted"] and r["iterations"] >= 2


def test_map_correction_applies_anchors_in_slot_order():
    rng = np.random.Generator(np.random.PCG64(24))
    n = 6
    T_corr = np.stack([np.eye(4)] + [expmap_se3(0.1 * rng.standard_normal(6)) for _ in range(n - 1)])
    corrected = np.array([1, 1, 0, 1, 1, 1], bool)
    lm = pgo.anchored_landmarks(n, 50, seed=25, n_double=5)
    X, med, dirs = R.correct_landmarks(T_corr, corrected, lm["anchor_ptr"], lm["anchor_idx"], lm["valid"], lm["X"],
                                       lm["med_dir"], lm["dir_ptr"], lm["dirs"])
    for j in range(50):
        slots = [k for k in range(n) for a in range(lm["anchor_ptr"][k], lm["anchor_ptr"][k + 1]) if lm["anchor_idx"][a] == j]
        p = lm["X"][j].copy()
        if lm["valid"][j]:
            for k in slots:
                if corrected[k]:
                    p = T_corr[k][:3, :3] @ p + T_corr[k][:3, 3]
        assert np.allclose(X[j], p, atol=1e-12)


def test_generator_is_seeded():
    a, b = pgo.pose_graph(n_kf=50, seed=3), pgo.pose_graph(n_kf=50, seed=3)
    for k in a:
        assert np.array_equal(a[k], b[k])
    m = pgo.pose_graph(n_kf=1500, n_loops=3, seed=3)
    assert m["lc_idx"].shape == (3, 3) and m["lc_idx"][:, 1].max() == 1500 - 1 - 3


# ---- the inputs beyond the planar circle (tests/pgo_cases.py): which branches they reach --------------------------------------
BRANCH_FUNCS = ("quat_from_R", "se3quat_exp", "se3quat_log", "from_vector_mqt", "expmap_se3", "logmap_se3")


def _count_branches(monkeypatch, m, max_iters=100):
    """Runs the restatement (optimize + write_back) on m with its helpers wrapped -> Counter of the branch each call took.
    Only calls with a non-identity argument count towards a small-angle or tr > 0 branch: on the identity both branches of
    every helper return the same thing, so such a call tests nothing."""
    import collections
    cnt = collections.Counter()
    orig = {k: getattr(R, k) for k in BRANCH_FUNCS}
    eye = np.eye(3)

    def quat_from_R(Rm):
        q = orig["quat_from_R"](Rm)
        if Rm[0, 0] + Rm[1, 1] + Rm[2, 2] > 0.0:
            cnt["quat_tr_pos"] += not np.array_equal(Rm, eye)
        else:
            cnt["quat_pivot%d" % int(np.argmax(np.abs(q[1:])))] += 1          # the pivot component is the largest of x, y, z
        cnt["quat_w_neg"] += bool(q[0] < 0.0)
        return q

    def se3quat_exp(u):
        th = float(np.sqrt(np.dot(u[:3], u[:3])))
        cnt["exp_small" if th < R.G2O["exp_small_theta"] else "exp_full"] += th > 0.0
        return orig["se3quat_exp"](u)

    def se3quat_log(X):
        Rq = R.R_from_quat(R.unit_quat(X[0]))
        d = 0.5 * (Rq[0, 0] + Rq[1, 1] + Rq[2, 2] - 1.0)
        cnt["log_first_order" if d > R.G2O["log_d_threshold"] else "log_full"] += not np.array_equal(X[0], eye)
        return orig["se3quat_log"](X)

    def from_vector_mqt(v):
        cnt["mqt_outside_unit_ball"] += bool(1.0 - (v[3] * v[3] + v[4] * v[4] + v[5] * v[5]) < 0.0)
        return orig["from_vector_mqt"](v)

    def expmap(x):
        th = float(np.sqrt(x[3] * x[3] + x[4] * x[4] + x[5] * x[5]))
        cnt["expmap_small" if th < 0.000001 else "expmap_full"] += th > 0.0
        return orig["expmap_se3"](x)

    def logmap(T):
        th = np.arccos(min(1.0, max(-1.0, (T[0, 0] + T[1, 1] + T[2, 2] - 1.0) / 2.0)))
        cnt["logmap_full" if th > 0.000001 else "logmap_small"] += not np.array_equal(T[:3, :3], eye)
        return orig["logmap_se3"](T)

    with monkeypatch.context() as mp:
        for k, f in zip(BRANCH_FUNCS, (quat_from_R, se3quat_exp, se3quat_log, from_vector_mqt, expmap, logmap)):
            mp.setattr(R, k, f)
        P = R.Pgo(m["kf_valid"], m["full_graph"], m["lc_idx"])
        r = P.optimize(m["T_kf_w"], m["x_kf_w"], m["lc_pose"], max_iters=max_iters)
        R.write_back(P, r, m["T_kf_w"], m["x_kf_w"])
    return cnt, P, r


ALL_PIVOTS = ("quat_tr_pos", "quat_pivot0", "quat_pivot1", "quat_pivot2", "quat_w_neg")
# (input of pgo_cases.INPUTS, max_iters_pgo) -> the branches it exists for; each at least REACH_MIN times.  max_iters 0 and 1
# are the stage probes of the device tests (initial guess + write-back alone; one linearisation and its trials)
REACH_MIN = 3
REACH = {
    ("conj_about_x", 100): ("quat_pivot2",),
    ("conj_about_z", 100): ("quat_pivot0",),
    ("conj_generic", 100): ("quat_pivot0",),
    ("tumbling", 100): ALL_PIVOTS,
    ("tumbling", 0): ALL_PIVOTS,
    ("tumbling", 1): ALL_PIVOTS,
    ("tumbling_2loops", 100): ALL_PIVOTS,
    ("tumbling_rejections", 100): ("mqt_outside_unit_ball", "quat_pivot0", "quat_pivot1", "quat_pivot2"),
    ("near_5e-7", 100): ("logmap_small", "logmap_full", "expmap_small", "expmap_full", "exp_small"),
    ("near_5e-7", 0): ("logmap_small", "logmap_full", "exp_small"),
    ("near_5e-6", 100): ("exp_small", "exp_full"),
    ("near_5e-6", 0): ("exp_small", "exp_full"),
    ("near_3e-5", 100): ("exp_small", "exp_full"),
    ("near_3e-5", 0): ("exp_small", "exp_full"),
    ("near_3e-5", 1): ("exp_small", "exp_full"),
    ("near_2e-3", 100): ("log_first_order", "log_full"),
    ("near_2e-3", 0): ("log_first_order", "log_full"),
    ("near_2e-3", 1): ("log_first_order", "log_full"),
}


def _missed(cnt, wanted):
    return [b for b in wanted if cnt[b] < REACH_MIN]


@pytest.mark.parametrize("name,max_iters", list(REACH))
def test_inputs_reach_their_branches(monkeypatch, name, max_iters):
    """The condition that keeps the device tests of these inputs honest: an input that stops reaching its branch fails here."""
    import pgo_cases
    cnt, P, r = _count_branches(monkeypatch, pgo_cases.INPUTS[name](), max_iters)
    assert not _missed(cnt, REACH[(name, max_iters)]), dict(cnt)
    if name == "tumbling":                     # the two isolated keyframes are vertices without a column
        assert len(P.active) == len(P.g["verts"]) - 1 - 2
    if name == "near_5e-6":                    # four of them here, two on each side of SE3Quat::exp's threshold
        m = pgo_cases.INPUTS[name]()
        assert len(P.active) == len(P.g["verts"]) - 1 - 4
        th = np.linalg.norm(m["x_kf_w"][[12, 23, 29, 48], 3:], axis=1)
        assert (th < 1e-5).sum() == 2 and (th > 1e-5).sum() == 2
    if name == "near_3e-5":                    # the measured relative rotations lie on both sides of it
        m = pgo_cases.INPUTS[name]()
        th = np.array([np.linalg.norm(logmap_se3(inverse_se3(m["T_kf_w"][i]) @ m["T_kf_w"][j])[3:])
                       for i, j, kind, _ in P.g["edges"] if kind == 0])
        assert (th < 1e-5).sum() >= 3 and (th > 1e-5).sum() >= 3
    if name == "tumbling_rejections":          # a step outside the unit ball within the trials that the device test compares
        assert any(not t["accepted"] for t in r["trace"])


@pytest.mark.parametrize("wanted", sorted(set(REACH.values())))
def test_the_planar_circle_reaches_none_of_them(monkeypatch, wanted):
    """Each set of branches above is missed by the generator's own circle (the null_slots case of the device tests), at every
    iteration limit used: swapping a new input for the circle fails its reach test."""
    for max_iters in (0, 1, 100):
        cnt, _, _ = _count_branches(monkeypatch, pgo.pose_graph(n_kf=60, null_slots=(9, 20, 33, 58), seed=6), max_iters)
        assert _missed(cnt, wanted), (max_iters, dict(cnt))


def test_chi_does_not_depend_on_the_world_frame():
    """Conjugating a map by a world rotation conjugates every edge error by it: chi_initial and chi_final are those of the
    unrotated map.  The restatement alone differs by 4e-13 relative over the three frames."""
    import pgo_cases
    m0 = pgo.pose_graph(n_kf=60, seed=6)
    P = R.Pgo(m0["kf_valid"], m0["full_graph"], m0["lc_idx"])
    r0 = P.optimize(m0["T_kf_w"], m0["x_kf_w"], m0["lc_pose"])
    T0 = R.write_back(P, r0, m0["T_kf_w"], m0["x_kf_w"])[0]
    for name in pgo_cases.FRAMES:
        G = pgo_cases.frame(name)
        m = pgo_cases.conjugate(m0, G)
        assert np.array_equal(m["full_graph"], m0["full_graph"]) and np.array_equal(m["lc_idx"], m0["lc_idx"])
        r = P.optimize(m["T_kf_w"], m["x_kf_w"], m["lc_pose"])
        assert r["chi_initial"] == pytest.approx(r0["chi_initial"], rel=1e-10)
        assert r["chi_final"] == pytest.approx(r0["chi_final"], rel=1e-10)
        T = R.write_back(P, r, m["T_kf_w"], m["x_kf_w"])[0]
        back = np.stack([inverse_se3(G) @ Tk @ G for Tk in T])
        assert np.abs(back - T0).max() <= 1e-9


# ---- the small-angle branches against their full formulas in extended precision ---------------------------------------------
LD = np.longdouble


def _skew_ld(w):
    return np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]], LD)


def _rodrigues_ld(w):
    """-> (R, V) of the rotation vector w by the full formulas, in long double; 1 - cos as 2 sin^2(theta / 2), which does not
    cancel."""
    w = np.asarray(w, LD)
    th = np.sqrt(w @ w)
    Om = _skew_ld(w)
    I = np.eye(3, dtype=LD)
    omc = 2 * np.sin(th / 2) ** 2
    return (I + np.sin(th) / th * Om + omc / (th * th) * (Om @ Om),
            I + omc / (th * th) * Om + (th - np.sin(th)) / (th ** 3) * (Om @ Om))


AXIS = np.array([0.48, -0.6, 0.64])            # a unit vector


@pytest.mark.parametrize("theta", [9e-6, 2e-6, 3e-7])
def test_se3quat_exp_small_angle_truncation(theta):
    """Below 1e-5 SE3Quat::exp takes R = I + Omega + Omega^2 through the unit quaternion, and V = R.  Normalising removes the
    symmetric part's error (Omega^2 in place of Omega^2 / 2), so R is Rodrigues' up to third-order terms; V = R is I + Omega where
    I + Omega / 2 belongs, so the translation is off in first order by Omega upsilon / 2."""
    assert np.finfo(LD).eps < 1e-18
    w, ups = theta * AXIS, np.array([1.0, -2.0, 0.5])
    Rs, t = R.se3quat_exp(np.concatenate([w, ups]))
    Rf, Vf = _rodrigues_ld(w)
    assert np.abs(Rs - Rf).max() <= theta ** 3 + 4 * np.finfo(float).eps
    d = np.asarray(t, LD) - Vf @ ups
    half = 0.5 * (_skew_ld(w) @ ups)
    assert np.linalg.norm(half.astype(float)) > 0.3 * theta
    assert np.linalg.norm((d - half).astype(float)) <= theta ** 2 * np.linalg.norm(ups)
    # just above the threshold the full branch is taken: no first-order term.  In double, 1 - cos(theta) = theta^2 / 2 carries a
    # few ulps of 1, i.e. 2 eps / theta^2 relative, on a term of size theta |upsilon|
    w2 = 1.1e-5 * AXIS
    R2, t2 = R.se3quat_exp(np.concatenate([w2, ups]))
    Rf2, Vf2 = _rodrigues_ld(w2)
    assert np.abs(R2 - Rf2).max() <= 1e-15
    assert np.abs(np.asarray(t2, LD) - Vf2 @ ups).max() <= 4 * np.finfo(float).eps * np.linalg.norm(ups) / 1.1e-5


@pytest.mark.parametrize("theta", [4.4e-3, 1e-3, 1e-4])
def test_se3quat_log_first_order_truncation(theta):
    """Above d = 0.99999 SE3Quat::log takes omega = dR / 2 = sin(theta) axis: short by theta^2 / 6 relative.  V^-1 carries that
    omega, so the translation is off by |omega x t| theta^2 / 12 at most; its own 1/12 series term is exact to theta^4 / 720."""
    assert np.finfo(LD).eps < 1e-18
    Rf, _ = _rodrigues_ld(theta * AXIS)
    X = (Rf.astype(float), np.array([1.0, -2.0, 0.5]))
    u = R.se3quat_log(X)
    # the full branch in long double on the same matrix
    Rl = np.asarray(X[0], LD)
    d = (Rl[0, 0] + Rl[1, 1] + Rl[2, 2] - 1) / 2
    th = np.arccos(d)
    wf = th / (2 * np.sqrt(1 - d * d)) * np.array([Rl[2, 1] - Rl[1, 2], Rl[0, 2] - Rl[2, 0], Rl[1, 0] - Rl[0, 1]], LD)
    Om = _skew_ld(wf)
    Vi = np.eye(3, dtype=LD) - Om / 2 + (1 - th / (2 * np.tan(th / 2))) / (th * th) * (Om @ Om)
    assert float(th) == pytest.approx(theta, rel=1e-6)
    short = np.linalg.norm((wf - u[:3]).astype(float)) / theta
    assert short == pytest.approx(theta * theta / 6, rel=1e-2)
    assert np.linalg.norm((Vi @ X[1] - u[3:]).astype(float)) <= 1.01 * theta ** 3 / 12 * np.linalg.norm(X[1]) + 1e-15


@pytest.mark.parametrize("theta", [9e-7, 1e-7])
def test_stvo_maps_small_angle_truncation(theta):
    """expmap_se3 / logmap_se3 below 1e-6 drop the rotation altogether: R = I and t = x[:3] (w = 0 and x[:3] = t).  Against the
    full formulas the rotation is off by theta and the translation by |omega x t| / 2, both first order."""
    assert np.finfo(LD).eps < 1e-18
    w, t = theta * AXIS, np.array([1.0, -2.0, 0.5])
    Rf, Vf = _rodrigues_ld(w)
    T = expmap_se3(np.concatenate([t, w]))
    assert np.array_equal(T[:3, :3], np.eye(3)) and np.array_equal(T[:3, 3], t)
    assert np.linalg.norm((Rf - np.eye(3)).astype(float)) == pytest.approx(np.sqrt(2.0) * theta, rel=1e-6)
    assert np.linalg.norm((Vf @ t - t - 0.5 * (_skew_ld(w) @ t)).astype(float)) <= theta ** 2 * np.linalg.norm(t)
    Tf = np.eye(4)
    Tf[:3, :3], Tf[:3, 3] = Rf.astype(float), t
    x = logmap_se3(Tf)
    assert np.array_equal(x[3:], np.zeros(3)) and np.array_equal(x[:3], t)
    # just above the threshold both take the full branch
    w2 = 1.5e-6 * AXIS
    R2, V2 = _rodrigues_ld(w2)
    T2 = expmap_se3(np.concatenate([t, w2]))
    assert np.abs(T2[:3, :3] - R2).max() <= 1e-15
    assert np.abs(T2[:3, 3] - V2 @ t).max() <= 4 * np.finfo(float).eps * np.linalg.norm(t) / 1.5e-6    # 1 - cos in double, as above
    assert np.abs(logmap_se3(T2)[3:] - w2).max() <= 1e-3 * 1.5e-6       # acos near 1: theta to ~1e-16 / theta absolute


def test_new_keywords_leave_the_generator_as_it_was():
    """true_poses / cov_step / vector drift and noise: their defaults, and the scalar forms, give the same bits."""
    a = pgo.pose_graph(n_kf=50, seed=3)
    b = pgo.pose_graph(n_kf=50, seed=3, drift=np.full(6, 0.003), lc_noise=np.full(6, 0.0005), cov_step=40, true_poses=None)
    c = pgo.pose_graph(n_kf=50, seed=3, true_poses=lambda n, period, step: a["T_true"])
    for k in a:
        assert np.array_equal(a[k], b[k]) and np.array_equal(a[k], c[k])
