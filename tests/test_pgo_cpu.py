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
