"""CPU side of the global bundle adjustment (K26-K39): tests/gba_ref.py against the reference's own first-pass loops and its
text, the restatement's Schur + L D L^T solve against a dense solve, the trajectory-shaped map generator, and the C++ shim."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from plslam_amd import gba, synth
from oracle import oracle as O

import gba_ref

OCAM = O.make_cam(**synth.EUROC)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_SRC = "/root/reference/src/mapHandler.cpp"


def _gba_text():
    if not os.path.exists(REF_SRC):
        pytest.skip("the reference source is not on this machine")
    src = open(REF_SRC).read()
    a = src.index("void MapHandler::levMarquardtOptimizationGBA")
    b = src.index("\n}\n", a)
    body = src[a:b]
    it = body.index("// LM iterations")
    return body[:it], body[it:]


def test_first_pass_equals_the_references_own_loops():
    m = gba.trajectory_map(6, 50, 16, obs_per_lm=3, loop=False, seed=5)
    P = gba_ref.Problem(OCAM, m)
    B = P.blocks(True, m["x_kf"], m["Xw"], m["Lw"])
    H, g = P.full_H(B)
    T_map = m["T_kf_w"]
    pt, ls = m["pt_obs"], m["ls_obs"]
    ref = O.ref_lba_accumulate("gba", OCAM, 1e-7, P.nkf, T_map, T_map[1:], m["Xw"], m["Lw"], pt[:, 1], pt[:, 3], pt[:, 4],
                               m["pt_uv"], ls[:, 1], ls[:, 3], ls[:, 4], m["ls_l"])
    if ref is None:
        pytest.skip("oracle/_ref not built with the LBA harness (needs the reference at build time)")
    Hr, gr, er = ref
    np.testing.assert_allclose(H, Hr, rtol=1e-11, atol=1e-11 * np.abs(Hr).max())
    np.testing.assert_allclose(g, gr, rtol=1e-11, atol=1e-11 * np.abs(gr).max())
    assert np.isclose(B["err"], er, rtol=1e-11)


def test_the_text_the_findings_rest_on():
    first, loop = _gba_text()
    # 1: the observation counts are declared and never incremented; err is divided by them in both passes
    for t in (first, loop):
        assert "err /= (Npt_obs+Nls_obs);" in t
    body = first + loop
    assert "int Npt = 0, Npt_obs = 0;" in body and "int Nls = 0, Nls_obs = 0;" in body
    assert not re.search(r"N(pt|ls)_obs\s*(\+\+|\+=|=[^=])", body.replace("int Npt = 0, Npt_obs = 0", "")
                         .replace("int Nls = 0, Nls_obs = 0", ""))
    assert "if( err > err_prev ){" in loop and "lambda *= lambda_k;" in loop
    # 2: Hmax is an int
    assert "int Hmax = 0.0;" in first and "lambda *= Hmax;" in first
    # 3: the epsilon stops
    assert "if( abs(err-err_prev) < numeric_limits<double>::epsilon() || err < numeric_limits<double>::epsilon() )" in loop
    assert "if( DX.norm() < numeric_limits<double>::epsilon() )" in loop
    # 4: the pose x line cross blocks per pass
    assert "H.coeffRef(idx+i,jdx+j) += Hij(i,j);\n                        H.coeffRef(jdx+j,idx+i) += Hij(i,j);" in first
    assert "H.coeffRef(idx+i,jdx+j) += Hij(i,j);\n                            H.coeffRef(jdx+j,idx+i) += Hij(j,i);" in loop
    assert "SimplicialLDLT< SparseMatrix<double> > solver1(H);" in first and "SimplicialLDLT< SparseMatrix<double> > solver1(H);" in loop
    # 5: the first pass reads the stored poses; the iteration pass's points read the estimate, its lines the stored pose and
    # both end points from one stride-3 block
    assert first.count("Matrix4d Tiw   = map_keyframes[kf_idx_map]->T_kf_w;") == 2
    assert "Tiw = expmap_se3( X.block( 6*kf_idx_loc,0,6,1 ) );" in loop
    assert "Vector3d Pwj = X.block(6*Nkf+3*Npt+3*lm_idx_loc,0,3,1);" in loop
    assert "Vector3d Qwj = X.block(6*Nkf+3*Npt+3*lm_idx_loc,0,3,1);" in loop
    assert "Matrix4d Tiw   = map_keyframes[kf_idx_map]->T_kf_w;" in loop
    assert "SlamConfig::homogTh()" in loop and "0.0000001" not in loop
    # 6: keyframe 0 is not optimised
    src = open(REF_SRC).read()
    g = src[src.index("void MapHandler::globalBundleAdjustment"):src.index("void MapHandler::levMarquardtOptimizationGBA")]
    assert "if( (*kf_it)->kf_idx != 0 )" in g and "obs_aux(4) = -1;" in g


@pytest.mark.parametrize("first", [True, False])
@pytest.mark.parametrize("shape", [(5, 40, 0), (5, 0, 12), (7, 60, 20)])
def test_schur_ldlt_equals_a_dense_solve_of_the_lower_triangle(first, shape):
    n_kf, npt, nls = shape
    m = gba.trajectory_map(n_kf, npt, nls, obs_per_lm=3, loop=False, seed=17 + n_kf)
    P = gba_ref.Problem(OCAM, m)
    x = m["x_kf"] + 0.001
    B = P.blocks(first, x, m["Xw"], m["Lw"])
    if not first:
        B = dict(B, Wls=B["Wls"])
    H, g = P.full_H(B)       # lower blocks mirrored: the symmetric matrix SimplicialLDLT factors
    lam = 1e-3
    Hd = H + lam * np.diag(np.diag(H))
    ref = np.linalg.solve(Hd, g)
    s = gba_ref.schur_solve(P, B, lam)
    got = np.concatenate([s["dp"], s["dx_pt"].reshape(-1), s["dx_ls"].reshape(-1)])
    cond = np.linalg.cond(Hd)
    np.testing.assert_allclose(got, ref, rtol=0, atol=cond * 1e-15 * np.abs(ref).max())
    assert s["n_singular"] == 0 and s["n_bad"] == 0


def test_ldlt_restatement_on_indefinite_input():
    rng = np.random.Generator(np.random.PCG64(3))
    for n in (6, 65, 130):
        A = rng.standard_normal((n, n))
        A = A + A.T
        b = rng.standard_normal(n)
        x, bad = gba_ref.ldlt_solve(np.tril(A) + np.triu(rng.standard_normal((n, n)), 1), b)   # the upper triangle is ignored
        np.testing.assert_allclose(A @ x, b, atol=1e-8 * np.linalg.cond(A))
        assert bad == 0


def test_generator_is_banded_with_the_loop_block_and_deterministic():
    m = gba.trajectory_map(120, 3000, 500, obs_per_lm=4, loop=True, seed=9)
    blocks = gba.covisible_blocks(m)
    nkf = len(m["kf_list"])
    band = {(k1, k2) for k1, k2 in blocks if k1 - k2 <= 3}
    far = blocks - band
    assert far and all(k1 - k2 >= nkf - 4 for k1, k2 in far)          # only the loop links the two ends
    assert len(blocks) < 5 * nkf                                      # banded, not dense (nkf (nkf + 1) / 2 = 7140)
    assert all((k, k) in blocks for k in range(nkf))
    m2 = gba.trajectory_map(120, 3000, 500, obs_per_lm=4, loop=True, seed=9)
    for k, v in m.items():
        assert np.array_equal(np.asarray(v), np.asarray(m2[k])), k
    m3 = gba.trajectory_map(120, 3000, 500, obs_per_lm=4, loop=False, seed=9)
    assert all(k1 - k2 <= 3 for k1, k2 in gba.covisible_blocks(m3))
    # keyframe 0's observations carry local index -1 and every landmark is seen in front of its keyframes
    assert (m["pt_obs"][:, 4] == m["pt_obs"][:, 3] - 1).all() and (m["pt_obs"][m["pt_obs"][:, 3] == 0, 4] == -1).all()


def test_restatement_loop_follows_the_reference_schedule():
    m = gba.trajectory_map(8, 200, 40, obs_per_lm=3, loop=False, seed=23)
    r = gba_ref.gba_lm(gba_ref.Problem(OCAM, m), m["x_kf"], m["Xw"], m["Lw"], max_iters=15)
    assert r["iters"] == 15 and r["stop_reason"] == 0 and len(r["trace"]) == 15
    lam0 = 1e-5 * np.trunc(r["hmax"])
    # the first solve leaves lambda alone (:2366-2380); every later one is accepted and multiplies it by lambda_k afterwards
    lam = lam0
    for i, t in enumerate(r["trace"]):
        assert t["accepted"] and t["lam"] == lam and np.isinf(t["err"])
        if i > 0:
            lam *= 10.0


def test_cpp_shim_compiles_against_the_header(tmp_path):
    exe = str(tmp_path / "test_gba_shim")
    cxx = shutil.which("g++") or "g++"
    subprocess.run([cxx, "-O1", "-std=c++17", "-fsyntax-only", os.path.join(ROOT, "tests", "cpp", "test_gba_shim.cpp"),
                    "-I" + os.path.join(ROOT, "include")], check=True)
    assert not os.path.exists(exe)
