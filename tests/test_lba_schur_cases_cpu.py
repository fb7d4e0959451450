"""The cases of tests/lba_schur_cases.py and the two statements of the Schur step in tests/lba_schur_ref.py, without a GPU.  The
blocks are the oracle's rows (plo_lba_point_rows / plo_lba_line_rows) through its dense accumulation, the lists the Python mirror
of lba_lists.hpp.  Shown here: each case reaches what REACHES says; the float64 restatement in the device's operation order is
within bound_e of the long-double values for every case x lambda; the cap (bound_e <= 1e-5 max|S_ld|) holds for every lambda kept
and fails for every lambda dropped; the long-double Schur route equals the elimination of the whole damped system on the cases of
at most 600 unknowns; the measured constant of the inverse's error is the one written in lba_schur_ref.py."""
import functools

import numpy as np
import pytest

from oracle import oracle as O

import lba_schur_cases as CS
import lba_schur_ref as R
from lba_schur_ref import LD

CAM = O.make_cam(**CS.K)
NAMES = list(CS.CASES)
CAP = 1e-5


@functools.lru_cache(maxsize=None)
def cpu_blocks(name):
    """the blocks of a case as LbaPlan.blocks() lays them out, from the oracle's rows and its dense H, g; the rows beside them"""
    c = CS.case(name)
    nkf, npt, nls = c["nkf"], c["npt"], c["nls"]
    N = 6 * nkf + 3 * npt + 6 * nls
    H, g = np.zeros((N, N)), np.zeros(N)
    rows = {}
    for kind, n, DL, args, lm, kf in (("points", npt, 3, (c["X"], c["pt_obs_uv"], c["pt_lm"], c["pt_slot"]), c["pt_lm"], c["pt_kf_loc"]),
                                      ("lines", nls, 6, (c["L"], c["ls_l_obs"], c["ls_lm"], c["ls_slot"]), c["ls_lm"], c["ls_kf_loc"])):
        if lm.size == 0:
            rows[kind] = (np.zeros((0, 6)), np.zeros((0, DL)), np.zeros(0), np.zeros(0))
            continue
        rows[kind] = (O.lba_point_rows if kind == "points" else O.lba_line_rows)(CAM, CS.HOMOG_TH, c["T"], *args)
        H, g, _ = O.lba_accumulate(kind, nkf, npt, nls, lm, kf, *rows[kind], H=H, g=g)
    out = dict(g=g, H_pose=np.stack([H[6 * k:6 * k + 6, 6 * k:6 * k + 6] for k in range(nkf)]) if nkf else np.zeros((0, 6, 6)))
    for key, base, n, DL in (("H_pt", 6 * nkf, npt, 3), ("H_ls", 6 * nkf + 3 * npt, nls, 6)):
        out[key] = np.stack([H[base + DL * j:base + DL * j + DL, base + DL * j:base + DL * j + DL] for j in range(n)]) if n else np.zeros((0, DL, DL))
    for key, kind, kf in (("W_pt", "points", c["pt_kf_loc"]), ("W_ls", "lines", c["ls_kf_loc"])):
        Jp, Jl, r, w = rows[kind]
        W = Jl[:, :, None] * Jp[:, None, :] * w[:, None, None]                   # plo accumulate: Haux = Jl[a] * Jp[b] * ww
        W[kf < 0] = 0.0
        out[key] = W
    out["rows"] = rows
    assert all(np.isfinite(out[k]).all() for k in ("g", "H_pose", "H_pt", "H_ls", "W_pt", "W_ls")), name
    return out


@functools.lru_cache(maxsize=None)
def lists_of(name):
    return R.build_lists(CS.case(name))


def full_table(name):
    return ((0.0,) if name in CS.FULL_RANK else ()) + CS.LAMBDAS


@functools.lru_cache(maxsize=None)
def solved(name, lam):
    """(the restatement, the truth) of one case x lambda"""
    B, c = cpu_blocks(name), CS.case(name)
    Rr = R.restate(B, lists_of(name), lam)
    return Rr, R.truth(B, c, lam, Rr["sing_pt"], Rr["sing_ls"])


def _ranks(H):
    return [int(np.linalg.matrix_rank(h, tol=1e-9 * np.abs(h).max())) if np.abs(h).max() > 0 else 0 for h in H]


def _reached(name):
    """the tags of REACHES that hold for the case, from its columns, lists and blocks"""
    c, B, Ls = CS.case(name), cpu_blocks(name), lists_of(name)
    nkf, npt, nls = c["nkf"], c["npt"], c["nls"]
    tags = set()
    rp, rl = _ranks(B["H_pt"]), _ranks(B["H_ls"])
    for r in (1, 2):
        if npt and set(rp) == {r}:
            tags.add(f"pt_rank_{r}")
        if nls and set(rl) == {r}:
            tags.add(f"ls_rank_{r}")
    if set(rp) <= {3} and set(rl) <= {6}:
        tags.add("every_block_of_full_rank")
    # landmarks the fixed keyframe alone sees: no pair, no cross block -- but a block and a gradient of their own
    alone = [j for j in range(npt) if (c["pt_kf_loc"][c["pt_lm"] == j] < 0).all()] if npt else []
    if npt and len(alone) * 3 == npt and not set(alone) & set(Ls["pairs"][Ls["pairs"][:, 3] == 0, 2].tolist()) \
            and all(np.abs(B["H_pt"][j]).max() > 0 and np.abs(B["g"][6 * nkf + 3 * j:6 * nkf + 3 * j + 3]).max() > 0 for j in alone) \
            and all((B["W_pt"][c["pt_lm"] == j] == 0).all() for j in alone):
        tags.add("a_third_by_the_fixed_keyframe_only")
    if all(np.array_equal(T.reshape(4, 4)[:3, :3], np.eye(3)) for T in c["T"]):
        tags.add("rotations_are_identity")
    zero_diag = [(B["H_pt"][j, 2, 2] == 0.0 and np.abs(B["H_pt"][j]).max() > 0) for j in range(npt)]
    zero_diag += [(B["H_ls"][j, 2, 2] == 0.0 and B["H_ls"][j, 5, 5] == 0.0 and np.abs(B["H_ls"][j]).max() > 0) for j in range(nls)]
    if sum(zero_diag) == 4:
        tags.add("zero_on_the_diagonal_of_a_nonzero_block_x4")
        # the zero is exact: every row of these landmarks has a z column of zeros (either sign), so each term of the sum is one
        Jl_p, Jl_l = B["rows"]["points"][1], B["rows"]["lines"][1]
        on = [j for j in range(npt) if zero_diag[j]], [j for j in range(nls) if zero_diag[npt + j]]
        assert all((Jl_p[c["pt_lm"] == j][:, 2] == 0.0).all() and np.abs(Jl_p[c["pt_lm"] == j][:, :2]).min() > 0 for j in on[0])
        assert all((Jl_l[c["ls_lm"] == j][:, [2, 5]] == 0.0).all() for j in on[1])
        assert on == ([0, 1, 2], [0])
        if all(solved(name, lam)[0]["n_singular"] == 4 and np.flatnonzero(solved(name, lam)[0]["sing_pt"]).tolist() == [0, 1, 2]
               and np.flatnonzero(solved(name, lam)[0]["sing_ls"]).tolist() == [0] for lam in CS.LAMBDAS):
            tags.add("four_singular_at_every_lambda")
    pr = Ls["pairs"]
    nblk = nkf * (nkf + 1) // 2
    diag = {k * nkf - k * (k - 1) // 2 for k in range(nkf)}
    for blk in diag:
        q = pr[Ls["blk_ptr"][blk]:Ls["blk_ptr"][blk + 1]]
        q = {tuple(x) for x in q[q[:, 3] != 2].tolist()}
        if any((o2, o1, j, ln) in q for (o1, o2, j, ln) in q if o1 != o2):
            tags.add("both_orders_in_a_diagonal_block")
    cnt = np.diff(Ls["blk_ptr"])
    if nkf >= 2 and cnt[1] == 0 and (cnt[[b for b in range(nblk) if b != 1]] > 0).all():
        tags.add("a_block_without_pairs")                                         # block 1 = (0, 1)
    if nkf == 6:
        off = [1, 2, 7]                                                             # (0,1), (0,2), (1,2) of six keyframes
        kinds = [pr[Ls["blk_ptr"][b]:Ls["blk_ptr"][b + 1], 3] for b in off]
        if [int((k == 0).sum()) for k in kinds] == [63, 64, 65] and all((k == 1).sum() == 3 for k in kinds):
            tags.add("point_pairs_63_64_65")
        if [int((k == 2).sum()) for k in kinds] == [1, 0, 63]:
            tags.add("null_pairs_1_0_63")
        if np.diff(Ls["kf_ptr"])[3:].tolist() == [63, 64, 65]:
            tags.add("keyframes_of_63_64_65")
    nch = (cnt + R.SCH_CHUNK - 1) // R.SCH_CHUNK
    if nkf == 2 and nch[1] == 33 and (pr[Ls["blk_ptr"][1]:Ls["blk_ptr"][2], 3] == 0).all():
        tags.add("block_of_33_chunks")
    if ((np.diff(Ls["kf_ptr"]) + R.POSE_CHUNK - 1) // R.POSE_CHUNK).tolist() == [33, 33] and Ls["max_chunks"] == 33:
        tags.add("keyframes_of_33_chunks")
    tags.add(f"workgroups_{npt}_{nls}")
    if npt:
        z = np.concatenate([c["X"][:, 2], c["L"][:, 2]])
        if z.min() <= 0.55 and z.max() >= 480.0:
            tags.add("depths_over_three_decades")
        # a landmark block is J^T J w with J ~ f / depth: depths over a factor 1000 spread the blocks over 1000^2, the cross blocks
        # (one factor J of the landmark, one of the pose) over 1000
        m, w = np.abs(B["H_pt"]).max(axis=(1, 2)), np.abs(B["W_pt"][c["pt_kf_loc"] >= 0]).max(axis=(1, 2))
        if m.max() / m.min() >= 1e6 and w.max() / w.min() >= 1e3:
            tags.add("blocks_over_six_decades")
    if 0.0 in CS.lambdas(name) and 1e-8 in CS.lambdas(name):                      # (test_the_cap: what DROPPED leaves is under the cap)
        tags.add("lambda_zero_under_the_cap")
    if nls == 0 and npt:
        tags.add("no_lines")
    if npt == 0 and nls:
        tags.add("no_points")
    if nkf == 1 and nblk == 1:
        tags.add("one_block")
    return tags


@pytest.mark.parametrize("name", NAMES)
def test_cases_reach_what_they_are_for(name):
    assert set(CS.REACHES) == set(CS.CASES)
    got = _reached(name)
    missing = [t for t in CS.REACHES[name] if t not in got]
    assert not missing, (missing, sorted(got))


def test_lambda_zero_is_kept_for_exactly_the_full_rank_cases():
    full = [n for n in NAMES if set(_ranks(cpu_blocks(n)["H_pt"])) <= {3} and set(_ranks(cpu_blocks(n)["H_ls"])) <= {6}]
    assert tuple(full) == CS.FULL_RANK
    assert all((0.0 in full_table(n)) == (n in CS.FULL_RANK) and set(CS.lambdas(n)) <= set(full_table(n)) for n in NAMES)


def test_the_case_sizes_the_issue_names():
    dims = {n: (CS.case(n)["n_pose_slots"], CS.case(n)["npt"], CS.case(n)["nls"]) for n in NAMES}
    assert dims["two_views"] == (4, 90, 40) and dims["chunks_33"] == (3, 2049, 10)
    assert {dims[f"backsub_{p}_{l}"][1:] for p in (63, 64, 65) for l in (31, 32, 33)} == {(p, l) for p in (63, 64, 65) for l in (31, 32, 33)}
    assert dims["points_only"] == (6, 300, 0) and dims["lines_only"] == (6, 0, 90) and dims["one_optimised_keyframe"] == (2, 200, 40)
    assert 5900 <= lists_of("chunks_33")["pairs"].shape[0] <= 6600


def test_the_mirror_of_the_lists_on_a_case_worked_by_hand():
    """lba_plan_dev_cases.py's twice_by_one_keyframe: landmark 1 seen twice by keyframe 2 (observations 0 and 2) and once by 1"""
    c = dict(nkf=3, npt=2, nls=1, pt_lm=[1, 0, 1, 1, 0], pt_kf_loc=[2, 0, 2, 1, -1], ls_lm=[0, 0, 0], ls_kf_loc=[1, 1, 0])
    Ls = R.build_lists(c)
    assert Ls["pt_ptr"].tolist() == [0, 2, 5] and Ls["pt_ids"].tolist() == [1, 4, 0, 2, 3]
    assert Ls["kf_ptr"].tolist() == [0, 2, 5, 7] and Ls["kf_ids"].tolist() == [1, 5 + 2, 3, 5 + 0, 5 + 1, 0, 2]
    pr = [tuple(x) for x in Ls["pairs"].tolist()]
    # blocks (0,0) (0,1) (0,2) (1,1) (1,2) (2,2)
    assert Ls["blk_ptr"].tolist() == [0, 65, 67, 67, 135, 137, 141]
    assert pr[0] == (1, 1, 0, 0) and pr[1:64] == [(0, 0, 0, 2)] * 63 and pr[64] == (2, 2, 0, 1)
    assert pr[65:67] == [(2, 0, 0, 1), (2, 1, 0, 1)]
    assert pr[67] == (3, 3, 1, 0) and pr[68:131] == [(0, 0, 0, 2)] * 63
    assert pr[131:135] == [(0, 0, 0, 1), (0, 1, 0, 1), (1, 0, 0, 1), (1, 1, 0, 1)]
    assert pr[135:137] == [(3, 0, 1, 0), (3, 2, 1, 0)]
    assert pr[137:141] == [(0, 0, 1, 0), (0, 2, 1, 0), (2, 0, 1, 0), (2, 2, 1, 0)]
    assert Ls["schur_chunks"] == 2 and Ls["max_chunks"] == 1


def _dp(name, lam):
    """the pose step the GPU test uses: a float64 solve of the restated system (an input like any other)"""
    Rr = solved(name, lam)[0]
    return np.linalg.solve(Rr["S"], Rr["b"])


@pytest.mark.parametrize("name", NAMES)
def test_the_restatement_is_within_the_bound_of_the_long_double_values(name):
    c, B, Ls = CS.case(name), cpu_blocks(name), lists_of(name)
    assert CS.lambdas(name), name
    for lam in CS.lambdas(name):
        Rr, Tr = solved(name, lam)
        bS, bb = R.bounds_system(Tr, Ls, c["nkf"], c["nls"] > 0)
        eS = np.abs(np.asarray(Rr["S"], LD) - Tr["S"]).astype(np.float64)
        eb = np.abs(np.asarray(Rr["b"], LD) - Tr["b"]).astype(np.float64)
        assert (eS <= bS).all(), (name, lam, float((eS / np.maximum(bS, 1e-300)).max()))
        assert (eb <= bb).all(), (name, lam, float((eb / np.maximum(bb, 1e-300)).max()))
        nk = c["nkf"]                                                               # an off-diagonal block is its mirror's transpose, to the word
        assert all(np.array_equal(Rr["S"][6 * i:6 * i + 6, 6 * j:6 * j + 6], Rr["S"][6 * j:6 * j + 6, 6 * i:6 * i + 6].T)
                   for i in range(nk) for j in range(i + 1, nk))
        assert Rr["diag_max"] == max(np.abs(np.diagonal(B[k], axis1=1, axis2=2)).max() for k in ("H_pose", "H_pt", "H_ls") if B[k].size)
        n_wg = -(-c["npt"] // CS.BACK_PT) + -(-c["nls"] // CS.BACK_LS)
        for dp in (np.zeros(6 * c["nkf"]), _dp(name, lam)):
            dxp, dxl, ss = R.restate_backsub(B, Ls, Rr, dp)
            tp, tl, ss_ld, ap, al = R.truth_steps(B, c, Tr, dp)
            bp, bl = R.bounds_steps(Tr, Ls, ap, al)
            for got, want, bd in ((dxp, tp, bp), (dxl, tl, bl)):
                e = np.abs(np.asarray(got, LD) - want).astype(np.float64)
                assert (e <= bd).all(), (name, lam, float((e / np.maximum(bd, 1e-300)).max()))
            assert abs(float(LD(ss) - ss_ld)) <= R.bound_sumsq(tp, tl, bp, bl, n_wg), (name, lam)
            if not dp.any():                                                        # backsub(0) returns t itself, to the word
                assert np.array_equal(dxp.view(np.uint64), Rr["tp"].view(np.uint64))
                assert np.array_equal(dxl.view(np.uint64), Rr["tl"].view(np.uint64))
        # a dropped landmark: Vinv = t = step = 0.0 exactly
        for V, t, d, s in ((Rr["Vp"], Rr["tp"], dxp, Rr["sing_pt"]), (Rr["Vl"], Rr["tl"], dxl, Rr["sing_ls"])):
            assert not V[s].any() and not t[s].any() and not d[s].any() and not np.signbit(d[s]).any()


@pytest.mark.parametrize("name", NAMES)
def test_the_cap(name):
    """bound_e <= 1e-5 max|S_ld| for every entry, for every lambda kept; and DROPPED holds exactly the lambdas that miss it"""
    c, Ls = CS.case(name), lists_of(name)
    miss = []
    for lam in full_table(name):
        Rr, Tr = solved(name, lam)
        bS, _ = R.bounds_system(Tr, Ls, c["nkf"], c["nls"] > 0)
        if not bS.max() <= CAP * float(np.abs(Tr["S"]).max()):
            miss.append(lam)
    assert tuple(miss) == tuple(CS.DROPPED.get(name, ())), (name, miss)
    assert set(CS.DROPPED) <= set(CS.CASES)


def test_on_the_axis_is_the_map_without_its_four_landmarks():
    """S and b of on_the_axis are, to the word, those of the same map with points 0, 1, 2 and line 0 never observed"""
    name = "on_the_axis"
    c, B = CS.case(name), cpu_blocks(name)
    keep_p, keep_l = c["pt_lm"] > 2, c["ls_lm"] > 0
    c2 = dict(c, pt_lm=c["pt_lm"][keep_p], pt_kf_loc=c["pt_kf_loc"][keep_p], ls_lm=c["ls_lm"][keep_l], ls_kf_loc=c["ls_kf_loc"][keep_l])
    B2 = dict(B, W_pt=B["W_pt"][keep_p], W_ls=B["W_ls"][keep_l])
    for lam in CS.lambdas(name):
        a, b = solved(name, lam)[0], R.restate(B2, R.build_lists(c2), lam)
        # (the pose blocks still hold the four landmarks' observations: H_pose and g_pose are inputs here, the same for both)
        assert a["n_singular"] == 4 and b["n_singular"] == 4
        assert np.array_equal(a["S"].view(np.uint64), b["S"].view(np.uint64)) and np.array_equal(a["b"].view(np.uint64), b["b"].view(np.uint64))


def test_strangers_have_a_block_of_positive_zeros():
    for lam in CS.lambdas("strangers"):
        S = solved("strangers", lam)[0]["S"]
        for blk in (S[0:6, 6:12], S[6:12, 0:6]):
            assert not blk.any() and not np.signbit(blk).any()
        assert S[0:6, 12:18].all()


SMALL = [n for n in NAMES if 6 * CS.case(n)["nkf"] + 3 * CS.case(n)["npt"] + 6 * CS.case(n)["nls"] <= 600]


@pytest.mark.parametrize("name", SMALL)
def test_the_long_double_schur_route_equals_the_whole_system(name):
    """The damped system H + lambda diag(H) of at most 600 unknowns, the dropped landmarks' rows and columns deleted, through
    solve_long_double whole -- against S_ld dp = b_ld and the back-substitution, to 1e-15 of the largest step.

    Plain long double does not reach 1e-15 here: either route errs by about cond * 1e-19, and the two differed by up to 8.7e-14
    of the largest step (lines_only, lambda = 1e-3; 4.9e-14 on backsub_63_32, 1.1e-14 on twice_by_one_keyframe).  So each route is used as
    what it is, a solver, on its own residual: two rounds of x += solve(g - H x) with the residual formed in rational
    arithmetic.  A route that solved another system than H x = g would not close on the other one's answer in two rounds."""
    c, B = CS.case(name), cpu_blocks(name)
    for lam in CS.lambdas(name):
        Rr, Tr = solved(name, lam)
        Hk, g, whole, keep = R.whole_system(B, c, lam, Rr["sing_pt"], Rr["sing_ls"])
        schur = lambda rhs: R.schur_solve(B, c, Tr, rhs)                          # noqa: E731
        out = []
        for solve in (schur, whole):
            x = solve(g)
            first = x.copy()
            for _ in range(2):
                r = np.zeros(g.size)
                r[keep] = R.exact_residual(Hk, g[keep], x[keep])
                x = x + solve(r)
            out.append((first, x))
        (a0, a), (b0, b) = out
        top = float(np.abs(b).max())
        print(f"{name} lambda {lam:g}: routes apart by {float(np.abs(a0 - b0).max()) / top:.2e} plain, {float(np.abs(a - b).max()) / top:.2e} refined")
        assert not a[~keep].any() and not b[~keep].any()
        assert float(np.abs(a - b).max()) <= 1e-15 * top, (name, lam, float(np.abs(a - b).max()) / top)
        # and the plain values, the ones the bounds are measured against, are the refined ones to far below any bound
        assert float(np.abs(a0 - a).max()) <= 1e-11 * top and float(np.abs(b0 - b).max()) <= 1e-11 * top


def test_small_cases_are_the_ones_meant():
    assert {"two_views", "one_view", "on_the_axis", "twice_by_one_keyframe", "strangers", "backsub_65_33"} <= set(SMALL)


def test_the_measurement_of_c_inv():
    """C_INV_MEASURED is the largest normalised error of the restated Gauss-Jordan inverse over every landmark x case x lambda of
    the table (the lambdas the cap drops too), and C_INV four times it"""
    assert np.finfo(LD).eps < 1e-18
    worst = 0.0
    for name in NAMES:
        for lam in full_table(name):
            Rr, Tr = solved(name, lam)
            worst = max(worst, R.c_inv_ratio(Rr["Vp"], Tr["Vp"], Tr["kap_p"], Rr["sing_pt"]),
                        R.c_inv_ratio(Rr["Vl"], Tr["Vl"], Tr["kap_l"], Rr["sing_ls"]))
    print(f"measured C_inv = {worst:.6g}")
    assert R.C_INV == 4 * R.C_INV_MEASURED
    assert 0.98 * R.C_INV_MEASURED <= worst <= 1.02 * R.C_INV_MEASURED, worst


# ---- what the exact comparison sees and 1e-9 max|S| does not ------------------------------------------------------------------------
def _reversed_block(Ls, blk):
    p = Ls["pairs"].copy()
    a, b = Ls["blk_ptr"][blk], Ls["blk_ptr"][blk + 1]
    p[a:b] = p[a:b][::-1]
    return dict(Ls, pairs=p)


def _smallest_pair_dropped(name, lam):
    """the pair of block (0, 1) whose contribution is the smallest becomes a null pair"""
    B, Ls = cpu_blocks(name), lists_of(name)
    Rr = solved(name, lam)[0]
    a, b = Ls["blk_ptr"][1], Ls["blk_ptr"][2]
    q = Ls["pairs"][a:b]
    size = np.full(b - a, np.inf)
    pt = np.flatnonzero(q[:, 3] == 0)
    size[pt] = np.abs(R.restate_pair_blocks(B["W_pt"][q[pt, 0]], B["W_pt"][q[pt, 1]], Rr["Vp"][q[pt, 2]])).max(axis=(1, 2))
    p = Ls["pairs"].copy()
    p[a + int(np.argmin(size))] = (0, 0, 0, 2)
    return dict(Ls, pairs=p)


MUTANTS = {
    "chunks of 32 pairs": ("chunks_33", True, lambda n, lam: R.restate(cpu_blocks(n), lists_of(n), lam, sch_chunk=32)),
    "a block's pairs in reverse order": ("chunks_33", True, lambda n, lam: R.restate(cpu_blocks(n), _reversed_block(lists_of(n), 1), lam)),
    "the smallest pair of a block dropped": ("depths", False, lambda n, lam: R.restate(cpu_blocks(n), _smallest_pair_dropped(n, lam), lam)),
}


@pytest.mark.parametrize("what", list(MUTANTS))
def test_a_wrong_order_or_a_dropped_pair_changes_words(what):
    """test_gpu_lba.py compares S at atol = 1e-9 max|S|: the wrong orders pass it (a dropped pair does not: W^T Vinv W does not
    shrink with the landmark's depth), and none of the three gives the restatement's words"""
    name, small, mutant = MUTANTS[what]
    lam = CS.lambdas(name)[0]
    S, M = solved(name, lam)[0]["S"], mutant(name, lam)["S"]
    diff = np.abs(M - S).max()
    assert not np.array_equal(M.view(np.uint64), S.view(np.uint64)), what
    assert diff > 0 and (not small or diff <= 1e-9 * np.abs(S).max()), (what, diff / np.abs(S).max())
