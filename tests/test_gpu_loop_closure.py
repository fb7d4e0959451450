"""K25 (plslam_amd/csrc/loop_closure.hip) on the device against tests/lc_ref.py, the numpy restatement of
MapHandler::isLoopClosure + computeRelativePoseRobustGN (src/mapHandler.cpp:3192-3300, :3566-3957)."""
import math

import numpy as np
import pytest

import plslam_amd
from plslam_amd import loop_closure as LC, synth
from oracle import oracle as O

import lc_cases as CASES
import lc_ref

pytestmark = pytest.mark.gpu

OCAM = O.make_cam(**synth.EUROC)
MODES = {"pl": dict(has_points=1, has_lines=1), "p": dict(has_points=1, has_lines=0), "l": dict(has_points=0, has_lines=1)}
REL = 1e-9


@pytest.fixture(scope="module")
def ctx():
    c = plslam_amd.Context(0)
    yield c
    c.close()


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.max(np.abs(a - b)) / max(1e-300, float(np.max(np.abs(b))))) if a.size else 0.0


def _margins(ref, prm):
    """the fixture's own margins: 0.05 px around sqrt(7.815) at the outlier pass, 1 % around every decision threshold"""
    rp, rl = ref["res_at_outlier_pass"]
    for r in (rp, rl):
        r = r[np.isfinite(r)]
        assert r.size == 0 or np.min(np.abs(r - lc_ref.CHI)) >= 0.05, "a residual sits on the outlier threshold"
    for v, th in ((ref["e"], prm["lc_res"]), (ref["cov_eig"], prm["lc_unc"]), (ref["t"], prm["lc_trs"]),
                  (ref["r"], prm["lc_rot"])):
        if np.isfinite(v):
            assert abs(v - th) >= 0.01 * abs(th), f"{v} is within 1 % of its threshold {th}"


def _check(dev, pc, pi, lc, li, ref, prm, margins=True, rank_deficient=False, nan_pattern=False):
    """nan_pattern: the input holds a NaN -- on top of everything else, every entry of T_inc is NaN where the restatement's is
    and within REL of it where it is finite"""
    d = dev
    for k in ("common_pt", "common_ls", "gn_ran", "is_lc"):
        assert d[k] == ref[k], (k, d[k], ref[k])
    assert np.array_equal(pc, ref["pt_corr"]) and np.array_equal(lc, ref["ls_corr"])
    for k in ("inl_ratio_pt", "inl_ratio_ls"):
        assert (math.isnan(d[k]) and math.isnan(ref[k])) or d[k] == ref[k], (k, d[k], ref[k])
    if not ref["gn_ran"]:
        assert pi.all() and li.all()
        return
    if margins:
        _margins(ref, prm)
    assert np.array_equal(pi, ref["pt_inlier"]) and np.array_equal(li, ref["ls_inlier"])
    for k in ("ok_res", "ok_unc", "ok_inl", "ok_trs", "ok_rot", "n_pt_inliers", "n_ls_inliers"):
        assert d[k] == ref[k], (k, d[k], ref[k])
    if ref["stops"][0] != "err_change" and ref["stops"][1] != "err_change":
        assert (d["iters_1"], d["iters_2"]) == (ref["iters_1"], ref["iters_2"])
    for k in ("e",) if rank_deficient else ("e", "t", "r", "cov_eig"):
        if math.isnan(ref[k]):
            assert math.isnan(d[k]), k
        else:
            assert abs(d[k] - ref[k]) <= REL * abs(ref[k]) + 1e-300, (k, d[k], ref[k])
    if rank_deficient:
        return
    if np.isfinite(ref["T_inc"]).all():
        assert _rel(d["T_inc"], ref["T_inc"]) <= REL
    if nan_pattern:
        got, exp = np.asarray(d["T_inc"], np.float64).reshape(4, 4), ref["T_inc"]
        assert np.array_equal(np.isnan(got), np.isnan(exp)), (got, exp)
        fin = ~np.isnan(exp)
        assert np.all(np.abs(got[fin] - exp[fin]) <= REL * np.abs(exp[fin]))
    assert _rel(d["pose_inc"], ref["pose_inc"]) <= REL or not ref["is_lc"]
    if ref["is_lc"]:
        got0, got1 = (pc[pi], lc[li])
        exp0, exp1 = lc_ref.reference_outputs(ref)
        assert np.array_equal(got0, exp0) and np.array_equal(got1, exp1)


def _run(ctx, prm_over, kf0, kf1, margins=True, rank_deficient=False):
    p = LC.params(**prm_over)
    prm = LC.params_dict(p)
    ref = lc_ref.is_loop_closure(prm, OCAM, kf0, kf1)
    dev = ctx.loop_closure_verify(p, kf0, kf1)
    _check(*dev, ref, prm, margins=margins, rank_deficient=rank_deficient)
    return dev, ref


@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("size", [(1500, 200), (800, 100), (4000, 600)])
def test_seeded_pairs_against_the_restatement(ctx, mode, size):
    kf0, kf1, truth = LC.keyframe_pair(11 + size[0], *size)
    dev, ref = _run(ctx, MODES[mode], kf0, kf1)
    assert ref["is_lc"] == 1 and dev[0]["is_lc"] == 1
    # the match tables themselves, from the rows
    m12p, _ = O.match(kf0["pdesc"], kf1["pdesc"], 0.75, True)
    if MODES[mode]["has_points"]:
        got = np.full(size[0], -1, np.int32)
        got[dev[1][:, 1]] = dev[1][:, 3]
        assert np.array_equal(got, m12p)


def test_kitti_iterations(ctx):
    kf0, kf1, _ = LC.keyframe_pair(5, 1500, 200)
    _run(ctx, LC.KITTI_ITERS, kf0, kf1)


def test_the_size_limit(ctx):
    n = plslam_amd.capi.LC_MAX_FEATURES
    kf0, kf1, _ = LC.keyframe_pair(21, n, 64)
    _run(ctx, {}, kf0, kf1)
    big0, big1, _ = LC.keyframe_pair(22, n + 1, 8)
    with pytest.raises(plslam_amd.PlslamError) as ei:
        ctx.loop_closure_verify(LC.params(), big0, big1)
    assert ei.value.code == plslam_amd.capi.ERANGE


def test_each_branch(ctx):
    kf0, kf1, _ = LC.keyframe_pair(31, 1500, 200)
    base = lc_ref.is_loop_closure(LC.params_dict(LC.params()), OCAM, kf0, kf1)
    assert base["is_lc"]
    # the ratio gate fails: no GN
    d, _ = _run(ctx, dict(lc_inlier_ratio=95.0), kf0, kf1)
    assert d[0]["gn_ran"] == 0 and d[0]["is_lc"] == 0
    # each decision test fails on its own
    for name, field, flag in (("lc_res", "e", "ok_res"), ("lc_unc", "cov_eig", "ok_unc"), ("lc_trs", "t", "ok_trs"),
                              ("lc_rot", "r", "ok_rot")):
        d, ref = _run(ctx, {name: 0.5 * base[field]}, kf0, kf1)
        assert d[0][flag] == 0 and d[0]["is_lc"] == 0 and sum(d[0][f] for f in ("ok_res", "ok_unc", "ok_trs", "ok_rot")) == 3
    # ratio_inliers < lc_inl is still a loop closure (:3903)
    d, _ = _run(ctx, dict(lc_inl=0.995), kf0, kf1)
    assert d[0]["ok_inl"] == 0 and d[0]["is_lc"] == 1


def test_kf0_without_points_gives_a_nan_ratio(ctx):
    kf0, kf1, _ = LC.keyframe_pair(41, 0, 200)
    k1, _, _ = LC.keyframe_pair(42, 300, 10)
    kf1 = dict(kf1, pdesc=k1["pdesc"], P=k1["P"], pl=k1["pl"], pt_idx=k1["pt_idx"])
    d, ref = _run(ctx, {}, kf0, kf1)
    assert math.isnan(d[0]["inl_ratio_pt"]) and d[0]["gn_ran"] == 0
    d, ref = _run(ctx, MODES["l"], kf0, kf1)
    assert d[0]["gn_ran"] == 1


def test_every_correspondence_rejected_gives_nan_e_and_a_zero_step(ctx):
    kf0, kf1, _ = LC.keyframe_pair(51, 400, 50, outlier_frac=1.0, outlier_px=(60.0, 90.0), keep_frac=1.0)
    d, ref = _run(ctx, dict(max_iters=0), kf0, kf1)
    assert ref["n_pt_inliers"] == 0 and ref["n_ls_inliers"] == 0
    assert math.isnan(d[0]["e"]) and d[0]["is_lc"] == 0 and d[0]["iters_2"] == 1 and ref["stops"][1] == "x_small"
    assert np.array_equal(d[0]["T_inc"], np.eye(4))


@pytest.mark.parametrize("n", [0, 1, 2])
def test_tiny_keyframes(ctx, n):
    kf0, kf1, _ = LC.keyframe_pair(61 + n, n, n, keep_frac=1.0, outlier_frac=0.0, flip_p=0.0)
    # with two correspondences per kind H has rank <= 4: the solve's step in H's null space is set by the rank cut, which
    # compares column norms of ~eps * max against a threshold of ~eps * max, and by last-ulp differences of the SE(3) maps --
    # so T_inc, t, r and the eigenvalue of H^-1 are rounding-decided (measured: t 0.1396 on the device, 0.1351 restated).
    # What the data decide is compared: every count, row, mask and flag, and e within 1e-9
    d, ref = _run(ctx, {}, kf0, kf1, margins=False, rank_deficient=True)
    assert n > 0 or d[0]["gn_ran"] == 0
    if ref["gn_ran"]:
        assert d[0]["ok_unc"] == 0


def test_one_iteration_equals_k17(ctx):
    kf0, kf1, _ = LC.keyframe_pair(71, 1500, 200)
    p = LC.params(max_iters=1, max_iters_ref=0)
    d, pc, pi, lc, li = ctx.loop_closure_verify(p, kf0, kf1)
    P, pl = kf0["P"][pc[:, 1]], kf1["pl"][pc[:, 3]]
    S, le = kf0["sPeP"][lc[:, 1]], kf1["le"][lc[:, 3]]
    cam = plslam_amd.make_cam(**synth.EUROC)
    H, g, e, n = ctx.pose_gn_accumulate(cam, 1e-7, np.eye(4), P, pl, np.ones(len(P), np.uint8), S, le, np.ones(len(S), np.uint8))
    assert np.array_equal(d["H"], H) and np.array_equal(d["g"], g)          # K17's lane assignment and tree: bit for bit
    assert d["e"] == e / (n[0] + n[1])


def test_dev_form_equals_host_form_and_repeats_are_bitwise(ctx):
    torch = pytest.importorskip("torch")
    kf0, kf1, _ = LC.keyframe_pair(81, 1500, 200)
    p = LC.params()
    host = ctx.loop_closure_verify(p, kf0, kf1)
    for _ in range(19):
        again = ctx.loop_closure_verify(p, kf0, kf1)
        for k, v in host[0].items():
            if k in ("clk_total", "clk_serial"):
                continue
            assert np.array_equal(np.asarray(again[0][k]), np.asarray(v), equal_nan=True), k
        for a, b in zip(host[1:], again[1:]):
            assert np.array_equal(a, b)
    dev = torch.device("cuda:0")
    keep = []

    def put(a):
        t = torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        keep.append(t)
        return t.data_ptr()

    recs = []
    for kf in (kf0, kf1):
        recs.append(dict(pdesc=put(kf["pdesc"]), P=put(kf["P"]), pl=put(kf["pl"]), pt_idx=put(kf["pt_idx"]),
                         ldesc=put(kf["ldesc"]), sPeP=put(kf["sPeP"]), le=put(kf["le"]), ls_idx=put(kf["ls_idx"]),
                         n_pt=len(kf["P"]), n_ls=len(kf["sPeP"])))
    res = torch.zeros(C_sizeof(), dtype=torch.uint8, device=dev)
    pc = torch.zeros((len(kf0["P"]), 4), dtype=torch.int32, device=dev)
    pi = torch.zeros(len(kf0["P"]), dtype=torch.uint8, device=dev)
    lcr = torch.zeros((len(kf0["sPeP"]), 4), dtype=torch.int32, device=dev)
    li = torch.zeros(len(kf0["sPeP"]), dtype=torch.uint8, device=dev)
    s = torch.cuda.Stream(dev)
    ctx.loop_closure_verify_dev(p, recs[0], recs[1], res.data_ptr(), pc.data_ptr(), pi.data_ptr(), lcr.data_ptr(),
                                li.data_ptr(), stream=s.cuda_stream)
    s.synchronize()
    r = plslam_amd.LcResult.from_buffer_copy(res.cpu().numpy().tobytes()).as_dict()
    for k, v in host[0].items():
        if k in ("clk_total", "clk_serial"):
            continue
        assert np.array_equal(np.asarray(r[k]), np.asarray(v), equal_nan=True), k
    n, m = r["common_pt"], r["common_ls"]
    assert np.array_equal(pc.cpu().numpy()[:n], host[1]) and np.array_equal(pi.cpu().numpy()[:n].astype(bool), host[2])
    assert np.array_equal(lcr.cpu().numpy()[:m], host[3]) and np.array_equal(li.cpu().numpy()[:m].astype(bool), host[4])


def C_sizeof():
    import ctypes
    return ctypes.sizeof(plslam_amd.LcResult)


def test_one_record_as_both_keyframes_is_uploaded_once_and_equals_the_dev_form(ctx):
    """kf0 and kf1 the same record: the host form's image holds it once and both device records point into it.  257 points: one
    row past the gather's 256-row chunk; 3 lines."""
    torch = pytest.importorskip("torch")
    kf, _, _ = LC.keyframe_pair(83, 257, 3)
    p = LC.params()
    host = ctx.loop_closure_verify(p, kf, kf)
    assert host[0]["common_pt"] == 257 and host[0]["common_ls"] == 3          # every feature is its own nearest neighbour
    dev = torch.device("cuda:0")
    t = {k: torch.from_numpy(np.ascontiguousarray(kf[k])).to(dev) for k in ("pdesc", "P", "pl", "pt_idx", "ldesc", "sPeP", "le", "ls_idx")}
    rec = dict({k: v.data_ptr() for k, v in t.items()}, n_pt=257, n_ls=3)
    res = torch.zeros(C_sizeof(), dtype=torch.uint8, device=dev)
    pc = torch.zeros((257, 4), dtype=torch.int32, device=dev)
    pi = torch.zeros(257, dtype=torch.uint8, device=dev)
    lcr = torch.zeros((3, 4), dtype=torch.int32, device=dev)
    li = torch.zeros(3, dtype=torch.uint8, device=dev)
    s = torch.cuda.Stream(dev)
    ctx.loop_closure_verify_dev(p, rec, rec, res.data_ptr(), pc.data_ptr(), pi.data_ptr(), lcr.data_ptr(), li.data_ptr(),
                                stream=s.cuda_stream)
    s.synchronize()
    r = plslam_amd.LcResult.from_buffer_copy(res.cpu().numpy().tobytes()).as_dict()
    for k, v in host[0].items():
        if k in ("clk_total", "clk_serial"):
            continue
        assert np.array_equal(np.asarray(r[k]), np.asarray(v), equal_nan=True), k
    assert np.array_equal(pc.cpu().numpy(), host[1]) and np.array_equal(pi.cpu().numpy().astype(bool), host[2])
    assert np.array_equal(lcr.cpu().numpy(), host[3]) and np.array_equal(li.cpu().numpy().astype(bool), host[4])
    assert np.array_equal(host[1][:, 1], np.arange(257)) and np.array_equal(host[1][:, 3], np.arange(257))


def test_relpose_robust_gn_alone(ctx):
    kf0, kf1, _ = LC.keyframe_pair(91, 1500, 200)
    prm = LC.params_dict(LC.params())
    full = lc_ref.is_loop_closure(prm, OCAM, kf0, kf1)
    P, pl, S, le = full["corr_inputs"]
    ref = lc_ref.relpose_robust_gn(prm, OCAM, P, pl, S, le)
    d, pi, li = ctx.relpose_robust_gn(LC.params(), P, pl, S, le)
    assert np.array_equal(pi, ref["pt_inlier"]) and np.array_equal(li, ref["ls_inlier"]) and d["is_lc"] == ref["is_lc"]
    assert _rel(d["T_inc"], ref["T_inc"]) <= REL and abs(d["e"] - ref["e"]) <= REL * ref["e"]


def test_argument_validation(ctx):
    kf0, kf1, _ = LC.keyframe_pair(3, 50, 10)
    for bad in (dict(max_iters=-1), dict(max_iters_ref=-1), dict(max_iters=plslam_amd.capi.LC_MAX_ITERS + 1)):
        with pytest.raises(plslam_amd.PlslamError):
            ctx.loop_closure_verify(LC.params(**bad), kf0, kf1)
    L = plslam_amd.load()
    res = plslam_amd.LcResult()
    p = LC.params()
    assert L.plslam_loop_closure_verify(ctx._h, p, None, None, res, None, None, None, None) == plslam_amd.capi.EINVAL
    k = plslam_amd.LcKeyframe()
    k.n_pt = -1
    assert L.plslam_loop_closure_verify(ctx._h, p, k, k, res, None, None, None, None) == plslam_amd.capi.EINVAL
    k.n_pt = 3                                   # rows without arrays
    assert L.plslam_loop_closure_verify(ctx._h, p, k, k, res, None, None, None, None) == plslam_amd.capi.EINVAL
    assert L.plslam_relpose_robust_gn(ctx._h, p, None, None, 2, None, None, 0, res, None, None) == plslam_amd.capi.EINVAL


# ---- off the one forward-facing scene: tests/lc_cases.py (tests/test_lc_cpu.py shows what each case reaches) ---------------
def _verify_case(ctx, name, **over):
    prm_over, cam, kf0, kf1 = CASES.case(name)
    return ctx.loop_closure_verify(LC.params(cam, **dict(prm_over, **over)), kf0, kf1)


@pytest.mark.parametrize("name", CASES.VALUE_COMPARED)
def test_cases_against_the_restatement(ctx, name):
    ref, prm, _ = CASES.reference(name)
    dev = _verify_case(ctx, name)
    _check(*dev, ref, prm)
    assert dev[0]["gn_ran"] == 1


def test_a_pair_at_rest_with_points_is_exact(ctx):
    """still_p: every residual is exactly 0, so e == 0 and H == 0 whatever the summation order: all of it is compared exactly"""
    ref, prm, _ = CASES.reference("still_p")
    d, pc, pi, lc, li = _verify_case(ctx, "still_p")
    _check(d, pc, pi, lc, li, ref, prm)
    assert d["e"] == 0.0 and not np.asarray(d["H"]).any() and not np.asarray(d["g"]).any() and math.isnan(d["cov_eig"])
    assert (d["iters_1"], d["iters_2"]) == (1, 1) and d["is_lc"] == 0 and d["ok_unc"] == 0 and d["ok_res"] == 1
    assert np.array_equal(np.asarray(d["T_inc"]).reshape(4, 4), np.eye(4)) and d["t"] == 0.0 and d["r"] == 0.0
    assert not np.asarray(d["pose_inc"]).any() and pi.all() and d["n_pt_inliers"] == 257 and d["common_ls"] == 0


def test_a_pair_at_rest_with_lines_stops_on_a_small_error(ctx):
    """still_pl: e (1e-27) and H are rounding noise and the eigenvalue of H^-1 (1e8) is rounding-decided: the counts, rows,
    masks, iteration counts, flags and T_inc == I are what the data decide"""
    ref, prm, _ = CASES.reference("still_pl")
    d, pc, pi, lc, li = _verify_case(ctx, "still_pl")
    for k in ("common_pt", "common_ls", "gn_ran", "is_lc", "iters_1", "iters_2", "ok_unc", "n_pt_inliers", "n_ls_inliers",
              "inl_ratio_pt", "inl_ratio_ls"):
        assert d[k] == ref[k], (k, d[k], ref[k])
    assert (d["iters_1"], d["iters_2"]) == (1, 1) and d["is_lc"] == 0 and d["ok_unc"] == 0 and d["gn_ran"] == 1
    assert np.array_equal(pc, ref["pt_corr"]) and np.array_equal(lc, ref["ls_corr"]) and pi.all() and li.all()
    assert np.array_equal(np.asarray(d["T_inc"]).reshape(4, 4), np.eye(4))
    assert 0.0 <= d["e"] < lc_ref.EPS


def test_a_nan_landmark(ctx):
    ref, prm, _ = CASES.reference("nan_landmark")
    d, pc, pi, lc, li = _verify_case(ctx, "nan_landmark")
    _check(d, pc, pi, lc, li, ref, prm, nan_pattern=True)
    assert d["gn_ran"] == 1 and pi.all() and li.all() and (d["iters_1"], d["iters_2"]) == (5, 10) and d["is_lc"] == 0
    assert math.isnan(d["e"]) and math.isnan(d["cov_eig"])


@pytest.mark.parametrize("name", CASES.VALUE_COMPARED)
def test_first_system_against_long_double(ctx, name):
    """One iteration leaves the first system in the result.  The device sums the oracle's terms in a tree where the oracle sums
    them in sequence; one order says little about the tail of another, so the device may lie ten times as far from the
    long-double system as the oracle does on the same input (tests/test_lc_cpu.py prints that distance; DESIGN.md has both)"""
    ld, oracle_dist = CASES.first_system(name)
    d = _verify_case(ctx, name, max_iters=1, max_iters_ref=0)[0]
    assert (d["iters_1"], d["iters_2"]) == (1, 0)
    dist = lc_ref.system_distance(d["H"], d["g"], d["e"], ld)
    print(f"first system {name}: device {dist:.2e} oracle {oracle_dist:.2e}")
    assert dist <= 10.0 * oracle_dist, (name, dist, oracle_dist)


@pytest.mark.parametrize("name", sorted(CASES.IDENTITY))
def test_relpose_robust_gn_at_the_chunk_sizes(ctx, name):
    """the identity path (correspondence k is row k, no rows kept) with one kind only, at 255 / 256 / 257 points and at
    63 / 64 / 65 lines"""
    P, pl, S, le = CASES.identity_problem(name)
    ref, prm, _ = CASES.reference(name)
    d, pi, li = ctx.relpose_robust_gn(LC.params(), P, pl, S, le)
    _margins(ref, prm)
    assert (d["common_pt"], d["common_ls"]) == (len(P), len(S)) and d["gn_ran"] == 1
    assert np.array_equal(pi, ref["pt_inlier"]) and np.array_equal(li, ref["ls_inlier"])
    for k in ("is_lc", "ok_res", "ok_unc", "ok_inl", "ok_trs", "ok_rot", "n_pt_inliers", "n_ls_inliers", "iters_1", "iters_2"):
        assert d[k] == ref[k], (k, d[k], ref[k])
    for k in ("e", "t", "r", "cov_eig", "ratio_inliers"):
        assert abs(d[k] - ref[k]) <= REL * abs(ref[k]), (k, d[k], ref[k])
    assert _rel(d["T_inc"], ref["T_inc"]) <= REL and _rel(d["pose_inc"], ref["pose_inc"]) <= REL and ref["is_lc"] == 1
