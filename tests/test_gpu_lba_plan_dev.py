"""GPU tests of the LBA plan built on the device (plslam_lba_plan_create_dev) and of the write-back into the map image
(plslam_local_map_apply_lba).  The yardstick for every list is the HOST builder: a plan made by plslam_lba_plan_create from the
same columns, downloaded through plslam_lba_plan_lists.  Everything compared is an integer or a verbatim double: every comparison
is exact, there is no tolerance in this file."""
import numpy as np
import pytest

import lba_plan_dev_cases as PC
import local_map_cases as CS
import plslam_amd
from plslam_amd import local_map as LM
from plslam_amd import synth
from plslam_amd.capi import EINVAL, LbaPlan, PlslamError

pytestmark = pytest.mark.gpu

_LISTS = ("pt_ptr", "pt_ids", "ls_ptr", "ls_ids", "kf_ptr", "kf_ids", "pt_lm_loc", "pt_pose_slot", "pt_kf_loc", "pt_obs_uv", "ls_lm_loc",
          "ls_pose_slot", "ls_kf_loc", "ls_l_obs", "blk_ptr", "pairs")
_COLS = ("pt_lm", "pt_slot", "pt_kf_loc", "pt_obs_uv", "ls_lm", "ls_slot", "ls_kf_loc", "ls_l_obs")


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


def _same(a, b, what=""):
    a, b = np.asarray(a), np.asarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape, (what, a.dtype, b.dtype, a.shape, b.shape)
    assert np.array_equal(_bits(a), _bits(b)), what


def _cam():
    return plslam_amd.make_cam(**synth.EUROC)


class _Dev:
    """device copies of host arrays (kept alive); .p(name) -> the device pointer, 0 for an empty array"""

    def __init__(self, ctx, **arrays):
        import torch
        self._t = {}
        for k, a in arrays.items():
            a = np.ascontiguousarray(a)
            self._t[k] = (torch.from_numpy(a.copy() if a.size else np.zeros(1, a.dtype)).to(torch.device("cuda", ctx.device)), a.size)
        torch.cuda.synchronize()

    def p(self, k):
        t, n = self._t[k]
        return t.data_ptr() if n else 0


def _host_plan(ctx, c):
    return LbaPlan(ctx, _cam(), 1e-7, c["n_pose_slots"], c["nkf"], c["npt"], c["nls"], c["pt_lm"], c["pt_slot"], c["pt_kf_loc"],
                   c["pt_obs_uv"], c["ls_lm"], c["ls_slot"], c["ls_kf_loc"], c["ls_l_obs"])


def _dev_plan(ctx, c):
    d = _Dev(ctx, **{k: c[k] for k in _COLS})
    plan = LbaPlan.from_device(ctx, _cam(), 1e-7, c["n_pose_slots"], c["nkf"], c["npt"], c["nls"], d.p("pt_lm"), d.p("pt_slot"),
                               d.p("pt_kf_loc"), d.p("pt_obs_uv"), c["pt_lm"].size, d.p("ls_lm"), d.p("ls_slot"), d.p("ls_kf_loc"),
                               d.p("ls_l_obs"), c["ls_lm"].size)
    plan._keep = d                                                       # (the columns are read at creation only; kept all the same)
    return plan


# ---- 1. the lists equal the host builder's ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(PC.CASES))
def test_lists_equal_the_host_builders(ctx, name):
    c = PC.CASES[name]()
    host, dev = _host_plan(ctx, c), _dev_plan(ctx, c)
    a, b = host.lists(prepare_schur=True), dev.lists(prepare_schur=True)
    assert set(a) == set(b) == set(_LISTS) | {"max_chunks", "schur_chunks"}
    for k in _LISTS:
        _same(b[k], a[k], f"{name}: {k}")
    assert b["max_chunks"] == a["max_chunks"] and b["schur_chunks"] == a["schur_chunks"], name
    # the cases are what their names say
    nblk = c["nkf"] * (c["nkf"] + 1) // 2
    assert a["blk_ptr"].size == nblk + 1 and a["kf_ids"].size == int((c["pt_kf_loc"] >= 0).sum() + (c["ls_kf_loc"] >= 0).sum())
    if name == "no_optimised_keyframe":
        assert a["kf_ids"].size == 0 and a["pairs"].shape[0] == 0 and a["max_chunks"] == 0
    if name == "twice_by_one_keyframe":
        pr = {tuple(r) for r in a["pairs"].tolist()}
        assert (0, 2, 1, 0) in pr and (2, 0, 1, 0) in pr               # both orders of the two observations of landmark 1 by keyframe 2
    if name == "nkf_23":
        assert nblk == 276
    if name == "npt_over_65536":
        assert c["npt"] > 65536
    if name.startswith("block_6"):
        n_null = int((a["pairs"][:, 3] == 2).sum())
        assert n_null == (0 if name == "block_64_point_pairs" else 3 * 63), n_null
    if name == "keyframe_63_64_65":
        assert np.diff(a["kf_ptr"]).tolist() == [63, 64, 65] and a["max_chunks"] == 2
    if name.startswith("both_") and c["pt_lm"].size > 1:
        assert (np.diff(c["pt_lm"]) < 0).any()                          # lm_loc is NOT sorted
    host.close()
    dev.close()


# ---- the scene the numeric tests share: local_map_cases.mixed(700) with its landmarks in front of the cameras --------------------
def _scene():
    m, p = CS.mixed(700)
    rng = np.random.Generator(np.random.PCG64(3))
    P, L = m["points"], m["lines"]
    P["X"][:] = rng.uniform(-3, 3, P["X"].shape) + [0, 0, 12]
    L["X"][:] = rng.uniform(-3, 3, L["X"].shape) + [0, 0, 12, 0, 0, 12]
    T = np.stack([synth.se3_exp(0.05 * rng.standard_normal(6)) for _ in range(m["n_map_kf"])]).reshape(-1, 16)
    return m, p, T


def _gathered(ctx, m, p):
    ix = LM.DeviceMapIndex(m, ctx.device)
    lm = LM.LocalMap(ctx)
    lm.form(ix, p["anchor"], m["row"], p["min_cov"], p["window"])
    c = lm.gather(ix)
    return ix, lm, c


def _slots(T, g):
    """the pose slots of optimize(): the stored pose of every map keyframe, then the estimates of the optimised ones"""
    return np.concatenate([T, T[g["kf_list"]]])


def _plan_from_gather(ctx, m, lm, c):
    b, n = lm.device_buffers(), m["n_map_kf"]
    return LbaPlan.from_device(ctx, _cam(), 1e-7, n + c["nkf"], c["nkf"], c["npt"], c["nls"], b["pt_lm_loc"], b["pt_pose_slot"],
                               b["pt_kf_loc"], b["pt_obs_uv"], c["n_pt_obs"], b["ls_lm_loc"], b["ls_pose_slot"], b["ls_kf_loc"],
                               b["ls_l_obs"], c["n_ls_obs"], b["X_aux"] + 8 * 6 * c["nkf"], b["X_aux"] + 8 * (6 * c["nkf"] + 3 * c["npt"]), n)


def _host_plan_from_gather(ctx, m, g):
    n, nkf = m["n_map_kf"], len(g["kf_list"])
    slot = np.where(g["pt_kf_loc"] >= 0, n + g["pt_kf_loc"], g["pt_pose_slot"]).astype(np.int32)
    return LbaPlan(ctx, _cam(), 1e-7, n + nkf, nkf, len(g["pt_list"]), len(g["ls_list"]), g["pt_lm_loc"], slot, g["pt_kf_loc"],
                   g["pt_obs_uv"], g["ls_lm_loc"], g["ls_pose_slot"], g["ls_kf_loc"], g["ls_l_obs"])


def _lm_step(plan, first):
    """iterate -> diag_max -> schur(lambda) -> the host's solve -> backsub(apply) -> landmarks; `first`: the plan's first iteration"""
    err = first()
    hmax = plan.diag_max()
    S, b, nsing = plan.schur(1e-5 * hmax)
    dp = np.linalg.solve(S, b)
    dxp, dxl = plan.backsub(dp, apply=True)
    X, Lw = plan.get_landmarks()
    return dict(err=np.float64(err), hmax=np.float64(hmax), S=S, b=b, nsing=np.int32(nsing), dp=dp, dxp=dxp, dxl=dxl, X=X, L=Lw)


# ---- 2. same plan, same bits; 3. the slot rewrite -----------------------------------------------------------------------------
def test_same_plan_same_bits_and_the_slot_rewrite(ctx):
    m, p, T = _scene()
    ix, lm, c = _gathered(ctx, m, p)
    g = lm.download()
    n = m["n_map_kf"]
    assert c["nkf"] > 2 and c["n_pt_obs"] > 300 and c["n_ls_obs"] > 100 and (g["pt_kf_loc"] == -1).any() and (g["pt_kf_loc"] >= 0).any()
    Ts = _slots(T, g)
    dev, host = _plan_from_gather(ctx, m, lm, c), _host_plan_from_gather(ctx, m, g)
    # the slot rewrite, on the gather's columns
    ld = dev.lists()
    _same(ld["pt_pose_slot"], np.where(g["pt_kf_loc"] >= 0, n + g["pt_kf_loc"], g["pt_pose_slot"]).astype(np.int32), "pt_pose_slot")
    _same(ld["ls_pose_slot"], g["ls_pose_slot"], "ls_pose_slot")
    assert (ld["pt_pose_slot"] != g["pt_pose_slot"]).any()
    # the device-built plan: landmarks from X_aux on the device, poses from set_poses; the host-built plan: an uploading iterate
    x = g["X_aux"][6 * c["nkf"]:]
    X0, L0 = x[:3 * c["npt"]].reshape(-1, 3), x[3 * c["npt"]:].reshape(-1, 6)

    def first_dev():
        dev.set_poses(Ts)
        return dev.iterate_resident()
    a = _lm_step(dev, first_dev)
    b = _lm_step(host, lambda: host.iterate_dev(Ts, X0, L0, want_g=False)[0])
    assert np.isfinite(a["err"]) and a["err"] > 0 and np.isfinite(a["X"]).all() and np.isfinite(a["S"]).all()
    for k in a:
        _same(a[k], b[k], k)
    ba, bb = dev.blocks(), host.blocks()
    for k in ba:
        _same(np.float64(ba[k]) if k == "err" else ba[k], np.float64(bb[k]) if k == "err" else bb[k], k)
    assert not np.array_equal(a["X"], X0)                                # the step moved the landmarks
    # s + nkf > n_pose_slots
    b_ = lm.device_buffers()
    with pytest.raises(PlslamError) as e:
        LbaPlan.from_device(ctx, _cam(), 1e-7, n + c["nkf"], c["nkf"], c["npt"], c["nls"], b_["pt_lm_loc"], b_["pt_pose_slot"],
                            b_["pt_kf_loc"], b_["pt_obs_uv"], c["n_pt_obs"], b_["ls_lm_loc"], b_["ls_pose_slot"], b_["ls_kf_loc"],
                            b_["ls_l_obs"], c["n_ls_obs"], 0, 0, n + 1)
    assert e.value.code == EINVAL
    for q in (dev, host, lm):
        q.close()


# ---- 4. refusals ------------------------------------------------------------------------------------------------------------------
def test_refusals(ctx):
    c = PC.random_case(300, 120, seed=21)
    good = _dev_plan(ctx, c)
    ref = good.lists(prepare_schur=True)
    good.close()
    bad_values = dict(pt_lm=(c["npt"], -1), pt_kf_loc=(c["nkf"], -2), pt_slot=(c["n_pose_slots"], -1),
                      ls_lm=(c["nls"], -1), ls_kf_loc=(c["nkf"], -2), ls_slot=(c["n_pose_slots"], -1))
    for col, values in bad_values.items():
        for v in values:
            bad = dict(c, **{col: c[col].copy()})
            bad[col][c[col].size // 2] = v                              # ONE entry out of range: a range check, no index is followed
            with pytest.raises(PlslamError) as e:
                _dev_plan(ctx, bad)
            assert e.value.code == EINVAL, (col, v)
    # NULL and negative arguments: refused before anything is launched
    d = _Dev(ctx, **{k: c[k] for k in _COLS})

    def create(n_pose_slots=c["n_pose_slots"], nkf=c["nkf"], npt=c["npt"], nls=c["nls"], np_=c["pt_lm"].size, nl=c["ls_lm"].size, null=(),
               first=-1):
        q = lambda k: 0 if k in null else d.p(k)                        # noqa: E731
        return LbaPlan.from_device(ctx, _cam(), 1e-7, n_pose_slots, nkf, npt, nls, q("pt_lm"), q("pt_slot"), q("pt_kf_loc"), q("pt_obs_uv"),
                                   np_, q("ls_lm"), q("ls_slot"), q("ls_kf_loc"), q("ls_l_obs"), nl, 0, 0, first)
    for kw in ([dict(null=(k,)) for k in _COLS] + [dict(n_pose_slots=-1), dict(nkf=-1), dict(npt=-1), dict(nls=-1), dict(np_=-1), dict(nl=-1),
                                                  dict(first=-2), dict(npt=0), dict(nls=0), dict(n_pose_slots=0)]):
        with pytest.raises(PlslamError) as e:
            create(**kw)
        assert e.value.code == EINVAL, kw
    # the context is still usable: one more good create, the same lists
    again = create()
    got = again.lists(prepare_schur=True)
    for k in _LISTS:
        _same(got[k], ref[k], k)
    again.close()


# ---- 5. the write-back -------------------------------------------------------------------------------------------------------------
def _moved(before, after):
    """LbaPlanSolver::movedLandmarks' operations: d = after - before per component, s2 summed left to right from 0, sqrt(s2)"""
    s2 = np.zeros(before.shape[0])
    for a in range(before.shape[1]):
        d = after[:, a] - before[:, a]
        s2 = s2 + d * d
    return np.sqrt(s2)


def _write_back(m, g, Xn, Ln, th):
    """:1828-1855 on host arrays -> (the four image arrays after it, the two masks)"""
    out, masks = {}, []
    for kind, lst, new in (("points", g["pt_list"], Xn), ("lines", g["ls_list"], Ln)):
        X, inl = m[kind]["X"].copy(), m[kind]["inlier"].copy()
        mv = _moved(X[lst], new) > th
        inl[lst[mv]] = 0
        X[lst] = new
        out[kind + ".X"], out[kind + ".inlier"] = X, inl
        masks.append(mv.astype(np.uint8))
    return out, masks


def _image(ix):
    return {f"{k}.{f}": ix.host(f"{k}.{f}").reshape(-1) for k in ("points", "lines") for f in ("X", "inlier", "valid", "feat_idx")}


_WB_CASES = {**{f"exact_{n}": (lambda n=n: CS.exact(n)) for n in (0, 1, 63, 64, 65)}, "points_only": CS.CASES["points_only"],
             "lines_only": CS.CASES["lines_only"], "mixed_300": lambda: CS.mixed(300)}


@pytest.mark.parametrize("name", list(_WB_CASES))
def test_write_back_equals_the_restatement(ctx, name):
    m, p = _WB_CASES[name]()
    th = 0.01
    rng = np.random.Generator(np.random.PCG64(11))
    ref_g, _ = CS.run_ref(m, p)
    # the landmarks on the threshold: the first three listed points sit at the origin and move along ONE axis, so sqrt(s2) is exact
    pl = ref_g["pt_list"]
    edge = pl[:3] if len(pl) >= 3 else pl[:0]
    m["points"]["X"][edge] = 0.0
    m["points"]["inlier"][edge] = 1
    still = pl[3:5] if len(pl) >= 5 else pl[:0]                           # already outliers that do not move
    m["points"]["inlier"][still] = 0
    ix, lm, c = _gathered(ctx, m, p)
    g = lm.download()
    _same(g["pt_list"], ref_g["pt_list"])
    Xn = m["points"]["X"][g["pt_list"]] + rng.choice([0.0, 0.004, 0.02], (c["npt"], 3)) * rng.choice([-1.0, 1.0], (c["npt"], 3))
    Ln = m["lines"]["X"][g["ls_list"]] + rng.choice([0.0, 0.003, 0.02], (c["nls"], 6)) * rng.choice([-1.0, 1.0], (c["nls"], 6))
    if len(edge):
        Xn[:3] = [[th, 0, 0], [0, np.nextafter(th, np.inf), 0], [0, 0, -th]]
        Xn[3:5] = m["points"]["X"][still]
    n = m["n_map_kf"]
    plan = LbaPlan(ctx, _cam(), 1e-7, n, c["nkf"], c["npt"], c["nls"], g["pt_lm_loc"], g["pt_pose_slot"], g["pt_kf_loc"], g["pt_obs_uv"],
                   g["ls_lm_loc"], g["ls_pose_slot"], g["ls_kf_loc"], g["ls_l_obs"])
    before = _image(ix)
    # the three refusals, the image untouched
    fresh = LM.LocalMap(ctx)
    fresh.form(ix, p["anchor"], m["row"], p["min_cov"], p["window"])
    other = LbaPlan(ctx, _cam(), 1e-7, n, 0, c["npt"] + 1, c["nls"], *[np.zeros(0, np.int32)] * 3, np.zeros((0, 2)),
                    *[np.zeros(0, np.int32)] * 3, np.zeros((0, 3)))
    other.iterate_dev(np.tile(np.eye(4).reshape(-1), (n, 1)), np.zeros((c["npt"] + 1, 3)), np.zeros((c["nls"], 6)), want_g=False)
    for who, pl_ in ((fresh, plan), (lm, other), (lm, plan)):            # no gather | other counts | the state is not resident
        with pytest.raises(PlslamError) as e:
            who.apply_lba(pl_, ix, th)
        assert e.value.code == EINVAL
    after = _image(ix)
    for k in before:
        _same(after[k], before[k], k)
    fresh.close()
    other.close()
    # the state becomes resident: the poses do not matter to the write-back
    plan.iterate_dev(np.tile(np.eye(4).reshape(-1), (n, 1)), Xn, Ln, want_g=False)
    counts = lm.apply_lba(plan, ix, th)                                   # in place on the image's own arrays
    want, (mp, ml) = _write_back(m, g, Xn, Ln, th)
    got = _image(ix)
    for k in ("points.X", "points.inlier", "lines.X", "lines.inlier"):
        _same(got[k], want[k].reshape(-1), k)                            # landmarks not in the lists included
    for k in ("points.valid", "points.feat_idx", "lines.valid", "lines.feat_idx"):
        _same(got[k], before[k], k)
    masks = lm.download("pt_moved", "ls_moved")
    _same(masks["pt_moved"], mp)
    _same(masks["ls_moved"], ml)
    assert counts == dict(n_pt_moved=int(mp.sum()), n_ls_moved=int(ml.sum()))
    if len(edge):
        assert mp[:5].tolist() == [0, 1, 0, 0, 0]                         # on the threshold: kept; one ulp past it: cleared
        assert got["points.inlier"][edge].tolist() == [1, 0, 1] and got["points.inlier"][still].tolist() == [0, 0]
    if name == "mixed_300":
        assert mp.any() and ml.any() and not mp.all() and c["npt"] < m["points"]["n"]
    plan.close()
    lm.close()


# ---- 6. the chain on the image -----------------------------------------------------------------------------------------------------
def test_the_chain_on_the_image_equals_the_host_route(ctx):
    """form -> gather -> from_device straight from device_buffers() -> set_poses -> one LM step -> apply_lba -> cull, against the
    host route: download of the gather, host LbaPlan, the same step, get_landmarks, the numpy write-back, upload, cull.  The image
    must agree to the bit after the cull.  The cull skips LOCAL landmarks (removeBadMapLandmarks: !local), and every landmark the
    write-back touches is local to the form it was gathered under: a landmark the write-back turned into an outlier can only go at
    a cull under a LATER form.  So both routes then form the next keyframe's (narrower) local map and cull again -- that cull must
    remove a landmark that had enough observations and was an inlier before the write-back."""
    m, p, T = _scene()
    th = 0.01
    # ---- the device route
    ix, lm, c = _gathered(ctx, m, p)
    g = lm.download()
    Ts = _slots(T, g)
    dev = _plan_from_gather(ctx, m, lm, c)
    dev.set_poses(Ts)
    dev.iterate_resident()
    S, b, _ = dev.schur(1e-5 * dev.diag_max())
    dev.backsub(np.linalg.solve(S, b), apply=True, want=False)
    moved = lm.apply_lba(dev, ix, th)
    masks = lm.download("pt_moved", "ls_moved")
    lm.cull(ix, p["max_kf_idx"], p["min_lm_obs"])
    dev_first = _image(ix)
    lm.form(ix, p["anchor"], m["row"], 10 ** 6, -1)                       # the next form: the anchor alone is local
    lm.cull(ix, p["max_kf_idx"], p["min_lm_obs"])
    dev_removed = lm.download("pt_removed", "ls_removed")
    dev_second = _image(ix)
    # ---- the host route
    host = _host_plan_from_gather(ctx, m, g)
    x = g["X_aux"][6 * c["nkf"]:]
    host.iterate_dev(Ts, x[:3 * c["npt"]].reshape(-1, 3), x[3 * c["npt"]:].reshape(-1, 6), want_g=False)
    S2, b2, _ = host.schur(1e-5 * host.diag_max())
    host.backsub(np.linalg.solve(S2, b2), apply=True, want=False)
    Xn, Ln = host.get_landmarks()
    want, (mp, ml) = _write_back(m, g, Xn, Ln, th)
    m2 = dict(m, points=dict(m["points"], X=want["points.X"], inlier=want["points.inlier"]),
              lines=dict(m["lines"], X=want["lines.X"], inlier=want["lines.inlier"]))
    ix2 = LM.DeviceMapIndex(m2, ctx.device)
    lm2 = LM.LocalMap(ctx)
    lm2.form(ix2, p["anchor"], m["row"], p["min_cov"], p["window"])
    lm2.cull(ix2, p["max_kf_idx"], p["min_lm_obs"])
    host_first = _image(ix2)
    lm2.form(ix2, p["anchor"], m["row"], 10 ** 6, -1)
    lm2.cull(ix2, p["max_kf_idx"], p["min_lm_obs"])
    host_second = _image(ix2)
    for k in dev_first:
        _same(dev_first[k], host_first[k], "after the cull: " + k)
        _same(dev_second[k], host_second[k], "after the next form's cull: " + k)
    _same(masks["pt_moved"], mp)
    _same(masks["ls_moved"], ml)
    assert moved == dict(n_pt_moved=int(mp.sum()), n_ls_moved=int(ml.sum())) and mp.any()
    # not vacuous: a point the write-back turned into an outlier -- an inlier before, with enough observations to stay -- is removed
    P = m["points"]
    was_inlier = P["inlier"][g["pt_list"]] != 0
    enough = np.diff(P["obs_ptr"])[g["pt_list"]] >= p["min_lm_obs"]
    turned = g["pt_list"][(mp != 0) & was_inlier & enough]
    assert turned.size and dev_removed["pt_removed"][turned].any()
    for q in (dev, host, lm, lm2):
        q.close()
