"""GPU tests of the global bundle adjustment on the device-resident map: plslam_local_map_form_all + gather, the plan built on
the device (plslam_gba_plan_create_dev), plslam_gba_optimize_dev and the write-back plslam_local_map_apply_gba.  The yardstick
for every list is the HOST builder (a plan made by plslam_gba_plan_create from the same columns, downloaded through
plslam_gba_plan_lists); for the gather, the numpy restatement (tests/gba_dev_ref.py); for the optimisation, plslam_gba_optimize on
the host-built plan.  Everything compared is an integer or a bit pattern: every comparison is exact, there is no tolerance here."""
import numpy as np
import pytest

import gba_dev_cases as DC
import gba_dev_ref as R
import plslam_amd
from plslam_amd import capi, gba, synth
from plslam_amd import local_map as LM
from plslam_amd.capi import EINVAL, GbaPlan, PlslamError

pytestmark = pytest.mark.gpu
CAM = plslam_amd.make_cam(**{k: synth.EUROC[k] for k in ("fx", "fy", "cx", "cy", "b", "width", "height")})
_MAPS = {}


def _map(name):
    """the inputs, made once and shared (never written)"""
    if name not in _MAPS:
        _MAPS[name] = (DC.MAPS.get(name) or DC.COLUMNS[name])()
    return _MAPS[name]


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


def _same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    ne = np.flatnonzero(_bits(got).reshape(-1) != _bits(want).reshape(-1))
    assert ne.size == 0, f"{what}: {ne.size} entries differ, the first at flat index {ne[0]}: {got.reshape(-1)[ne[0]]} != {want.reshape(-1)[ne[0]]}"


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


def _host_plan(ctx, m):
    return GbaPlan(ctx, CAM, m["n_map_kf"], m["kf_list"], m["npt"], m["nls"], m["pt_obs"], m["pt_uv"], m["ls_obs"], m["ls_l"])


def _columns(ctx, m, **over):
    a = dict(kf_list=np.asarray(m["kf_list"], np.int32), pt_obs=np.asarray(m["pt_obs"], np.int32), pt_uv=np.asarray(m["pt_uv"], np.float64),
             ls_obs=np.asarray(m["ls_obs"], np.int32), ls_l=np.asarray(m["ls_l"], np.float64))
    a.update(over)
    return _Dev(ctx, **a), a


def _dev_plan(ctx, m, **over):
    d, a = _columns(ctx, m, **over)
    plan = GbaPlan.from_device(ctx, CAM, m["n_map_kf"], a["kf_list"].size, d.p("kf_list"), m["npt"], m["nls"], d.p("pt_obs"), d.p("pt_uv"),
                               a["pt_obs"].shape[0], d.p("ls_obs"), d.p("ls_l"), a["ls_obs"].shape[0])
    plan._keep = d
    return plan


def _gathered(ctx, m):
    ix = LM.DeviceMapIndex(gba.map_image(m), ctx.device)
    lm = LM.LocalMap(ctx)
    f = lm.form_all(ix)
    c = lm.gather(ix)
    return ix, lm, f, c


def _plan_from_gather(ctx, m, lm, c):
    b = lm.device_buffers()
    return GbaPlan.from_device(ctx, CAM, m["n_map_kf"], c["nkf"], b["kf_list"], c["npt"], c["nls"], b["pt_obs"], b["pt_obs_uv"],
                               c["n_pt_obs"], b["ls_obs"], b["ls_l_obs"], c["n_ls_obs"])


def _compare_lists(name, got, want):
    assert set(got) == set(want) == set(capi.GBA_LIST_NAMES)
    for k in capi.GBA_LIST_NAMES:
        _same(got[k], want[k], f"{name}: {k}")


# ---- 1. the lists equal the host builder's ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(DC.MAPS) + list(DC.COLUMNS))
def test_lists_equal_the_host_builders(ctx, name):
    m = _map(name)
    host, dev = _host_plan(ctx, m), _dev_plan(ctx, m)
    a, b = host.lists(), dev.lists()
    _compare_lists(name, b, a)
    # the cases are what their names say
    nkf = len(m["kf_list"])
    assert a["blk"].shape[0] >= nkf and (a["chk"][:, 3] >= 1).all() and (a["chk"][:, 3] <= 64).all()
    if name == "chunks":
        import gba_cases
        per = {(int(k1), int(k2)): (c0, c1) for k1, k2, c0, c1 in a["blk"]}
        for blk, (n_p, n_l) in gba_cases.CHUNK_BLOCKS.items():
            c0, c1 = per[blk]
            assert int(a["chk"][c0:c1][a["chk"][c0:c1, 1] == 0, 3].sum()) == n_p and int(a["chk"][c0:c1][a["chk"][c0:c1, 1] == 1, 3].sum()) == n_l
    if name == "ragged":
        assert a["blk"].shape[0] > 3 * DC.LOOKBACK                       # more blocks than one tile of the block compaction
        assert a["lpo"].size > 3 * DC.LOOKBACK                           # the pair enumeration spans more than three look-back tiles
    if name == "no_obs_keyframe":
        k1, k2, c0, c1 = a["blk"][-1]
        assert (k1, k2) == (nkf - 1, nkf - 1) and c0 == c1               # a diagonal block without a pair
    if name == "both_0":
        assert a["pair"].shape[0] == 0 and a["chk"].shape[0] == 0 and a["blk"].shape[0] == nkf
    if name == "twice":
        pr = {tuple(r) for r in a["pair"].tolist()}
        o = np.flatnonzero(m["pt_obs"][:, 1] == DC.TWICE_POINTS[0])
        o1 = [x for x in o if m["pt_obs"][x, 3] == m["pt_obs"][o[-1], 3]]
        assert len(o1) == 2 and (o1[0], o1[1]) in pr and (o1[1], o1[0]) in pr
    host.close()
    dev.close()


# ---- 2. the gather chain ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(DC.MAPS))
def test_form_all_and_gather_equal_the_restatement_and_feed_the_plan(ctx, name):
    m = _map(name)
    img = gba.map_image(m)
    ref = R.gba_gather(img)
    ix, lm, f, c = _gathered(ctx, m)
    assert f == dict(n_kf_local=int(img["kf_valid"].sum()), n_pt_local=m["npt"], n_ls_local=m["nls"])
    fl = lm.download("kf_local", "pt_local", "ls_local")
    _same(fl["kf_local"], img["kf_valid"], "kf_local")
    _same(fl["pt_local"], img["points"]["valid"], "pt_local")
    _same(fl["ls_local"], img["lines"]["valid"], "ls_local")
    got = lm.download(*R.GATHER_KEYS)
    for k in R.GATHER_KEYS:
        _same(got[k], ref[k], f"{name}: {k}")
    plan, up = _plan_from_gather(ctx, m, lm, c), _dev_plan(ctx, m)
    _compare_lists(name, plan.lists(), up.lists())
    plan.close()
    up.close()
    lm.close()


def test_form_all_on_a_map_with_null_slots_and_null_landmarks(ctx):
    m = LM.synthetic_map(n_kf=40, n_pt=600, n_ls=150, seed=1, null_kf=(3, 17, 39))
    ref = R.gba_gather(m)
    ix, lm = LM.DeviceMapIndex(m, ctx.device), LM.LocalMap(ctx)
    f = lm.form_all(ix)
    assert f == dict(n_kf_local=int(m["kf_valid"].sum()), n_pt_local=int(m["points"]["valid"].sum()), n_ls_local=int(m["lines"]["valid"].sum()))
    lm.gather(ix)
    got = lm.download(*R.GATHER_KEYS)
    for k in R.GATHER_KEYS:
        _same(got[k], ref[k], k)
    lm.close()


# ---- 3. same plan, same bits --------------------------------------------------------------------------------------------------
def _trace_bits(tr):
    return [tuple(np.float64(v).view(np.uint64) if isinstance(v, float) else v for v in t.values()) for t in tr]


def _result_bits(r):
    return tuple(np.float64(r[k]).view(np.uint64) if isinstance(r[k], float) else r[k]
                 for k in ("iters", "n_solves", "stop_reason", "err", "err_prev", "lam", "hmax"))


def _device_route(ctx, m):
    ix, lm, _, c = _gathered(ctx, m)
    plan = _plan_from_gather(ctx, m, lm, c)
    x = lm.device_buffers()["X_aux"]
    r = plan.optimize_dev(m["T_kf_w"], x, x + 8 * 6 * c["nkf"], x + 8 * (6 * c["nkf"] + 3 * c["npt"]), max_iters=3)
    lm.apply_gba(plan, ix)
    r["Xw"], r["Lw"] = ix.host("points.X").reshape(-1, 3), ix.host("lines.X").reshape(-1, 6)
    plan.close()
    lm.close()
    return r


@pytest.mark.parametrize("name", DC.OPTIMIZE)
def test_the_device_route_gives_the_host_routes_bits(ctx, name):
    m = _map(name)
    host = _host_plan(ctx, m)
    want = host.optimize(m["T_kf_w"], m["x_kf"], m["Xw"], m["Lw"], max_iters=3)
    host.close()
    a, b = _device_route(ctx, m), _device_route(ctx, m)
    for got in (a, b):
        for k in ("x_kf", "T", "Xw", "Lw"):
            _same(got[k], want[k], f"{name}: {k}")
        assert _trace_bits(got["trace"]) == _trace_bits(want["trace"]) and len(want["trace"]) == want["n_solves"] >= 1
        assert _result_bits(got) == _result_bits(want)
    if name == "nan_landmark":
        assert np.isnan(want["Xw"]).any() and np.isnan(want["Lw"]).any()


def test_the_host_loop_works_on_a_device_built_plan_and_the_device_loop_on_a_host_built_one(ctx):
    m = _map("gaps")
    host, dev = _host_plan(ctx, m), _dev_plan(ctx, m)
    want = host.optimize(m["T_kf_w"], m["x_kf"], m["Xw"], m["Lw"], max_iters=3)
    got = dev.optimize(m["T_kf_w"], m["x_kf"], m["Xw"], m["Lw"], max_iters=3)
    for k in ("x_kf", "T", "Xw", "Lw"):
        _same(got[k], want[k], k)
    d = _Dev(ctx, x=m["x_kf"], X=m["Xw"], L=m["Lw"])
    got = host.optimize_dev(m["T_kf_w"], d.p("x"), d.p("X"), d.p("L"), max_iters=3)
    for k in ("x_kf", "T"):
        _same(got[k], want[k], k)
    assert _trace_bits(got["trace"]) == _trace_bits(want["trace"])
    host.close()
    dev.close()


# ---- 4. the write-back --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("npt,nls", [(0, 1), (1, 0), (63, 65), (64, 64), (65, 63)])
def test_write_back_copies_the_listed_landmarks_and_nothing_else(ctx, npt, nls):
    """npt listed points and nls listed lines among NULL ones (list lengths 0, 1, 63, 64, 65 of either kind); the plan is the map's
    own (nkf = 1), optimised twice"""
    base = gba.trajectory_map(n_kf=2, n_pt=npt, n_ls=nls, obs_per_lm=2, loop=False, seed=50 + npt)
    img = gba.map_image(base)
    # NULL landmarks in between: every other slot of a longer image is a NULL landmark with its own coordinates
    rng = np.random.Generator(np.random.PCG64(npt))
    for kind, dl in (("points", 3), ("lines", 6)):
        K = img[kind]
        k = K["n"]
        valid = np.zeros(2 * k + 3, np.uint8)
        valid[1:2 * k:2] = 1
        X = rng.uniform(-9, 9, (2 * k + 3, dl))
        X[valid != 0] = K["X"]
        cnt = np.zeros(2 * k + 3, np.int64)
        cnt[valid != 0] = np.diff(K["obs_ptr"])
        K.update(n=2 * k + 3, valid=valid, X=X, obs_ptr=np.concatenate([[0], np.cumsum(cnt)]).astype(np.int32),
                 inlier=rng.integers(0, 256, 2 * k + 3).astype(np.uint8))             # a sentinel pattern, not flags
    ix, lm = LM.DeviceMapIndex(img, ctx.device), LM.LocalMap(ctx)
    lm.form_all(ix)
    c = lm.gather(ix)
    assert (c["npt"], c["nls"]) == (base["npt"], base["nls"]) == (npt, nls)
    plan = _plan_from_gather(ctx, base, lm, c)
    x = lm.device_buffers()["X_aux"]
    plan.optimize_dev(base["T_kf_w"], x, x + 48 * c["nkf"], x + 48 * c["nkf"] + 24 * c["npt"], max_iters=2)
    # the plan's landmarks, read through the host loop's outputs of the same plan from the same start
    want = plan.optimize(base["T_kf_w"], base["x_kf"], base["Xw"], base["Lw"], max_iters=2)
    lm.apply_gba(plan, ix)
    g = lm.download("pt_list", "ls_list")
    for kind, tag, dl, new in (("points", "pt", 3, want["Xw"]), ("lines", "ls", 6, want["Lw"])):
        X = ix.host(kind + ".X").reshape(-1, dl)
        lst = g[tag + "_list"]
        _same(X[lst], new, kind + ": the listed landmarks")
        rest = np.setdiff1d(np.arange(img[kind]["n"]), lst)
        _same(X[rest], img[kind]["X"][rest], kind + ": the landmarks not listed")
        _same(ix.host(kind + ".inlier"), img[kind]["inlier"], kind + ": inlier")
        if lst.size:
            assert (_bits(X[lst]) != _bits(img[kind]["X"][lst])).any()            # the optimisation moved them
    plan.close()
    lm.close()


# ---- 5. refusals ----------------------------------------------------------------------------------------------------------------
def _refused(fn, code=EINVAL):
    with pytest.raises(PlslamError) as e:
        fn()
    assert e.value.code == code, e.value


def test_refusals_leave_the_context_usable(ctx):
    m = _map("nkf16")
    nkf, n_map = len(m["kf_list"]), m["n_map_kf"]
    # device-side: one bad entry each
    for col, val in ((1, m["npt"]), (1, -1), (3, n_map), (3, -1), (4, nkf), (4, -2)):
        bad = m["pt_obs"].copy()
        bad[7, col] = val
        _refused(lambda: _dev_plan(ctx, m, pt_obs=bad))
        bad = m["ls_obs"].copy()
        bad[3, col] = m["nls"] if (col, val) == (1, m["npt"]) else val
        _refused(lambda: _dev_plan(ctx, m, ls_obs=bad))
    bad = m["pt_obs"].copy()                                             # kf_list[v4] != v3
    r = int(np.flatnonzero(bad[:, 4] >= 0)[0])
    bad[r, 3] = bad[r, 3] % (n_map - 1) + 1 if bad[r, 3] % (n_map - 1) + 1 != bad[r, 3] else 1
    assert m["kf_list"][bad[r, 4]] != bad[r, 3]
    _refused(lambda: _dev_plan(ctx, m, pt_obs=bad))
    for val in (n_map, -1):                                              # a kf_list entry out of range (no observation names it)
        kl = np.concatenate([m["kf_list"], [val]]).astype(np.int32)
        d, a = _columns(ctx, m, kf_list=kl)
        _refused(lambda: GbaPlan.from_device(ctx, CAM, n_map, nkf + 1, d.p("kf_list"), m["npt"], m["nls"], d.p("pt_obs"), d.p("pt_uv"),
                                             a["pt_obs"].shape[0], d.p("ls_obs"), d.p("ls_l"), a["ls_obs"].shape[0]))
    # before anything is launched
    d, a = _columns(ctx, m)
    np_, nl_ = a["pt_obs"].shape[0], a["ls_obs"].shape[0]

    def make(n_map=n_map, nkf=nkf, kl=d.p("kf_list"), npt=m["npt"], nls=m["nls"], po=d.p("pt_obs"), uv=d.p("pt_uv"), np_=np_, lo=d.p("ls_obs"),
             ll=d.p("ls_l"), nl_=nl_, th=1e-7):
        return GbaPlan.from_device(ctx, CAM, n_map, nkf, kl, npt, nls, po, uv, np_, lo, ll, nl_, homog_th=th)

    for kw in (dict(nkf=0), dict(nkf=capi.GBA_MAX_KEYFRAMES + 1), dict(th=1e-6), dict(kl=0), dict(po=0), dict(uv=0), dict(lo=0), dict(ll=0),
               dict(npt=-1), dict(nls=-1), dict(np_=-1), dict(nl_=-1), dict(n_map=-1), dict(n_map=0), dict(npt=0), dict(nls=0),
               dict(np_=(2**31 - 1) // 18 + 1), dict(nl_=(2**31 - 1) // 36 + 1), dict(npt=(2**31 - 1) // 9 + 1), dict(nls=(2**31 - 1) // 36 + 1)):
        _refused(lambda: make(**kw))
    # the context and a handle are usable afterwards
    plan = make()
    host = _host_plan(ctx, m)
    _compare_lists("after the refusals", plan.lists(), host.lists())
    plan.close()
    host.close()


def test_apply_gba_refusals(ctx):
    m, other = _map("nkf16"), _map("twice")
    ix, lm = LM.DeviceMapIndex(gba.map_image(m), ctx.device), LM.LocalMap(ctx)
    plan = _dev_plan(ctx, m)
    lm.form_all(ix)
    _refused(lambda: lm.apply_gba(plan, ix))                             # before gather
    c = lm.gather(ix)
    _refused(lambda: lm.apply_gba(plan, ix))                             # before optimize
    x = lm.device_buffers()["X_aux"]
    small = _dev_plan(ctx, other)
    d = _Dev(ctx, x=other["x_kf"], X=other["Xw"], L=other["Lw"])
    small.optimize_dev(other["T_kf_w"], d.p("x"), d.p("X"), d.p("L"), max_iters=1)
    _refused(lambda: lm.apply_gba(small, ix))                            # a plan of other counts
    ctx2 = plslam_amd.Context(0)
    try:
        foreign = _dev_plan(ctx2, m)
        d2 = _Dev(ctx2, x=m["x_kf"], X=m["Xw"], L=m["Lw"])
        foreign.optimize_dev(m["T_kf_w"], d2.p("x"), d2.p("X"), d2.p("L"), max_iters=1)
        _refused(lambda: lm.apply_gba(foreign, ix))                      # another context's plan
        foreign.close()
    finally:
        ctx2.close()
    before = ix.host("points.X")
    plan.optimize_dev(m["T_kf_w"], x, x + 48 * c["nkf"], x + 48 * c["nkf"] + 24 * c["npt"], max_iters=1)
    lm.apply_gba(plan, ix)                                               # and the handle still works
    assert (_bits(ix.host("points.X")) != _bits(before)).any()
    for p in (plan, small):
        p.close()
    lm.close()
