"""GPU tests of the local map on the device (plslam_local_map_*): every output bit-exact against the sequential restatement
(tests/local_map_ref.py) on the shared cases (tests/local_map_cases.py: list lengths and observation counts 0, 1, T-1, T, T+1,
3T+37 around the look-back tile T, one keyframe, everything / only the anchor local, NULL slots, NULL features, one kind only, no
observation at all, the cull's edges, both overloads of form), on one ~100 k-landmark map, and through the two consumers: the
candidate mask into the map <-> keyframe driver, the gathered columns into the LBA plan."""
import numpy as np
import pytest

import local_map_cases as CS
from plslam_amd import local_map as LM
from plslam_amd import synth

pytestmark = pytest.mark.gpu

_EXACT = ("kf_local", "pt_local", "ls_local", "pt_candidate", "ls_candidate", "kf_list", "pt_list", "ls_list", "pt_obs", "ls_obs",
          "pt_lm_loc", "pt_kf_loc", "pt_pose_slot", "ls_lm_loc", "ls_kf_loc", "ls_pose_slot", "pt_obs_uv", "ls_l_obs", "X_aux",
          "pt_removed", "ls_removed")


def _run_device(ctx, m, p):
    """the four calls in the order addKeyFrame makes them -> (every output, the counts, the index after the cull)"""
    ix = LM.DeviceMapIndex(m, ctx.device)
    lm = LM.LocalMap(ctx)
    counts = lm.form(ix, p["anchor"], m["row"], p["min_cov"], p["window"])
    lm.candidates(ix, p["kf2"])
    counts.update(lm.gather(ix))
    counts.update(lm.cull(ix, p["max_kf_idx"], p["min_lm_obs"]))
    out = lm.download()
    after = {f"{k}.{f}": ix.host(f"{k}.{f}") for k in ("points", "lines") for f in ("valid", "feat_idx")}
    lm.close()
    return out, counts, after


def _check(m, p, out, counts, after):
    ref, m_after = CS.run_ref(m, p)
    for k in _EXACT:
        assert out[k].dtype == ref[k].dtype and out[k].shape == ref[k].shape, (k, out[k].shape, ref[k].shape)
        if out[k].dtype == np.float64:
            assert np.array_equal(out[k].view(np.uint64), ref[k].view(np.uint64)), k      # verbatim copies of doubles
        else:
            assert np.array_equal(out[k], ref[k]), k
    assert counts == dict(n_kf_local=int(ref["kf_local"].sum()), n_pt_local=int(ref["pt_local"].sum()),
                          n_ls_local=int(ref["ls_local"].sum()), nkf=len(ref["kf_list"]), npt=len(ref["pt_list"]),
                          nls=len(ref["ls_list"]), n_pt_obs=len(ref["pt_obs"]), n_ls_obs=len(ref["ls_obs"]), empty=bool(ref["empty"]),
                          n_pt_removed=int(ref["pt_removed"].sum()), n_ls_removed=int(ref["ls_removed"].sum()))
    for kind in ("points", "lines"):
        assert np.array_equal(after[kind + ".valid"], m_after[kind]["valid"]), kind
        assert np.array_equal(after[kind + ".feat_idx"], m_after[kind]["feat_idx"]), kind
    return ref


@pytest.mark.parametrize("name", sorted(CS.CASES))
def test_cases_equal_the_restatement(ctx, name):
    m, p = CS.CASES[name]()
    ref = _check(m, p, *_run_device(ctx, m, p))
    if name.startswith("exact_"):                      # n list entries and n observations of each kind, as the name says
        n = int(name.split("_")[1])
        assert len(ref["pt_list"]) == len(ref["ls_list"]) == len(ref["pt_obs"]) == len(ref["ls_obs"]) == n
    if name == "no_observations":
        assert ref["empty"]


def test_form_twice_and_a_smaller_map_after_a_larger_one(ctx):
    """one handle across keyframes: the second form clears what the first one set, and a smaller map reuses the buffers"""
    big, pb = CS.CASES["mixed_805"]()
    small, ps = CS.CASES["overload_kf"]()
    lm = LM.LocalMap(ctx)
    for m, p in ((big, pb), (small, ps), (small, dict(ps, anchor=29, window=0))):
        ix = LM.DeviceMapIndex(m, ctx.device)
        lm.form(ix, p["anchor"], m["row"], p["min_cov"], p["window"])
        ref, _ = CS.run_ref(m, p)
        got = lm.download("kf_local", "pt_local", "ls_local")
        for k in got:
            assert np.array_equal(got[k], ref[k]), k
    lm.close()


def test_a_hundred_thousand_landmarks(ctx):
    """the many-tile path: 313 + 79 tiles chain their counts"""
    m = LM.synthetic_map(n_kf=120, n_pt=80_000, n_ls=20_000, seed=31, max_obs=4, null_kf=(40, 117))
    p = dict(anchor=119, min_cov=120, window=6, kf2=119, max_kf_idx=125, min_lm_obs=3)
    ref = _check(m, p, *_run_device(ctx, m, p))
    assert 256 * 8 < len(ref["pt_list"]) < 70_000 and len(ref["pt_obs"]) > 256 * 8 and ref["pt_removed"].sum() > 100


def test_candidates_feed_the_map2kf_driver(ctx):
    """pt_candidate goes into plslam_map2kf_match_points_dev where it lies: the table the host-computed mask gives"""
    import torch
    import plslam_amd
    from test_map2kf import fast_cfg, scene
    s = scene(3000, 700, seed=5)
    m = LM.synthetic_map(n_kf=25, n_pt=3000, n_ls=10, seed=41)
    m["points"]["X"] = np.ascontiguousarray(s["LM"], np.float64)
    p = dict(anchor=24, min_cov=60, window=4, kf2=24)
    ix = LM.DeviceMapIndex(m, ctx.device)
    lm = LM.LocalMap(ctx)
    lm.form(ix, p["anchor"], m["row"], p["min_cov"], p["window"])
    lm.candidates(ix, p["kf2"])
    ref, _ = CS.run_ref(m, dict(p, max_kf_idx=0, min_lm_obs=0))
    assert 300 < ref["pt_candidate"].sum() < 2900
    cam = plslam_amd.make_cam(**synth.EUROC)
    d_md = torch.from_numpy(s["med"]).to(torch.device("cuda", ctx.device))
    d_ref = torch.from_numpy(ref["pt_candidate"]).to(torch.device("cuda", ctx.device))
    tail = (3000, s["kf_desc"], s["kf_feat"], s["kf_idx"], 0.9, True, 1.5, 10, fast_cfg())
    got = ctx.map2kf_match_dev("points", cam, s["Twf"], ix.ptr("points.X"), d_md.data_ptr(), lm.device_buffers()["pt_candidate"], *tail)
    want = ctx.map2kf_match_dev("points", cam, s["Twf"], ix.ptr("points.X"), d_md.data_ptr(), d_ref.data_ptr(), *tail)
    assert want[1] > 20 and got[1] == want[1] and got[2] == want[2]
    np.testing.assert_array_equal(got[0], want[0])
    assert (got[0][ref["pt_candidate"] == 0] == -1).all()
    lm.close()


def test_gather_feeds_the_lba_plan(ctx):
    """the gathered columns go into plslam_lba_plan_create as they come: one iterate equals the plan built from the restatement's
    lists (n_pose_slots = n_map_kf: the pose slot is the keyframe index)"""
    import plslam_amd
    m, p = CS.mixed(700)
    rng = np.random.Generator(np.random.PCG64(3))
    P, L = m["points"], m["lines"]
    P["X"][:] = rng.uniform(-3, 3, P["X"].shape) + [0, 0, 12]
    L["X"][:] = rng.uniform(-3, 3, L["X"].shape) + [0, 0, 12, 0, 0, 12]
    ix = LM.DeviceMapIndex(m, ctx.device)
    lm = LM.LocalMap(ctx)
    lm.form(ix, p["anchor"], m["row"], p["min_cov"], p["window"])
    c = lm.gather(ix)
    g = lm.download()
    ref, _ = CS.run_ref(m, p)
    assert c["nkf"] > 2 and c["n_pt_obs"] > 500 and c["n_ls_obs"] > 100 and (ref["pt_kf_loc"] == -1).any() and (ref["pt_kf_loc"] >= 0).any()
    cam = plslam_amd.make_cam(**synth.EUROC)
    T = np.stack([synth.se3_exp(0.05 * rng.standard_normal(6)) for _ in range(m["n_map_kf"])])
    res = []
    for o in (g, ref):
        plan = plslam_amd.LbaPlan(ctx, cam, 1e-7, m["n_map_kf"], len(o["kf_list"]), len(o["pt_list"]), len(o["ls_list"]), o["pt_lm_loc"],
                                  o["pt_pose_slot"], o["pt_kf_loc"], o["pt_obs_uv"], o["ls_lm_loc"], o["ls_pose_slot"], o["ls_kf_loc"],
                                  o["ls_l_obs"])
        x = o["X_aux"][6 * len(o["kf_list"]):]
        res.append(plan.iterate(T, x[:3 * len(o["pt_list"])], x[3 * len(o["pt_list"]):]))
        plan.close()
    assert np.isfinite(res[1]["err"]) and res[1]["err"] > 0
    for k in res[0]:
        np.testing.assert_array_equal(res[0][k], res[1][k], err_msg=k)
    lm.close()
