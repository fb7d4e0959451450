"""The local BA's Schur step on the device (plslam_lba_plan_diag_max / _schur / _backsub / _apply_step / _iterate_schur; K19-K24 of
lba_schur.hip) against the sequential restatement of tests/lba_schur_ref.py -- as 64-bit WORDS.  The step is a fixed-order float64
computation without contraction: every S, b, step, updated landmark and sum of squares must be the restatement's bits, on the
cases of tests/lba_schur_cases.py (blocks without rank, exact zeros on a diagonal, lists on their chunk and workgroup edges) and
the lambdas its table keeps.  tests/test_lba_schur_cases_cpu.py ties the restatement to long-double values.  There is no
tolerance in this file.  The blocks are the device's own (plan.iterate_dev + plan.blocks()); the lists are shown equal to the
Python mirror the CPU test uses."""
import numpy as np
import pytest

import lba_schur_cases as CS
import lba_schur_ref as R
import plslam_amd
from plslam_amd import synth
from plslam_amd.capi import EINVAL, LbaPlan, PlslamError

pytestmark = pytest.mark.gpu
NAMES = list(CS.CASES)
_BLOCKS = ("g", "H_pose", "H_pt", "H_ls", "W_pt", "W_ls")
_LISTS = ("pt_ptr", "pt_ids", "ls_ptr", "ls_ids", "kf_ptr", "kf_ids", "pt_lm_loc", "pt_kf_loc", "ls_lm_loc", "ls_kf_loc", "blk_ptr", "pairs")


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


def _same(a, b, what=""):
    a, b = np.asarray(a), np.asarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape, (what, a.dtype, b.dtype, a.shape, b.shape)
    if not np.array_equal(_bits(a), _bits(b)):
        bad = np.flatnonzero(_bits(a).reshape(-1) != _bits(b).reshape(-1))
        i = int(bad[0])
        raise AssertionError(f"{what}: {bad.size} of {a.size} words differ, first at {i}: {a.reshape(-1)[i]!r} != {b.reshape(-1)[i]!r}")


def _cam():
    return plslam_amd.make_cam(**synth.EUROC)


def _plan(ctx, c):
    return LbaPlan(ctx, _cam(), CS.HOMOG_TH, *CS.plan_args(c))


def _first(plan, c):
    """the first iteration, state uploaded -> err"""
    return plan.iterate_dev(c["T"], c["X"], c["L"], want_g=False)[0]


_EXPECT = {}


def _expect(ctx, name):
    """the device's blocks and lists of a case (once per session) and, per lambda of its table, the restatement on them:
    (B, lists, err, {lam: dict(R = restate(...), dp, dxp, dxl, ss, t_pt, t_ls)})"""
    if name not in _EXPECT:
        c = CS.case(name)
        plan = _plan(ctx, c)
        err = _first(plan, c)
        B, Ls = plan.blocks(), plan.lists(prepare_schur=True)
        plan.close()
        assert all(np.isfinite(B[k]).all() for k in _BLOCKS) and np.isfinite(err)
        per = {}
        for lam in CS.lambdas(name):
            Rr = R.restate(B, Ls, lam)
            dp = np.linalg.solve(Rr["S"], Rr["b"])
            dxp, dxl, ss = R.restate_backsub(B, Ls, Rr, dp)
            t_pt, t_ls, _ = R.restate_backsub(B, Ls, Rr, np.zeros_like(dp))
            per[lam] = dict(R=Rr, dp=dp, dxp=dxp, dxl=dxl, ss=np.float64(ss), t_pt=t_pt, t_ls=t_ls)
        _EXPECT[name] = (B, Ls, np.float64(err), per)
    return _EXPECT[name]


def _check_step(plan, c, E, what):
    """schur's outputs are checked by the caller; here: backsub(0), backsub(dp), the sum of squares and the update in place"""
    t_pt, t_ls = plan.backsub(np.zeros_like(E["dp"]))
    _same(t_pt, E["t_pt"], what + " backsub(0) points")
    _same(t_ls, E["t_ls"], what + " backsub(0) lines")
    _same(t_pt, E["R"]["tp"], what + " backsub(0) = t, points")
    _same(t_ls, E["R"]["tl"], what + " backsub(0) = t, lines")
    dxp, dxl = plan.backsub(E["dp"])
    _same(dxp, E["dxp"], what + " dX points")
    _same(dxl, E["dxl"], what + " dX lines")
    _same(np.float64(plan.apply_step(E["dp"], None, apply=False)), E["ss"], what + " sum of squares")
    plan.backsub(E["dp"], apply=True, want=False)
    X, L = plan.get_landmarks()
    _same(X, c["X"] + E["dxp"], what + " X += d")
    _same(L, c["L"] + E["dxl"], what + " L += d")


def _check_system(got, E, what):
    S, b, ns = got
    _same(S, E["R"]["S"], what + " S")
    _same(b, E["R"]["b"], what + " b")
    assert ns == E["R"]["n_singular"], (what, ns, E["R"]["n_singular"])


@pytest.mark.parametrize("name", NAMES)
def test_the_step_equals_the_restatement_word_for_word(ctx, name):
    c = CS.case(name)
    B, Ls, err, per = _expect(ctx, name)
    # the lists the restatement walked are the mirror's, which the CPU test walks
    mirror = R.build_lists(c)
    for k in _LISTS:
        _same(Ls[k], mirror[k], f"{name}: {k}")
    assert (Ls["max_chunks"], Ls["schur_chunks"]) == (mirror["max_chunks"], mirror["schur_chunks"])
    plan = _plan(ctx, c)
    _same(np.float64(_first(plan, c)), err, "err")
    _same(np.float64(plan.diag_max()), np.float64(next(iter(per.values()))["R"]["diag_max"]), "diag_max")
    for lam, E in per.items():
        what = f"{name} lambda {lam:g}:"
        _check_system(plan.schur(lam), E, what)
        _same(np.linalg.solve(*plan.schur(lam)[:2]), E["dp"], what + " dp")          # (the host's solve of the same words)
        _check_step(plan, c, E, what)
        Rr = E["R"]
        if name == "on_the_axis":
            assert Rr["n_singular"] == 4 and Rr["sing_pt"][:3].all() and Rr["sing_ls"][0]
            for a in (E["t_pt"][:3], E["t_ls"][:1], E["dxp"][:3], E["dxl"][:1], Rr["Vp"][:3], Rr["Vl"][:1]):
                assert not _bits(a).any()                                            # +0.0, every word
        if name == "strangers":
            assert not _bits(Rr["S"][0:6, 6:12]).any() and not _bits(Rr["S"][6:12, 0:6]).any()
        _same(np.float64(_first(plan, c)), err, what + " err again")                  # the state back to the case's
    after = plan.blocks()
    for k in _BLOCKS:
        _same(after[k], B[k], f"{name}: {k} after the steps")
    plan.close()


@pytest.mark.parametrize("name", NAMES)
def test_the_fused_calls_give_the_same_words(ctx, name):
    """plslam_lba_plan_iterate_schur (the landmark inverses computed in the blocks' launch, K10 riding in the partials' launch)
    and plslam_lba_plan_apply_step against the same restatement"""
    c = CS.case(name)
    B, Ls, err, per = _expect(ctx, name)
    plan = _plan(ctx, c)
    _first(plan, c)
    for lam, E in per.items():
        what = f"{name} fused, lambda {lam:g}:"
        e, S, b, ns = plan.iterate_schur(lam, 0)
        _same(np.float64(e), err, what + " err")
        _check_system((S, b, ns), E, what)
        _same(np.float64(plan.apply_step(E["dp"], None, apply=True)), E["ss"], what + " sum of squares")
        X, L = plan.get_landmarks()
        _same(X, c["X"] + E["dxp"], what + " X += d")
        _same(L, c["L"] + E["dxl"], what + " L += d")
        with pytest.raises(PlslamError):
            plan.apply_step(E["dp"], None, apply=True)                                # applied: a new Schur step is needed
        _first(plan, c)
    after = plan.blocks()
    for k in _BLOCKS:
        _same(after[k], B[k], f"{name}: {k}")
    plan.close()


@pytest.mark.parametrize("name", NAMES)
def test_a_plan_built_on_the_device_gives_the_same_words(ctx, name):
    """LbaPlan.from_device from the same columns: the lists built on the device, the landmarks copied in at creation"""
    import torch
    c = CS.case(name)
    B, Ls, err, per = _expect(ctx, name)
    dev = torch.device("cuda", ctx.device)
    keep = {k: torch.from_numpy(np.ascontiguousarray(c[k]).copy() if np.asarray(c[k]).size else np.zeros(1, np.asarray(c[k]).dtype)).to(dev)
            for k in CS.PLAN_COLUMNS + ("X", "L")}
    torch.cuda.synchronize()
    p = lambda k: keep[k].data_ptr() if np.asarray(c[k]).size else 0                  # noqa: E731
    plan = LbaPlan.from_device(ctx, _cam(), CS.HOMOG_TH, c["n_pose_slots"], c["nkf"], c["npt"], c["nls"], p("pt_lm"), p("pt_slot"),
                               p("pt_kf_loc"), p("pt_obs_uv"), c["pt_lm"].size, p("ls_lm"), p("ls_slot"), p("ls_kf_loc"), p("ls_l_obs"),
                               c["ls_lm"].size, p("X"), p("L"))
    got = plan.lists(prepare_schur=True)
    for k in _LISTS:
        _same(got[k], Ls[k], f"{name}: {k}")
    plan.set_poses(c["T"])
    _same(np.float64(plan.iterate_resident()), err, "err")
    blocks = plan.blocks()
    for k in _BLOCKS:
        _same(blocks[k], B[k], f"{name}: {k}")
    for lam, E in per.items():
        what = f"{name} from_device, lambda {lam:g}:"
        _check_system(plan.schur(lam), E, what)
        _check_step(plan, c, E, what)
        plan.iterate_dev(c["T"], c["X"], c["L"], want_g=False)
    plan.close()


@pytest.mark.parametrize("name", NAMES)
def test_three_calls_in_a_row_give_the_same_words(ctx, name):
    """the two counters of singular landmarks take turns and every call clears the other one: each call counts afresh; a block
    without pairs stays +0.0; nothing of an earlier call (a partial, a counter, a step) shows in a later one -- across lambdas,
    separate and fused calls mixed"""
    c = CS.case(name)
    B, Ls, err, per = _expect(ctx, name)
    plan = _plan(ctx, c)
    _first(plan, c)
    lams = list(per)
    for rep in range(3):
        for lam in lams if rep != 1 else lams[::-1]:
            E = per[lam]
            what = f"{name} call {rep}, lambda {lam:g}:"
            got = plan.schur(lam) if rep != 2 else plan.iterate_schur(lam, 0)[1:]
            _check_system(got, E, what)
            if name == "on_the_axis":
                assert got[2] == 4
            if name == "strangers":
                assert not _bits(got[0][0:6, 6:12]).any() and not _bits(got[0][6:12, 0:6]).any()
            dxp, dxl = plan.backsub(E["dp"])
            _same(dxp, E["dxp"], what + " dX points")
            _same(dxl, E["dxl"], what + " dX lines")
    plan.close()


def test_a_negative_lambda_is_refused_and_the_plan_still_works(ctx):
    name = "two_views"
    c = CS.case(name)
    B, Ls, err, per = _expect(ctx, name)
    plan = _plan(ctx, c)
    _first(plan, c)
    lam, E = next(iter(per.items()))
    _check_system(plan.schur(lam), E, "before")
    for bad in (-1e-3, -np.inf, np.nan, -5e-324):
        with pytest.raises(PlslamError) as e:
            plan.schur(bad)
        assert e.value.code == EINVAL, bad
        with pytest.raises(PlslamError) as e:
            plan.iterate_schur(bad, 0)
        assert e.value.code == EINVAL, bad
    _check_system(plan.schur(lam), E, "after the refusals")
    _check_step(plan, c, E, "after the refusals")
    _first(plan, c)
    _check_system(plan.iterate_schur(lam, 0)[1:], E, "fused, after the refusals")
    plan.close()
