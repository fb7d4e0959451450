"""The branches of the map<->keyframe drivers' launch sequences (plslam_amd/csrc/map2kf.hip) that tests/test_map2kf.py does not
reach: a map of exactly one workgroup of k_visible_compact (256 landmarks) and of one landmark more (the second workgroup holds a
single landmark, a visible candidate, whose list slot comes from the first workgroup's count), and the two early returns of the
step-by-step form.  Bit-exact against the oracle through the host-pointer and the device-resident entry points."""
import numpy as np
import pytest

from plslam_amd import synth
from test_map2kf import fast_cfg, scene


@pytest.mark.gpu
@pytest.mark.parametrize("n_map", [256, 257])
@pytest.mark.parametrize("kind", ["points", "lines"])
def test_gpu_drivers_at_the_workgroup_boundary_of_the_candidate_list(ctx, oracle, kind, n_map):
    import torch
    import plslam_amd
    cam, ocam = plslam_amd.make_cam(**synth.EUROC), oracle.make_cam(**synth.EUROC)
    s = scene(n_map, 40, lines=(kind == "lines"), seed=900 + n_map, frac_unmatched=0.9)
    # the last landmark: a candidate that projects inside the image (the place of one that does, a descriptor of its own)
    visible = oracle.map_line_visible if kind == "lines" else oracle.map_point_visible
    j = int(np.flatnonzero(visible(ocam, s["Twf"], s["LM"])[:-1])[0])
    s["LM"][-1], s["cand"][-1] = s["LM"][j], 1
    vis = visible(ocam, s["Twf"], s["LM"]).astype(bool) & s["cand"].astype(bool)
    assert vis[-1] and 30 < vis[:256].sum() < 256              # both workgroups of the 257-landmark map list something
    a = (s["Twf"], s["LM"], s["med"], s["cand"], s["kf_desc"], s["kf_feat"], s["kf_idx"])
    dev = torch.device("cuda", ctx.device)
    d = [torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in (s["LM"], s["med"], s["cand"])]
    seen = set()
    for mm, fm in ((2, fast_cfg()), (2, fast_cfg(enabled=0)), (30, fast_cfg())):
        ref = oracle.map2kf_match_fast(kind, ocam, *a, 0.9, True, 2.0, mm, fm, kf_seg=s.get("kf_seg"))
        got = ctx.map2kf_match_fast(kind, cam, *a, 0.9, True, 2.0, mm, fm, kf_seg=s.get("kf_seg"))
        gotd = ctx.map2kf_match_dev(kind, cam, s["Twf"], d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), n_map, s["kf_desc"],
                                    s["kf_feat"], s["kf_idx"], 0.9, True, 2.0, mm, fm, kf_seg=s.get("kf_seg"))
        for g in (got, gotd):
            np.testing.assert_array_equal(g[0], ref[0])
            assert g[1] == ref[1] and g[2] == ref[2]
        seen.add((bool(fm["enabled"]), ref[2]))
    # matchGrid alone, StVO::match alone, and StVO::match behind a matchGrid that found fewer than min_matches
    assert seen == {(True, 0), (False, 1), (True, 1)}


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["points", "lines"])
def test_gpu_step_by_step_form_returns_early(ctx, oracle, kind):
    """The step-by-step form (here: a brute-force problem that is not mutual) with nothing to do after its visibility pass: no
    visible candidate -- it returns before anything is gathered --, and a candidate list not longer than min_matches -- no
    matcher runs, no gate.  Every entry stays -1; host-pointer and device-resident entry points."""
    import torch
    import plslam_amd
    cam, ocam = plslam_amd.make_cam(**synth.EUROC), oracle.make_cam(**synth.EUROC)
    s = scene(300, 40, lines=(kind == "lines"), seed=950)
    dev = torch.device("cuda", ctx.device)
    off = fast_cfg(enabled=0)
    for cand, mm in ((np.zeros_like(s["cand"]), 2), (s["cand"], 300)):
        a = (s["Twf"], s["LM"], s["med"], cand, s["kf_desc"], s["kf_feat"], s["kf_idx"])
        ref = oracle.map2kf_match(kind, ocam, *a, 0.9, False, 2.0, mm)
        assert ref[1] == 0 and (ref[0] == -1).all()
        got = ctx.map2kf_match(kind, cam, *a, 0.9, False, 2.0, mm)
        d = [torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in (s["LM"], s["med"], cand)]
        gotd = ctx.map2kf_match_dev(kind, cam, s["Twf"], d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), 300, s["kf_desc"],
                                    s["kf_feat"], s["kf_idx"], 0.9, False, 2.0, mm, off, kf_seg=s.get("kf_seg"))
        for g in (got, gotd):
            np.testing.assert_array_equal(g[0], ref[0])
            assert g[1] == 0
