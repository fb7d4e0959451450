"""The cases of tests/map_gate_cases.py (the visibility pre-filter and the map<->keyframe gates ON their thresholds; what they
hold is checked without a device by tests/test_map_gate_cases_cpu.py) through every way that arithmetic runs on the device,
bit for bit against the oracle: masks, counts, association tables, match counts, the fall-back flag.

  lone calls        map_point_visible / map_line_visible (k_visible, no flags), map2kf_point_gate / map2kf_line_gate (K5 / K6
                    with the row count as an argument, the count by one atomic per wave)
  map2kf_match      host pointers, brute force, ONE synchronisation: k_visible_compact (flags folded in, the list by look-back,
                    the table's -1 fill), k_prepare_rows, the scan's plan with the row count on the device, K5 / K6 with
                    nq_dev, the association written from the gate, the counters published from the last workgroup
  map2kf_match_fast fast matching on (k_visible_compact, k_prepare_rows with the window centres, the windowed matcher, K5 / K6
                    as above; the brute-force scan behind it when it finds too little) and off (the road above)
                    (the window-centre classes cell_boundary and line_in_one_cell run with a window of the cell itself:
                    a centre one cell off misses its feature)
  map2kf_match_dev  the map resident on the device: the one-synchronisation forms as above, and -- under a context option the
                    scan's plan refuses -- the step-by-step form: k_visible WITH device flags, the list built on the host, row
                    gathers, the scan, K5 / K6 with the row count as an argument, the association on the host

On the driver routes the match table comes from the descriptor scan: map_gate_cases.descriptors makes it return the class's
m12 (asserted on the CPU against the restatement; here the oracle's driver is the reference)."""
import numpy as np
import pytest

import plslam_amd

import map_gate_cases as M

pytestmark = pytest.mark.gpu
KINDS_CLASSES = M.classes()
NNR, MM = 0.75, M.MIN_MATCHES


def _ids(kc):
    return f"{kc[0]}-{kc[1]}"


@pytest.fixture(scope="module")
def cams(oracle):
    return plslam_amd.make_cam(**M.K), oracle.make_cam(**M.K)


_EXPECTED = {}


def _expected(c, oracle, ocam):
    """The oracle's results of one case, computed once and shared by the tests."""
    if c.name not in _EXPECTED:
        pts = c.kind == "points"
        e = dict(vis=(oracle.map_point_visible if pts else oracle.map_line_visible)(ocam, c.Twf, c.LM),
                 gate=(oracle.map2kf_point_gate if pts else oracle.map2kf_line_gate)(ocam, c.Twf, c.LM, c.m12, c.feat, c.th))
        if c.driver:
            a = M.driver_args(c)
            e["bf"] = oracle.map2kf_match(c.kind, ocam, *a, NNR, True, c.th, MM)
            e["fast"] = oracle.map2kf_match_fast(c.kind, ocam, *a, NNR, True, c.th, MM, M.fast_cfg(ws=M.window_of(c)), kf_seg=c.seg)
            # ... and with min_matches just under the list's length: the windowed matcher finds too little, the scan runs behind it
            e["mm_fb"] = max(len(M.restate_driver(c)[2]) - 1, 1)
            e["fast_fb"] = oracle.map2kf_match_fast(c.kind, ocam, *a, NNR, True, c.th, e["mm_fb"], M.fast_cfg(ws=M.window_of(c)), kf_seg=c.seg)
            e["off"] = oracle.map2kf_match_fast(c.kind, ocam, *a, NNR, True, c.th, MM, M.fast_cfg(enabled=0), kf_seg=c.seg)
        _EXPECTED[c.name] = e
    return _EXPECTED[c.name]


@pytest.mark.parametrize("kc", [kc for kc in KINDS_CLASSES if kc[1] not in M.DRIVER_ONLY], ids=_ids)
def test_lone_visibility_and_gate_calls(ctx, oracle, cams, kc):
    cam, ocam = cams
    pts = kc[0] == "points"
    for c in M.cases_of(*kc):
        e = _expected(c, oracle, ocam)
        vis = (ctx.map_point_visible if pts else ctx.map_line_visible)(cam, c.Twf, c.LM)
        assert np.array_equal(vis, e["vis"]), c.name
        mask, cnt = (ctx.map2kf_point_gate if pts else ctx.map2kf_line_gate)(cam, c.Twf, c.LM, c.m12, c.feat, c.th)
        assert np.array_equal(mask, e["gate"][0]) and cnt == e["gate"][1] == int(mask.sum()), c.name


def _same(got, ref, name, used=True):
    np.testing.assert_array_equal(got[0], ref[0], err_msg=name)
    assert got[1] == ref[1], name
    if used:
        assert got[2] == ref[2], name


@pytest.mark.parametrize("kc", [kc for kc in KINDS_CLASSES if kc[1] not in M.NO_DRIVER], ids=_ids)
def test_host_pointer_drivers(ctx, oracle, cams, kc):
    """map2kf_match, map2kf_match_fast with fast matching on and off."""
    cam, ocam = cams
    seen = set()
    for c in M.cases_of(*kc):
        e = _expected(c, oracle, ocam)
        a = M.driver_args(c)
        _same(ctx.map2kf_match(c.kind, cam, *a, NNR, True, c.th, MM), e["bf"], c.name + " map2kf_match", used=False)
        assert e["bf"][1] == int((e["bf"][0] >= 0).sum())
        _same(ctx.map2kf_match_fast(c.kind, cam, *a, NNR, True, c.th, MM, M.fast_cfg(ws=M.window_of(c)), kf_seg=c.seg), e["fast"], c.name + " fast on")
        _same(ctx.map2kf_match_fast(c.kind, cam, *a, NNR, True, c.th, e["mm_fb"], M.fast_cfg(ws=M.window_of(c)), kf_seg=c.seg), e["fast_fb"], c.name + " fast, fall-back")
        _same(ctx.map2kf_match_fast(c.kind, cam, *a, NNR, True, c.th, MM, M.fast_cfg(enabled=0), kf_seg=c.seg), e["off"], c.name + " fast off")
        seen.add(e["fast_fb"][2])
    assert seen == {0, 1} or kc[1] == "compaction_shapes", seen


@pytest.mark.parametrize("kc", [kc for kc in KINDS_CLASSES if kc[1] not in M.NO_DRIVER], ids=_ids)
def test_device_resident_drivers_in_both_forms(ctx, oracle, cams, kc):
    """map2kf_match_dev: the one-synchronisation forms (k_visible_compact, the device row count, the published counters), and
    the step-by-step form (k_visible with device flags) that a context option the scan's plan refuses selects."""
    import torch
    cam, ocam = cams
    dev = torch.device("cuda", ctx.device)
    for c in M.cases_of(*kc):
        e = _expected(c, oracle, ocam)
        Twf, LM, med, cand, kfd, feat, kf_idx = M.driver_args(c)
        d = [torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in (LM, med, cand)]

        def call(fm, mm=MM):
            return ctx.map2kf_match_dev(c.kind, cam, Twf, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), c.n, kfd, feat, kf_idx,
                                        NNR, True, c.th, mm, fm, kf_seg=c.seg)
        _same(call(M.fast_cfg(ws=M.window_of(c))), e["fast"], c.name + " dev fast on")
        _same(call(M.fast_cfg(ws=M.window_of(c)), e["mm_fb"]), e["fast_fb"], c.name + " dev fast, fall-back")
        _same(call(M.fast_cfg(enabled=0)), e["off"], c.name + " dev one synchronisation")
        try:
            ctx.set_option("col_split", 1)
            _same(call(M.fast_cfg(enabled=0)), e["off"], c.name + " dev step by step")
        finally:
            ctx.set_option("col_split", 0)
        assert np.array_equal(d[2].cpu().numpy(), cand) and np.array_equal(d[0].cpu().numpy().view(np.uint64), LM.view(np.uint64))
