"""The stereo gates ON their thresholds, on the device: every case of tests/stereo_gate_cases.py (what each one reaches, and that
wrong gates would be told apart, is tests/test_stereo_gate_cases_cpu.py's business) through every way
plslam_amd/csrc/stereo_gates_dev.hpp runs, bit for bit against the oracle -- table, disparities as raw 64-bit words, count.

  host        plslam_stereo_point_gate / _line_gate (k_stereo_point_gate / k_stereo_line_gate)
  dev         the _dev calls on a side stream, with a counter and with n_stereo = NULL
  finalize    the gate stage of a match plan inside k_finalize.  Known from: option "post_fuse" 1 and key_state() without
              KEYS_COLUMNS_NOT_IN_MEMORY (no k_post_fused); set_wire16 accepted (the plan is neither fused nor column-split, so
              its tables are written by k_finalize); each gate's matches_12 / n_l are a problem's, which is what
              plslam_match_plan_add_stereo_gates tests before it hands a gate to the finalize kernel
  post_fused  inside k_post_fused ("post_fuse" 2 on a matrix-core plan).  Known from: key_state() & KEYS_COLUMNS_NOT_IN_MEMORY
  batched     k_stereo_gates_batched, the two plan forms that launch it: (external) gates over tables that are NOT the plan's --
              the plan's own problem is an unrelated 8 x 8 one, so no other kernel ever reads those tables; (fused) a plan with
              option "fuse" 2, which has no finalize kernel: known from set_wire16 answering ENOTSUP with "col_split" 1

In the plan paths a scan makes the table from descriptors built so that it is the case's m12 (asserted on the device result
and, on the CPU, against oracle.match).  The index-edge classes cannot come out of a scan: they run through host, dev and the
external form of the batched kernel.  n_l = 1 cannot be matched by a mutual scan (no second row on the column side): it runs
through k_finalize as a non-mutual problem and through host, dev and batched-external, not through k_post_fused or a fused plan
(both take mutual problems only here).  A gate record carries its own thresholds, so one plan holds every threshold record of
a class."""
import ctypes as C_
import functools
import os

import numpy as np
import pytest

import stereo_gate_cases as C

pytestmark = pytest.mark.gpu
CLASSES = C.classes()
SCANNED = [k for k in CLASSES if k[1] != "index_edges"]
KEYS_COLUMNS_NOT_IN_MEMORY = 4                                          # plslam_match_plan_key_state (include/plslam_hip.h)
_ids = lambda ks: [f"{k}-{c}" for k, c in ks]      # noqa: E731


@functools.lru_cache(maxsize=None)
def _ref(name):
    from oracle import oracle as O
    c = next(x for x in C.all_cases() if x.name == name)
    with np.errstate(all="ignore"):
        return (O.stereo_point_gate if c.kind == "points" else O.stereo_line_gate)(*C.case_args(c))


def _bits(d):
    return np.ascontiguousarray(d, np.float64).reshape(-1).view(np.uint64)


def _same(name, got, want, count=True):
    np.testing.assert_array_equal(np.asarray(got[0]), want[0], err_msg=name)
    np.testing.assert_array_equal(_bits(got[1]), _bits(want[1]), err_msg=name)
    if count:
        assert int(got[2]) == want[2] == int((want[0] >= 0).sum()), name


def _thresholds(c):
    if c.kind == "points":
        return dict(max_dist_epip=c.th[0], min_disp=c.th[1])
    return dict(min_disp=c.th[0], line_horiz_th=c.th[1], stereo_overlap_th=c.th[2], ls_min_disp_ratio=c.th[3])


def _p(a):
    return a.ctypes.data_as(C_.c_void_p) if a.size else None           # an empty right table is passed as NULL


def _host(ctx, c):
    n_l, lines = c.n_l, c.kind == "lines"
    out, disp, n = np.full(n_l, -7, np.int32), np.full((n_l, 2) if lines else n_l, -7.0), C_.c_int32(-7)
    fn = ctx._L.plslam_stereo_line_gate if lines else ctx._L.plslam_stereo_point_gate
    assert fn(ctx.handle, _p(c.m12), n_l, _p(c.f_l), _p(c.f_r), c.f_r.shape[0], *c.th, _p(out), _p(disp), C_.byref(n)) == 0, c.name
    return out, disp, n.value


class _Dev:
    """A case's tables on the device, outputs pre-filled with values no gate writes."""

    def __init__(self, ctx, c, table=None):
        import torch
        dev = torch.device("cuda", ctx.device)
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)         # noqa: E731
        self.c, self.lines = c, c.kind == "lines"
        self.m = t(c.m12) if table is None else table
        self.a = t(c.f_l)
        self.b = t(c.f_r) if c.f_r.size else None
        self.out = torch.full((c.n_l,), -7, dtype=torch.int32, device=dev)
        self.disp = torch.full((c.n_l * (2 if self.lines else 1),), -7.0, dtype=torch.float64, device=dev)

    def refill(self):
        self.out.fill_(-7)
        self.disp.fill_(-7.0)

    def gate(self, n_stereo):
        return dict(matches_12=self.m.data_ptr(), f_l=self.a.data_ptr(), f_r=self.b.data_ptr() if self.b is not None else 0,
                    n_l=self.c.n_l, n_r=self.c.f_r.shape[0], lines=int(self.lines), stereo_12=self.out.data_ptr(),
                    disp=self.disp.data_ptr(), n_stereo=n_stereo, **_thresholds(self.c))

    def result(self, n=None):
        return self.out.cpu().numpy(), self.disp.cpu().numpy(), n


def _dev_call(ctx, d, cnt_ptr, stream):
    g = d.gate(cnt_ptr)
    fn = ctx._L.plslam_stereo_line_gate_dev if d.lines else ctx._L.plslam_stereo_point_gate_dev
    return fn(ctx.handle, g["matches_12"], g["n_l"], g["f_l"], g["f_r"] or None, g["n_r"], *d.c.th, g["stereo_12"], g["disp"],
              cnt_ptr or None, stream)


@pytest.mark.parametrize("kind,cls", CLASSES, ids=_ids(CLASSES))
def test_host_pointer_calls(ctx, oracle, kind, cls):
    for c in C.cases_of(kind, cls):
        _same(c.name, _host(ctx, c), _ref(c.name))


@pytest.mark.parametrize("kind,cls", CLASSES, ids=_ids(CLASSES))
def test_dev_calls_on_a_side_stream_with_and_without_a_counter(ctx, oracle, kind, cls):
    import torch
    dev = torch.device("cuda", ctx.device)
    st = torch.cuda.Stream(device=dev)
    cases = C.cases_of(kind, cls)
    ds = [_Dev(ctx, c) for c in cases]
    cnt = torch.full((len(cases),), 77, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    for i, d in enumerate(ds):
        assert _dev_call(ctx, d, cnt.data_ptr() + 4 * i, st.cuda_stream) == 0, d.c.name
    st.synchronize()
    counts = cnt.cpu().numpy()
    for i, d in enumerate(ds):
        _same(d.c.name, d.result(counts[i]), _ref(d.c.name))
        d.refill()
    torch.cuda.synchronize()
    for d in ds:                                                     # n_stereo = NULL: succeeds, tables right, counters untouched
        assert _dev_call(ctx, d, 0, st.cuda_stream) == 0, d.c.name
    st.synchronize()
    for d in ds:
        _same(d.c.name, d.result(), _ref(d.c.name), count=False)
    assert np.array_equal(cnt.cpu().numpy(), counts)


def _scan_tables(ctx, cases):
    """Per case: descriptors on the device, a match table of -2 and the problem tuple of Context.plan()."""
    import torch
    from oracle import oracle as O
    dev = torch.device("cuda", ctx.device)
    keep, probs, ds = [], [], []
    mcnt = torch.zeros(len(cases), dtype=torch.int32, device=dev)
    for i, c in enumerate(cases):
        d_l, d_r = C.descriptors(c)
        m, _ = O.match(d_l, d_r, 0.75, C.scan_mutual(c))
        assert np.array_equal(m, c.m12), c.name                       # the scan's table IS the case's (CPU)
        tl, tr = torch.from_numpy(d_l).to(dev), torch.from_numpy(d_r).to(dev)
        table = torch.full((c.n_l,), -2, dtype=torch.int32, device=dev)
        keep += [tl, tr]
        probs.append((tl.data_ptr(), c.n_l, tr.data_ptr(), d_r.shape[0], 0.75, C.scan_mutual(c), table.data_ptr(), mcnt.data_ptr() + 4 * i))
        ds.append(_Dev(ctx, c, table=table))
    return keep, probs, ds, mcnt


def _run_and_compare(ctx, plan, ds, cnt, scanned):
    import torch
    st = torch.cuda.Stream(device=torch.device("cuda", ctx.device))
    for rerun in range(2):                                            # (the second run of a small plan replays its graph)
        for d in ds:
            d.refill()
        cnt.fill_(77)
        torch.cuda.synchronize()
        plan.run(st.cuda_stream)
        st.synchronize()
        counts = cnt.cpu().numpy()
        for i, d in enumerate(ds):
            if scanned:
                np.testing.assert_array_equal(d.m.cpu().numpy(), d.c.m12, err_msg=d.c.name)     # the scan's table IS the case's
            _same(d.c.name, d.result(counts[i]), _ref(d.c.name))


def _options(ctx, **kv):
    for k, v in kv.items():
        ctx.set_option(k, v)


@pytest.mark.parametrize("kind,cls", SCANNED, ids=_ids(SCANNED))
def test_gate_stage_inside_k_finalize(ctx, oracle, kind, cls):
    import torch
    cases = C.cases_of(kind, cls)
    keep, probs, ds, _ = _scan_tables(ctx, cases)
    cnt = torch.zeros(len(cases), dtype=torch.int32, device=ds[0].out.device)
    try:
        _options(ctx, post_fuse=1, fuse=1, col_split=1)
        plan = ctx.plan(probs)
    finally:
        _options(ctx, post_fuse=0, fuse=0, col_split=0)
    plan.add_stereo_gates([d.gate(cnt.data_ptr() + 4 * i) for i, d in enumerate(ds)])
    assert not plan.key_state() & KEYS_COLUMNS_NOT_IN_MEMORY
    w16 = torch.zeros(cases[0].n_l, dtype=torch.int16, device=cnt.device)
    plan.set_wire16(ds[0].m.data_ptr(), w16.data_ptr(), cases[0].n_l)         # accepted: k_finalize writes this plan's tables
    plan.set_wire16(ds[0].m.data_ptr(), 0, cases[0].n_l)
    _run_and_compare(ctx, plan, ds, cnt, True)
    plan.close()


@pytest.mark.parametrize("kind,cls", SCANNED, ids=_ids(SCANNED))
def test_gate_stage_inside_the_fused_stage(ctx, oracle, kind, cls):
    import torch
    import plslam_amd
    cases = [c for c in C.cases_of(kind, cls) if C.scan_mutual(c)]
    keep, probs, ds, _ = _scan_tables(ctx, cases)
    cnt = torch.zeros(len(cases), dtype=torch.int32, device=ds[0].out.device)
    try:
        _options(ctx, scan_variant=plslam_amd.SCAN_MFMA, post_fuse=2)
        plan = ctx.plan(probs)
    finally:
        _options(ctx, scan_variant=plslam_amd.SCAN_AUTO, post_fuse=0)
    plan.add_stereo_gates([d.gate(cnt.data_ptr() + 4 * i) for i, d in enumerate(ds)])
    assert plan.key_state() & KEYS_COLUMNS_NOT_IN_MEMORY                       # k_post_fused it is
    _run_and_compare(ctx, plan, ds, cnt, True)
    plan.close()


@pytest.mark.parametrize("kind,cls", SCANNED, ids=_ids(SCANNED))
def test_batched_gate_kernel_behind_a_fused_plan(ctx, oracle, kind, cls):
    import torch
    import plslam_amd
    from plslam_amd.capi import ENOTSUP, PlslamError
    cases = [c for c in C.cases_of(kind, cls) if C.scan_mutual(c)]
    keep, probs, ds, _ = _scan_tables(ctx, cases)
    cnt = torch.zeros(len(cases), dtype=torch.int32, device=ds[0].out.device)
    try:
        _options(ctx, scan_variant=plslam_amd.SCAN_MFMA, fuse=2, col_split=1)
        plan = ctx.plan(probs)
    finally:
        _options(ctx, scan_variant=plslam_amd.SCAN_AUTO, fuse=0, col_split=0)
    w16 = torch.zeros(cases[0].n_l, dtype=torch.int16, device=cnt.device)
    with pytest.raises(PlslamError) as e:                                      # no finalize kernel in this plan: it is fused
        plan.set_wire16(ds[0].m.data_ptr(), w16.data_ptr(), cases[0].n_l)
    assert e.value.code == ENOTSUP
    plan.add_stereo_gates([d.gate(cnt.data_ptr() + 4 * i) for i, d in enumerate(ds)])
    _run_and_compare(ctx, plan, ds, cnt, True)
    plan.close()


@pytest.mark.parametrize("kind,cls", CLASSES, ids=_ids(CLASSES))
def test_batched_gate_kernel_over_tables_outside_the_plan(ctx, oracle, kind, cls):
    import torch
    dev = torch.device("cuda", ctx.device)
    cases = C.cases_of(kind, cls)
    r = np.random.Generator(np.random.PCG64(3))
    d8 = torch.from_numpy(r.integers(0, 256, (16, 32), dtype=np.uint8)).to(dev)
    own = torch.full((8,), -2, dtype=torch.int32, device=dev)
    plan = ctx.plan([(d8.data_ptr(), 8, d8.data_ptr() + 8 * 32, 8, 0.75, True, own.data_ptr(), 0)])
    ds = [_Dev(ctx, c) for c in cases]
    cnt = torch.zeros(len(cases), dtype=torch.int32, device=dev)
    plan.add_stereo_gates([d.gate(cnt.data_ptr() + 4 * i) for i, d in enumerate(ds)])
    _run_and_compare(ctx, plan, ds, cnt, False)
    plan.add_stereo_gates([d.gate(0) for d in ds])                             # and without counters
    for d in ds:
        d.refill()
    torch.cuda.synchronize()
    plan.run(0)
    torch.cuda.synchronize()
    for d in ds:
        _same(d.c.name, d.result(), _ref(d.c.name), count=False)
    plan.close()


def test_committed_fixture_no_oracle(ctx):
    """GPU vs tests/golden/stereo_gate_edges.npz: nothing of the oracle at run time."""
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "stereo_gate_edges.npz"))
    for k in g["names"].tolist():
        kind = k.split("/")[0]
        c = C.Case(k, "", "", kind, g[k + ":m12"].shape[0], g[k + ":m12"], g[k + ":f_l"], g[k + ":f_r"], tuple(g[k + ":th"].tolist()), {}, [])
        _same(k, _host(ctx, c), (g[k + ":stereo"], g[k + ":disp"], int(g[k + ":n"])))


def test_point_gate_semantics_on_the_device(ctx):
    """test_stereo_gates.py::test_point_gate_semantics, its inputs as they stand."""
    kp_l = np.array([[100.0, 50.0], [100.0, 50.0], [100.0, 50.0], [100.0, 50.0], [10.0, 10.0]], np.float32)
    kp_r = np.array([[90.0, 50.5], [90.0, 51.5], [99.5, 50.0], [99.0, 50.0]], np.float32)
    m12 = np.array([0, 1, 2, 3, -1], np.int32)
    out, disp, n = ctx.stereo_point_gate(m12, kp_l, kp_r, 1.0, 1.0)
    assert out.tolist() == [0, -1, -1, 3, -1] and n == 2
    assert disp.tolist() == [10.0, 0.0, 0.0, 1.0, 0.0]
    assert ctx.stereo_point_gate(m12, kp_l, kp_r, 0.0, 1.0)[0].tolist() == [-1, -1, -1, 3, -1]
    a = np.array([[5.0, 16777216.0]], np.float32)
    b = np.array([[1.0, 16777215.0]], np.float32)
    assert ctx.stereo_point_gate([0], a, b, 1.0, 1.0)[2] == 1


def test_line_gate_semantics_on_the_device(ctx):
    """test_stereo_gates.py::test_line_gate_semantics, its gate inputs as they stand (lineSegmentOverlapStereo alone has no
    entry point on the device: its three branches are the overlap_branches class)."""
    seg_l = np.array([[100, 10, 100, 60]], np.float32)
    seg_r = np.array([[90, 10, 90, 60]], np.float32)
    out, d, n = ctx.stereo_line_gate([0], seg_l, seg_r, 1.0, 0.1, 0.75, 0.7)
    assert out.tolist() == [0] and n == 1 and d.tolist() == [[10.0, 10.0]]
    assert ctx.stereo_line_gate([0], seg_l, np.array([[90, 10, 90, 35]], np.float32), 1.0, 0.1, 0.75, 0.7)[2] == 0
    assert ctx.stereo_line_gate([0], seg_l, np.array([[90, 10, 90, 35]], np.float32), 1.0, 0.1, 0.4, 0.7)[2] == 1
    assert ctx.stereo_line_gate([0], seg_l, np.array([[90, 10, 96, 60]], np.float32), 1.0, 0.1, 0.75, 0.7)[2] == 0
    assert ctx.stereo_line_gate([0], np.array([[100, 10, 160, 10.05]], np.float32), seg_r, 1.0, 0.1, 0.75, 0.7)[2] == 0
