"""The cases of tests/lba_row_cases.py (the local-BA rows ON the switches of their two max(homogTh, .) terms, at depth zero and
with NaN / inf inputs; what they hold is checked without a device by tests/test_lba_row_cases_cpu.py) through every way the
rows run on the device.  Rows are compared with the oracle's as BIT PATTERNS (uint64 views): signed zeros and NaNs included.

  host calls   lba_point_rows / lba_line_rows (K3 / K4 on fresh device buffers; lines also with compat_iter_pass)
  _dev calls   lba_point_rows_dev / lba_line_rows_dev with n_pose_slots 0 (every pose from global memory) and stated as 70, 32
               and 31 (the workgroup's LDS copy holds the first min(n_pose_slots, 32) of the 70 matrices)
  alignment    the _dev calls with J_pose, J_lm, r, w based 8 bytes past a 16-byte boundary -- together and one at a time: the
               word-by-word branch of wave_store_rows, which no other test reaches (torch allocations are 256-byte aligned) --
               and with the observations and the landmarks 8 bytes past one (load3 / load6 / the double2 load of obs_uv);
               the outputs are carved out of buffers filled with a sentinel, and the words around them must stay untouched
  LbaPlan      for the finite classes, LbaPlan.iterate: err, g and the blocks against oracle.lba_accumulate of the oracle's rows
               under the bounds of test_gpu_lba._assert_blocks_match_dense"""
import numpy as np
import pytest

import plslam_amd

import lba_row_cases as R
from test_gpu_lba import _assert_blocks_match_dense

pytestmark = pytest.mark.gpu
KINDS_CLASSES = R.classes()
SENTINEL = np.uint64(0xDEADBEEFCAFEF00D)


def _ids(kc):
    return f"{kc[0]}-{kc[1]}"


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


@pytest.fixture(scope="module")
def cams(oracle):
    return plslam_amd.make_cam(**R.K), oracle.make_cam(**R.K)


_EXPECTED = {}


def _expected(c, compat, oracle, ocam):
    """The oracle's rows of one case, computed once and shared by the tests."""
    key = (c.name, compat)
    if key not in _EXPECTED:
        with np.errstate(all="ignore"):
            _EXPECTED[key] = oracle.lba_point_rows(ocam, *R.row_args(c)) if c.kind == "points" else \
                oracle.lba_line_rows(ocam, *R.row_args(c), compat_iter_pass=compat)
    return _EXPECTED[key]


def _passes(c):
    return (False,) if c.kind == "points" else (False, True)


def _assert_rows(got, exp, what):
    """The same uint64 words: signed zeros, and the NaN entries too -- the row kernels and the oracle both store an entry that
    is not a number as the one positive quiet NaN (one_nan), since which NaN an operation hands on is the hardware's choice."""
    for name, g, e in zip(("J_pose", "J_lm", "r", "w"), got, exp):
        g, e = np.asarray(g, np.float64).reshape(len(e), -1), np.asarray(e, np.float64).reshape(len(e), -1)
        bad = np.flatnonzero((_bits(g) != _bits(e)).any(1))
        assert bad.size == 0, (what, name, bad[:5].tolist(), g[bad[:2]], e[bad[:2]], _bits(g[bad[:1]]), _bits(e[bad[:1]]))
        nan = np.isnan(e)
        assert (_bits(e)[nan] == np.uint64(R.ONE_NAN_BITS)).all(), (what, name)


@pytest.mark.parametrize("kc", KINDS_CLASSES, ids=_ids)
def test_host_calls(ctx, oracle, cams, kc):
    cam, ocam = cams
    for c in R.cases_of(*kc):
        for compat in _passes(c):
            got = ctx.lba_point_rows(cam, *R.row_args(c)) if c.kind == "points" else \
                ctx.lba_line_rows(cam, *R.row_args(c), compat_iter_pass=compat)
            _assert_rows(got, _expected(c, compat, oracle, ocam), (c.name, compat))


def _carve(torch, dev, words, misaligned):
    """A float64 view of `words` doubles inside a sentinel-filled buffer, based 8 bytes past a 16-byte boundary (or on one), with
    at least four sentinel words either side -> (buffer as int64, view, first word)."""
    buf = torch.full((words + 16,), int(SENTINEL.astype(np.int64)), dtype=torch.int64, device=dev)
    s = 5 if misaligned else 4
    assert buf.data_ptr() % 16 == 0
    view = buf[s:s + words].view(torch.float64)
    assert view.data_ptr() % 16 == (8 if misaligned else 0)
    return buf, view, s


def _dev_rows(ctx, torch, dev, cam, c, compat, slots, mis_out=(False,) * 4, mis_in=False):
    """One _dev call on carved buffers -> the four outputs as numpy arrays; asserts that the sentinels around them are intact."""
    n, pts = c.n, c.kind == "points"
    wl = 3 if pts else 6
    T = torch.from_numpy(c.T).to(dev)
    lm, kf = torch.from_numpy(c.lm).to(dev), torch.from_numpy(c.kf).to(dev)
    ins = []
    for a in (c.LM, c.obs):
        b, v, _ = _carve(torch, dev, a.size, mis_in)
        v.copy_(torch.from_numpy(np.ascontiguousarray(a).reshape(-1)).to(dev))
        ins.append((b, v))
    outs = [_carve(torch, dev, w, m) for w, m in zip((6 * n, wl * n, n, n), mis_out)]
    p = [v.data_ptr() for _, v, _ in outs]
    if pts:
        ctx.lba_point_rows_dev(cam, c.th, T.data_ptr(), ins[0][1].data_ptr(), ins[1][1].data_ptr(), lm.data_ptr(), kf.data_ptr(), n,
                               *p, 0, n_pose_slots=slots)
    else:
        ctx.lba_line_rows_dev(cam, c.th, compat, T.data_ptr(), ins[0][1].data_ptr(), ins[1][1].data_ptr(), lm.data_ptr(), kf.data_ptr(), n,
                              *p, 0, n_pose_slots=slots)
    torch.cuda.synchronize()
    res = []
    for (buf, view, s), w in zip(outs, (6 * n, wl * n, n, n)):
        h = buf.cpu().numpy().view(np.uint64)
        assert (h[:s] == SENTINEL).all() and (h[s + w:] == SENTINEL).all(), (c.name, "a word outside the output was written")
        res.append(h[s:s + w].view(np.float64).copy())
    return res[0].reshape(n, 6), res[1].reshape(n, wl), res[2], res[3]


@pytest.mark.parametrize("kc", KINDS_CLASSES, ids=_ids)
def test_dev_calls_with_the_pose_count_stated_and_not(ctx, oracle, cams, kc):
    import torch
    cam, ocam = cams
    dev = torch.device("cuda", ctx.device)
    for c in R.cases_of(*kc):
        for compat in _passes(c):
            for slots in (0, R.N_SLOTS, 32, 31):
                got = _dev_rows(ctx, torch, dev, cam, c, compat, slots)
                _assert_rows(got, _expected(c, compat, oracle, ocam), (c.name, compat, slots))


@pytest.mark.parametrize("kind", ["points", "lines"])
def test_alignment_reaches_the_word_by_word_store(ctx, oracle, cams, kind):
    """Output bases at 8 (mod 16) take wave_store_rows' word-by-word branch (its test is gbase & 15; a wave's base is the
    array's plus a multiple of 64 rows = of 1536 or 3072 bytes): every size, odd and even tails, together and one output at a
    time; inputs at 8 (mod 16) with aligned outputs."""
    import torch
    cam, ocam = cams
    dev = torch.device("cuda", ctx.device)
    layouts = [((True,) * 4, False)] + [(tuple(i == j for i in range(4)), False) for j in range(4)] + [((False,) * 4, True), ((True,) * 4, True)]
    for cls in ("tails", "slot_edges"):
        for c in R.cases_of(kind, cls):
            for compat in _passes(c):
                for mis_out, mis_in in layouts:
                    got = _dev_rows(ctx, torch, dev, cam, c, compat, R.N_SLOTS, mis_out, mis_in)
                    _assert_rows(got, _expected(c, compat, oracle, ocam), (c.name, compat, mis_out, mis_in))


@pytest.mark.parametrize("kc", [kc for kc in KINDS_CLASSES if kc[1] in R.FINITE], ids=_ids)
def test_plan_iterate_on_the_finite_classes(ctx, oracle, cams, kc):
    cam, ocam = cams
    kind = kc[0]
    nkf = R.N_SLOTS - 1
    e_i, e2, e3 = np.zeros(0, np.int32), np.zeros((0, 2)), np.zeros((0, 3))
    for c in R.cases_of(*kc):
        pts = kind == "points"
        npt, nls = (c.n, 0) if pts else (0, c.n)
        kf_loc = (c.kf - 1).astype(np.int32)
        a = (c.lm, c.kf, kf_loc, c.obs) if pts else (e_i, e_i, e_i, e2)
        b = (e_i, e_i, e_i, e3) if pts else (c.lm, c.kf, kf_loc, c.obs)
        plan = plslam_amd.LbaPlan(ctx, cam, c.th, R.N_SLOTS, nkf, npt, nls, *a, *b)
        try:
            for compat in _passes(c):
                B = plan.iterate(c.T, c.LM if pts else np.zeros((0, 3)), np.zeros((0, 6)) if pts else c.LM, compat_iter_pass=compat)
                rows = _expected(c, compat, oracle, ocam)
                H, g, e = oracle.lba_accumulate(kind, nkf, npt, nls, c.lm, kf_loc, *rows)
                pr, lr = plan.rows()
                _assert_rows(pr if pts else lr, rows, (c.name, compat, "plan rows"))
                _assert_blocks_match_dense(B, H, g, nkf, npt, nls, a[0], a[2], b[0], b[2])
                assert abs(B["err"] - e) <= 1e-12 * abs(e), (c.name, compat)
        finally:
            plan.close()

