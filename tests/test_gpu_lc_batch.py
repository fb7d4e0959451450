"""K54 (plslam_amd/csrc/loop_closure.hip): B loop-closure candidates in one call.  The batched call runs the single call's
per-problem code in B workgroups, so "batched equals single, bit for bit" is the test; the restatement (tests/lc_ref.py) is
compared with the tolerances and margins of tests/test_gpu_loop_closure.py.  tests/test_lc_batch_cpu.py pins the branches
the batch takes."""
import ctypes

import numpy as np
import pytest

import plslam_amd
from plslam_amd import loop_closure as LC

import lc_batch_cases as CASES
import lc_cases
import lc_ref
from test_gpu_loop_closure import _check

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
RES = ctypes.sizeof(plslam_amd.LcResult)
KF_KEYS = ("pdesc", "P", "pl", "pt_idx", "ldesc", "sPeP", "le", "ls_idx")


@pytest.fixture(scope="module")
def ctx():
    c = plslam_amd.Context(0)
    yield c
    c.close()


class Dev:
    """device copies of keyframe dicts (one per dict, however often it appears) and of output buffers"""

    def __init__(self):
        self.dev = torch.device("cuda:0")
        self.keep = []
        self.recs = {}
        self.stream = torch.cuda.Stream(self.dev)

    def put(self, a):
        t = torch.from_numpy(np.ascontiguousarray(a)).to(self.dev)
        self.keep.append(t)
        return t.data_ptr() if t.numel() else 0

    def rec(self, kf):
        if id(kf) not in self.recs:
            self.keep.append(kf)
            self.recs[id(kf)] = dict({k: 0 if kf[k] is None else self.put(kf[k]) for k in KF_KEYS}, n_pt=len(kf["P"]),
                                     n_ls=len(kf["sPeP"]))
        return self.recs[id(kf)]

    def outputs(self, n_res, n_pt, n_ls):
        z = lambda shape, dt: torch.full(shape, 0x5A if dt == torch.uint8 else 0x5A5A5A5A, dtype=dt, device=self.dev)
        return (z((n_res * RES,), torch.uint8), z((max(n_pt, 1), 4), torch.int32), z((max(n_pt, 1),), torch.uint8),
                z((max(n_ls, 1), 4), torch.int32), z((max(n_ls, 1),), torch.uint8))


def _unpack(out, B, n_pts, n_lss):
    res, pc, pi, lc, li = (t.cpu().numpy() for t in out)
    rp, rl, got = 0, 0, []
    for b in range(B):
        d = plslam_amd.LcResult.from_buffer_copy(res[b * RES:(b + 1) * RES].tobytes()).as_dict()
        n, m = d["common_pt"], d["common_ls"]
        assert 0 <= n <= n_pts[b] and 0 <= m <= n_lss[b]
        got.append((d, pc[rp:rp + n].copy(), pi[rp:rp + n].astype(bool), lc[rl:rl + m].copy(), li[rl:rl + m].astype(bool)))
        rp += n_pts[b]
        rl += n_lss[b]
    return got


def run_batch_dev(dv, batch, prs):
    """prs: [(kf0, kf1), ...] -> per pair (result dict, pt_corr, pt_inlier, ls_corr, ls_inlier) from the device form"""
    r0, r1 = [dv.rec(p[0]) for p in prs], [dv.rec(p[1]) for p in prs]
    n_pts, n_lss = [r["n_pt"] for r in r0], [r["n_ls"] for r in r0]
    out = dv.outputs(len(prs), sum(n_pts), sum(n_lss))
    batch.verify_dev(r0, r1, *(t.data_ptr() for t in out), stream=dv.stream.cuda_stream)
    dv.stream.synchronize()
    return _unpack(out, len(prs), n_pts, n_lss)


def run_single_dev(dv, ctx, p, kf0, kf1):
    r0, r1 = dv.rec(kf0), dv.rec(kf1)
    out = dv.outputs(1, r0["n_pt"], r0["n_ls"])
    ctx.loop_closure_verify_dev(p, r0, r1, *(t.data_ptr() for t in out), stream=dv.stream.cuda_stream)
    dv.stream.synchronize()
    return _unpack(out, 1, [r0["n_pt"]], [r0["n_ls"]])[0]


def same(a, b):
    return CASES.same_result(a[0], b[0]) and all(np.array_equal(x, y) for x, y in zip(a[1:], b[1:]))


def _prs(seed=CASES.SEED, n=CASES.B, **kw):
    return [(k0, k1) for k0, k1, _ in CASES.pairs(seed, n, **kw)]


@pytest.mark.parametrize("name", sorted(CASES.PARAM_SETS))
def test_batched_equals_single_bit_for_bit(ctx, name):
    p = LC.params(**CASES.PARAM_SETS[name])
    dv, prs = Dev(), _prs()
    batch = plslam_amd.LcBatch(ctx, p, 16)
    got = run_batch_dev(dv, batch, prs)
    single = [run_single_dev(dv, ctx, p, *pr) for pr in prs]
    for b in range(len(prs)):
        assert same(got[b], single[b]), (name, b)
    for b in (0, 3, 5):                                   # B = 1
        assert same(run_batch_dev(dv, batch, [prs[b]])[0], single[b]), (name, b)
    batch.close()


@pytest.mark.parametrize("name", sorted(CASES.PARAM_SETS))
def test_against_the_restatement(ctx, name):
    p = LC.params(**CASES.PARAM_SETS[name])
    batch = plslam_amd.LcBatch(ctx, p, CASES.B)
    got = batch.verify(_prs())
    for b, dev in enumerate(got):
        ref, prm = CASES.reference(name, b)
        _check(*dev, ref, prm)
    batch.close()


def test_placement_independence(ctx):
    p = LC.params()
    dv = Dev()
    prs = _prs()
    batch = plslam_amd.LcBatch(ctx, p, 1024)
    base = run_batch_dev(dv, batch, prs)
    perm = [5, 2, 7, 0, 3, 6, 1, 4]
    got = run_batch_dev(dv, batch, [prs[i] for i in perm])
    for k, i in enumerate(perm):
        assert same(got[k], base[i]), (k, i)
    # 1024 workgroups over 32 distinct pairs whose device arrays repeat: period 32, bit for bit
    distinct = _prs(9, 32, sizes=((1500, 200), (800, 100), (300, 40)))
    first = run_batch_dev(dv, batch, distinct)
    big = run_batch_dev(dv, batch, [distinct[b % 32] for b in range(1024)])
    for b in range(1024):
        assert same(big[b], first[b % 32]), b
    assert any(r[0]["is_lc"] for r in first) and any(not r[0]["gn_ran"] for r in first)
    again = run_batch_dev(dv, batch, [distinct[b % 32] for b in range(1024)])          # one repeat
    for b in range(1024):
        assert same(again[b], big[b]), b
    batch.close()


@pytest.mark.parametrize("pset", sorted(lc_cases.PARAM_SETS))
def test_every_case_in_one_call_in_two_orders(ctx, pset):
    """A batch has one parameter record, so every case of tests/lc_cases.py runs under each of the cases' five parameter
    sets: one batched call over all of them, another in a seeded other order, each record bit for bit its single call.  The
    cases that belong to the set are compared with the restatement as well."""
    over, cam = lc_cases.PARAM_SETS[pset]
    p = LC.params(cam, **over)
    dv = Dev()
    names = list(lc_cases.NAMES)
    prs = [lc_cases.case(n)[2:] for n in names]
    batch = plslam_amd.LcBatch(ctx, p, len(prs))
    single = [run_single_dev(dv, ctx, p, *pr) for pr in prs]
    got = run_batch_dev(dv, batch, prs)
    perm = [int(i) for i in np.random.Generator(np.random.PCG64(5)).permutation(len(prs))]
    assert perm != list(range(len(prs)))
    other = run_batch_dev(dv, batch, [prs[i] for i in perm])
    for b, n in enumerate(names):
        assert same(got[b], single[b]), (pset, n)
    for k, i in enumerate(perm):
        assert same(other[k], single[i]), (pset, names[i], k)
    own = [n for n in lc_cases.VALUE_COMPARED if lc_cases.param_set_of(n) == pset]
    assert own
    for n in own:
        ref, prm, _ = lc_cases.reference(n)
        _check(*got[names.index(n)], ref, prm)
    batch.close()


def test_shared_kf1_across_eight_pairs(ctx):
    """the top-K shape: eight candidates against one current keyframe"""
    p = LC.params()
    dv = Dev()
    kf0, kf1, _ = LC.keyframe_pair(123, 1500, 200)
    rng = np.random.Generator(np.random.PCG64(124))
    cands = []
    for k in range(8):                                     # candidate k: the first 180 k point rows and 24 k line rows are strangers
        c = dict(kf0)
        c["pdesc"], c["ldesc"] = kf0["pdesc"].copy(), kf0["ldesc"].copy()
        c["pdesc"][:180 * k] = rng.integers(0, 256, (180 * k, 32), dtype=np.uint8)
        c["ldesc"][:24 * k] = rng.integers(0, 256, (24 * k, 32), dtype=np.uint8)
        cands.append(c)
    prs = [(c, kf1) for c in cands]
    batch = plslam_amd.LcBatch(ctx, p, 8)
    got = run_batch_dev(dv, batch, prs)
    host = batch.verify(prs)
    for k, pr in enumerate(prs):
        assert same(got[k], run_single_dev(dv, ctx, p, *pr)), k
        assert same(got[k], host[k]), k
    assert got[0][0]["is_lc"] == 1 and got[7][0]["gn_ran"] == 0
    assert len({r[0]["common_pt"] for r in got}) == 8
    batch.close()


def test_host_form_equals_device_form(ctx):
    p = LC.params(has_lines=0)
    dv, prs = Dev(), _prs()
    batch = plslam_amd.LcBatch(ctx, p, CASES.B)
    host, dev = batch.verify(prs), run_batch_dev(dv, batch, prs)
    for b in range(len(prs)):
        assert same(host[b], dev[b]), b
    again = batch.verify(prs[:3])                          # a shorter batch through the same object
    for b in range(3):
        assert same(again[b], dev[b]), b
    assert batch.verify([]) == []
    batch.close()


def test_relpose_batched_equals_the_single_call(ctx):
    p = LC.params()
    prm = LC.params_dict(p)
    dv = Dev()
    probs = []
    for b in (0, 2, 3, 6, 7):
        ref, _ = CASES.reference("pl", b)
        probs.append(tuple(np.ascontiguousarray(x) for x in ref["corr_inputs"]))
    P0, pl0, S0, le0 = probs[0]
    probs.append((P0[:200], pl0[:200], S0[:0], le0[:0]))           # a problem without lines, and one without points
    probs.append((P0[:0], pl0[:0], S0[:90], le0[:90]))
    for sel in (range(len(probs)), [1]):                          # B = 7 and B = 1
        sub = [probs[i] for i in sel]
        B = len(sub)
        pt_off = np.concatenate([[0], np.cumsum([len(q[0]) for q in sub])]).astype(np.int32)
        ls_off = np.concatenate([[0], np.cumsum([len(q[2]) for q in sub])]).astype(np.int32)
        cat = [np.concatenate([q[i] for q in sub]) for i in range(4)]
        res = torch.zeros(B * RES, dtype=torch.uint8, device=dv.dev)
        pi = torch.full((int(pt_off[-1]),), 0x5A, dtype=torch.uint8, device=dv.dev)
        li = torch.full((int(ls_off[-1]),), 0x5A, dtype=torch.uint8, device=dv.dev)
        ctx.relpose_robust_gn_batched_dev(p, dv.put(cat[0]), dv.put(cat[1]), dv.put(pt_off), dv.put(cat[2]), dv.put(cat[3]),
                                          dv.put(ls_off), B, res.data_ptr(), pi.data_ptr(), li.data_ptr(),
                                          stream=dv.stream.cuda_stream)
        dv.stream.synchronize()
        r, pi, li = res.cpu().numpy(), pi.cpu().numpy().astype(bool), li.cpu().numpy().astype(bool)
        for b, q in enumerate(sub):
            d = plslam_amd.LcResult.from_buffer_copy(r[b * RES:(b + 1) * RES].tobytes()).as_dict()
            one, opi, oli = ctx.relpose_robust_gn(p, *q)
            assert CASES.same_result(d, one), b
            assert np.array_equal(pi[pt_off[b]:pt_off[b + 1]], opi) and np.array_equal(li[ls_off[b]:ls_off[b + 1]], oli), b
    ref = lc_ref.relpose_robust_gn(prm, CASES.OCAM, *probs[0])
    one = ctx.relpose_robust_gn(p, *probs[0])
    assert one[0]["is_lc"] == ref["is_lc"] == 1


def test_validation_leaves_the_batch_usable(ctx):
    L = plslam_amd.load()
    EINVAL, ERANGE = plslam_amd.capi.EINVAL, plslam_amd.capi.ERANGE
    p = LC.params()
    h = ctypes.c_void_p()
    for bad in (dict(max_iters=-1), dict(max_iters_ref=plslam_amd.capi.LC_MAX_ITERS + 1)):
        assert L.plslam_lc_batch_create(ctx._h, ctypes.byref(LC.params(**bad)), 4, ctypes.byref(h)) == EINVAL
    assert L.plslam_lc_batch_create(ctx._h, ctypes.byref(p), 0, ctypes.byref(h)) == EINVAL
    assert L.plslam_lc_batch_create(ctx._h, ctypes.byref(p), plslam_amd.capi.LC_MAX_BATCH + 1, ctypes.byref(h)) == ERANGE
    assert L.plslam_lc_batch_create(ctx._h, None, 4, ctypes.byref(h)) == EINVAL
    prs = _prs()[:4]
    batch = plslam_amd.LcBatch(ctx, p, 4)
    good = batch.verify(prs)

    def still_good():
        now = batch.verify(prs)
        assert all(same(a, b) for a, b in zip(now, good))

    K = plslam_amd.LcKeyframe
    recs = (K * 5)()
    res = (plslam_amd.LcResult * 5)()
    call = lambda r0, r1, B: L.plslam_lc_batch_verify(batch._h, r0, r1, B, res, None, None, None, None)
    assert call(recs, recs, -1) == EINVAL                  # B < 0
    still_good()
    assert call(recs, recs, 5) == EINVAL                   # B > max_pairs
    still_good()
    assert call(recs, recs, 0) == plslam_amd.capi.OK       # B == 0: nothing is launched
    assert call(None, None, 2) == EINVAL
    still_good()
    recs[1].n_pt = -1
    assert call(recs, recs, 2) == EINVAL                   # a negative size in pair 1
    still_good()
    recs[1].n_pt = 3
    assert call(recs, recs, 2) == EINVAL                   # rows without arrays
    still_good()
    big0, big1, _ = LC.keyframe_pair(22, plslam_amd.capi.LC_MAX_FEATURES + 1, 8)
    with pytest.raises(plslam_amd.PlslamError) as ei:
        batch.verify([prs[0], (big0, big1)])
    assert ei.value.code == ERANGE
    still_good()
    with pytest.raises(plslam_amd.PlslamError) as ei:      # the device form without outputs for a kind that has rows
        dv = Dev()
        r0, r1 = dv.rec(prs[0][0]), dv.rec(prs[0][1])
        batch.verify_dev([r0], [r1], dv.outputs(1, 1, 1)[0].data_ptr(), 0, 0, 0, 0)
    assert ei.value.code == EINVAL
    still_good()
    # the batched GN: B < 0, missing offsets, half a kind
    z = ctypes.c_void_p(0)
    one = ctypes.c_void_p(256)
    f = L.plslam_relpose_robust_gn_batched_dev
    assert f(ctx._h, p, one, one, one, z, z, one, -1, one, one, z, z) == EINVAL
    assert f(ctx._h, p, one, one, z, z, z, one, 1, one, one, z, z) == EINVAL
    assert f(ctx._h, p, one, z, one, z, z, one, 1, one, one, z, z) == EINVAL
    assert f(ctx._h, p, one, one, one, z, z, one, 0, z, z, z, z) == plslam_amd.capi.OK
    assert f(ctx._h, p, one, one, one, z, z, one, plslam_amd.capi.LC_MAX_BATCH + 1, one, one, z, z) == ERANGE
    still_good()
    batch.close()
