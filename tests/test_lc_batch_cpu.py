"""What the batched loop-closure tests cover is a condition on their inputs: the restatement alone (tests/lc_ref.py) must take
every branch on the test batch, or the device test (tests/test_gpu_lc_batch.py) proves nothing about that branch."""
import numpy as np

from plslam_amd import loop_closure as LC

import lc_batch_cases as CASES
from test_gpu_loop_closure import _margins

FLAGS = ("ok_res", "ok_unc", "ok_trs", "ok_rot")


def _same_kf(a, b):
    return all((a[k] is None and b[k] is None) or np.array_equal(a[k], b[k]) for k in a)


def test_keyframe_batch_is_deterministic_and_prefix_stable():
    one, two = LC.keyframe_batch(5, 6), LC.keyframe_batch(5, 6)
    for (a0, a1, ta), (b0, b1, tb) in zip(one, two):
        assert _same_kf(a0, b0) and _same_kf(a1, b1) and np.array_equal(ta["T"], tb["T"])
    longer = LC.keyframe_batch(5, 9)
    for (a0, a1, _), (b0, b1, _) in zip(one, longer):
        assert _same_kf(a0, b0) and _same_kf(a1, b1)                    # pair b does not depend on B
    other = LC.keyframe_batch(6, 6)
    assert not np.array_equal(one[0][0]["pdesc"], other[0][0]["pdesc"])
    # pair b is keyframe_pair at seed 1000 * seed + b with the variant's arguments
    k0, k1, _ = LC.keyframe_pair(5000, 1500, 200)
    assert _same_kf(k0, one[0][0]) and _same_kf(k1, one[0][1])


def test_the_test_batch_takes_every_branch_in_the_restatement():
    ps = CASES.pairs()
    assert len(ps) == CASES.B
    sizes = {(len(k0["P"]), len(k0["sPeP"])) for k0, _, _ in ps}
    assert {(800, 100), (1500, 200), (4000, 600)} <= sizes
    assert any(len(k0["sPeP"]) == 0 and len(k0["P"]) > 0 for k0, _, _ in ps)       # a keyframe with 0 features of a kind
    assert any(len(k0["P"]) == 0 and len(k0["sPeP"]) > 0 for k0, _, _ in ps)
    R = {(n, b): CASES.reference(n, b) for n in CASES.PARAM_SETS for b in range(CASES.B)}
    for (n, b), (ref, prm) in R.items():
        if ref["gn_ran"]:
            _margins(ref, prm)                   # no residual on the outlier threshold, no value within 1 % of its test
    for n in ("pl", "p", "l"):                   # every feature mode accepts some pair and stops some pair at the gate
        assert any(R[(n, b)][0]["is_lc"] for b in range(CASES.B)), n
        assert any(R[(n, b)][0]["gn_ran"] == 0 for b in range(CASES.B)), n
    # points only and lines only also as data: the pair without lines runs (and is accepted) where lines are off, the pair
    # without points where points are off, and the gate stops both on a NaN ratio where both kinds are on
    no_ls = next(b for b, (k0, _, _) in enumerate(ps) if len(k0["sPeP"]) == 0)
    no_pt = next(b for b, (k0, _, _) in enumerate(ps) if len(k0["P"]) == 0)
    assert R[("p", no_ls)][0]["is_lc"] == 1 and R[("l", no_pt)][0]["is_lc"] == 1
    assert R[("pl", no_ls)][0]["gn_ran"] == 0 and np.isnan(R[("pl", no_ls)][0]["inl_ratio_ls"])
    assert R[("pl", no_pt)][0]["gn_ran"] == 0 and np.isnan(R[("pl", no_pt)][0]["inl_ratio_pt"])
    # GN ran and exactly one of the four tests rejected the pair, for each of the four
    for q, flag in enumerate(FLAGS):
        want = tuple(int(i != q) for i in range(4))
        hit = [(n, b) for (n, b), (ref, _) in R.items() if ref["gn_ran"] and tuple(int(ref[f]) for f in FLAGS) == want]
        assert hit, f"no pair of the batch is rejected by {flag} alone"
        assert all(R[k][0]["is_lc"] == 0 for k in hit)
    # translation and rotation are rejected by the data under the shipped parameters
    assert any(R[("pl", b)][0]["gn_ran"] and not R[("pl", b)][0]["ok_trs"] for b in range(CASES.B))
    assert any(R[("pl", b)][0]["gn_ran"] and not R[("pl", b)][0]["ok_rot"] for b in range(CASES.B))


def test_same_result_compares_bits():
    a = dict(e=0.0, g=np.array([np.nan, 1.0]), is_lc=1, clk_total=5, clk_serial=1)
    assert CASES.same_result(a, dict(a, clk_total=9))
    assert not CASES.same_result(a, dict(a, e=-0.0))
    assert not CASES.same_result(a, dict(a, is_lc=0))
    assert CASES.same_result(a, dict(a, g=np.array([np.nan, 1.0])))
