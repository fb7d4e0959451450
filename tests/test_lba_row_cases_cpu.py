"""What the cases of tests/lba_row_cases.py cover is a condition on their inputs: the Python restatement alone must take each
class to the switch it is named for (membership), its mutants must be told apart from it on a special row of the class meant
for them, the C oracle must agree with it bit for bit on every case (NaNs and signed zeros included), the oracle's rows on the
finite classes are pinned to the reference's own observation loops (src/mapHandler.cpp:1358-1431, :1436-1540 compiled
textually into oracle/_ref, or their recorded g and err in tests/golden/ref_calls_golden.npz), and they agree with an
order-free numpy.longdouble restatement within the contract's 1e-6 relative (BASELINE.json north_star)."""
import numpy as np
import pytest

from oracle import oracle as O

import lba_row_cases as R
from test_oracle_pin import _reference

CAM = O.make_cam(**R.K)
KINDS_CLASSES = R.classes()
RTOL = 1e-6


def _ids(kc):
    return f"{kc[0]}-{kc[1]}"


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _oracle(c, compat=False):
    with np.errstate(all="ignore"):
        if c.kind == "points":
            return O.lba_point_rows(CAM, *R.row_args(c))
        return O.lba_line_rows(CAM, *R.row_args(c), compat_iter_pass=compat)


def _passes(c):
    return (False,) if c.kind == "points" else (False, True)


@pytest.mark.parametrize("kc", KINDS_CLASSES, ids=_ids)
def test_membership(kc):
    for n in R.SIZES:
        assert [c for c in R.cases_of(*kc) if c.n == n], (kc, n)
    for c in R.cases_of(*kc):
        logs = []
        R.restate(c, logs=logs)
        assert c.rows and c.rows[0] == 0, c.name
        for p, j in c.rows.items():
            s = c.specials[j]
            assert s.tags <= set(logs[p]), (c.name, p, sorted(s.tags - set(logs[p])), logs[p])
            assert c.kf[p] == s.slot
        if kc[1] in R.FINITE:
            assert all(("row", "nonfinite") not in lg for lg in logs), c.name
        if kc[1] == "slot_edges":
            assert {31, 32, 33, R.N_SLOTS - 1} <= {int(c.kf[p]) for p in c.rows} or c.n == 1


# ---- the mutants ------------------------------------------------------------------------------------------------------------
MUTANTS = {
    "dmax_gt's operands swapped": (dict(dmax=lambda a, b: b if b > a else a), ("nan_inf", "depth_zero"), False),
    "1/th where 1/z^2 belongs": (dict(k=lambda th, z2, dmax: R.ddiv(1.0, th)), ("depth_sq_at_th",), False),
    "1/z^2 where 1/th belongs": (dict(k=lambda th, z2, dmax: R.ddiv(1.0, z2)), ("depth_sq_at_th",), False),
    "the stride-6 read in the compat pass": (dict(compat_stride=6), ("tails", "slot_edges", "residual_at_th"), True),
    "homogTh for the compat pass's literal 1e-7": (None, ("residual_at_th", "depth_sq_at_th"), True),
}


def test_every_mutant_is_told_apart_by_its_class(capsys):
    """Each mutant's rows differ in their BITS from the restatement's on a special row of the classes meant for it (the compat
    pass's stride: on any row, it moves every landmark), at every size above 1.  Prints mutant -> classes."""
    killed = {}
    for name, (ops, classes, compat) in MUTANTS.items():
        for kind in ("points", "lines"):
            if compat and kind == "points":
                continue
            by, hit = set(), set()
            for c in R.all_cases():
                if c.kind != kind:
                    continue
                a, b = R.restate(c, compat), R.restate(c, compat, ops if ops is not None else dict(compat_th=c.th))
                rows = range(c.n) if (compat and ops is not None) else c.rows
                diff = np.zeros(c.n, bool)
                for x, y in zip(a, b):
                    diff |= (_bits(x).reshape(c.n, -1) != _bits(y).reshape(c.n, -1)).any(1)
                if any(diff[p] for p in rows):
                    by.add(c.cls)
                    hit.add((c.cls, c.n))
            killed[(name, kind)] = sorted(by)
            for cls in classes:
                need = {(cls, n) for n in R.SIZES if n > 1}
                if cls == classes[0]:
                    assert need <= hit, (name, kind, sorted(need - hit))
    with capsys.disabled():
        for (name, kind), by in killed.items():
            print(f"\n  mutant [{kind}] {name} -> {', '.join(by)}", end="")
        print()


# ---- the oracle -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kc", KINDS_CLASSES, ids=_ids)
def test_oracle_agrees_with_the_restatement(kc):
    for c in R.cases_of(*kc):
        for compat in _passes(c):
            for a, b in zip(_oracle(c, compat), R.restate(c, compat)):
                assert np.array_equal(_bits(a), _bits(b)), (c.name, compat)
                assert (_bits(a)[np.isnan(a)] == np.uint64(R.ONE_NAN_BITS)).all(), (c.name, compat)     # one NaN, not the host's


# ---- the contract's tolerance against an order-free long double restatement -----------------------------------------------------
def _ld_row(kind, th, T, lm, ob):
    L = np.longdouble
    T = np.asarray(T, L).reshape(4, 4)
    Rm, t = T[:3, :3].T, -(T[:3, :3].T @ T[:3, 3])
    fx, fy, cx, cy = (L(R.K[k]) for k in ("fx", "fy", "cx", "cy"))
    ob = np.asarray(ob, L)

    def cam(X):
        g = Rm @ np.asarray(X, L) + t
        return g, cx + fx * g[0] / g[2], cy + fy * g[1] / g[2]

    def j6(g, a, b):
        k = 1 / max(L(th), g[2] * g[2])
        gx, gy, gz = g
        return k * np.array([a * gz, b * gz, -(a * gx + b * gy), -(a * gx * gy + b * gy * gy + b * gz * gz),
                             a * gx * gx + a * gz * gz + b * gx * gy, b * gx * gz - a * gy * gz], L)
    if kind == "points":
        g, u, v = cam(lm)
        dx, dy = ob[0] - u, ob[1] - v
        r = np.sqrt(dx * dx + dy * dy)
        Jc = j6(g, fx * dx, fy * dy)
        den = max(L(th), r)
        return Jc / den, (Jc[:3] @ Rm) / den, r, 1 / (1 + r * r)
    P, pu, pv = cam(lm[:3])
    Q, qu, qv = cam(lm[3:])
    e0, e1 = ob[0] * pu + ob[1] * pv + ob[2], ob[0] * qu + ob[1] * qv + ob[2]
    r = np.sqrt(e0 * e0 + e1 * e1)
    JP, JQ = j6(P, fx * e0, fy * e1), j6(Q, fx * e0, fy * e1)
    den = max(L(th), r)
    return (JP * e0 + JQ * e1) / den, np.concatenate([(JP[:3] @ Rm) * e0, (JQ[:3] @ Rm) * e1]) / den, r, 1 / (1 + r * r)


@pytest.mark.parametrize("kc", [kc for kc in KINDS_CLASSES if kc[1] in R.FINITE], ids=_ids)
def test_finite_rows_within_the_contract_of_a_long_double_restatement(kc):
    """Every row of the finite classes against numpy.longdouble arithmetic that keeps no operation order: 1e-6 relative to the
    row's largest entry per output (r and w on their own).  Left out, with the reason: the rows that sit exactly ON a dmax_gt
    switch (the two sides legitimately differ in which operand they pass on -- the same number), and the rows whose residual is
    exactly zero in double arithmetic: there the observation EQUALS the rounded projection, the long double one differs from
    it by its rounding error, and the relative error of a difference of equal numbers has no bound."""
    if np.finfo(np.longdouble).eps >= np.finfo(np.float64).eps:
        pytest.skip("numpy.longdouble is no wider than double here")
    checked = 0
    for c in R.cases_of(*kc):
        if c.n not in (65, 257):
            continue
        got = _oracle(c)
        logs = []
        R.restate(c, logs=logs)
        flat = c.LM.reshape(c.n, -1)
        for i in range(c.n):
            j = c.rows.get(i)
            if (j is not None and c.specials[j].on_switch) or ("nrm", "zero") in logs[i] or ("e0", "zero") in logs[i] or ("e1", "zero") in logs[i]:
                continue
            exp = _ld_row(c.kind, c.th, c.T[c.kf[i]], flat[c.lm[i]], c.obs[i])
            for g, e in zip((got[0][i], got[1][i], got[2][i], got[3][i]), exp):
                e = np.atleast_1d(np.asarray(e, np.longdouble))
                scale = np.abs(e).max()
                assert float(np.abs(np.atleast_1d(g) - e).max()) <= RTOL * float(scale), (c.name, i)
            checked += 1
    assert checked > 100


# ---- pinned to the reference's own loops ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("kc", [kc for kc in KINDS_CLASSES if kc[1] in R.FINITE], ids=_ids)
def test_pinned_to_reference_source_text(kc):
    """g and err after the reference's first-pass observation loop -- for lines also after its iteration-pass loop, whose
    threshold is the literal 1e-7 whatever homogTh says -- (compiled textually, or recorded by
    tests/golden/make_ref_calls_golden.py) against oracle.lba_accumulate of the oracle's rows, on the finite classes at n = 65:
    slot 0 is the key frame that is not optimised.  1e-11 relative as test_lba_rows_and_accumulation_pinned_to_reference_source_text
    (the stand-in for Eigen may round a three-term sum the other way)."""
    kind = kc[0]
    nkf = R.N_SLOTS - 1
    checked = 0
    for c in R.cases_of(*kc):
        if c.n != 65:
            continue
        pts = kind == "points"
        npt, nls = (c.n, 0) if pts else (0, c.n)
        e_i, e_f2, e_f3 = np.zeros(0, np.int32), np.zeros((0, 2)), np.zeros((0, 3))
        kf_loc = (c.kf - 1).astype(np.int32)
        Xw, Lw = (c.LM, np.zeros((0, 6))) if pts else (np.zeros((0, 3)), c.LM)
        a = (c.lm, c.kf, kf_loc, c.obs) if pts else (e_i, e_i, e_i, e_f2)
        b = (e_i, e_i, e_i, e_f3) if pts else (c.lm, c.kf, kf_loc, c.obs)

        for it in _passes(c):                                         # lines: also the iteration pass (:1668-1772)
            def live():
                r = O.ref_lba_accumulate(it, CAM, c.th, nkf, c.T, c.T[1:], Xw, Lw, *a, *b)
                return None if r is None else (r[1], np.float64(r[2]))
            g_ref, e_ref = _reference(f"lba_edges/{c.name}" + ("/iter" if it else ""), live)
            rows = _oracle(c, it)
            H, g, e = O.lba_accumulate(kind, nkf, npt, nls, c.lm, kf_loc, *rows)
            np.testing.assert_allclose(g_ref, g, rtol=1e-11, atol=1e-11 * np.abs(g).max(), err_msg=c.name)
            assert np.isclose(float(e_ref), e, rtol=1e-12), c.name
            if it and kc[1] in ("depth_sq_at_th", "residual_at_th"):
                # ... and the reference's iteration pass does NOT take homogTh: rows under the case's own th give another g
                wrong = R.restate(c, True, dict(compat_th=c.th))
                gw = O.lba_accumulate(kind, nkf, npt, nls, c.lm, kf_loc, *wrong)[1]
                assert not np.allclose(g_ref, gw, rtol=1e-6, atol=1e-6 * np.abs(g).max()), c.name
            checked += 1
    assert checked >= 1
