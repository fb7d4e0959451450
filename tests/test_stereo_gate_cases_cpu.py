"""What the cases of tests/stereo_gate_cases.py cover is a condition on their inputs: the Python restatement alone must take
each class to the comparison outcome it is named for (reach), must agree with the C oracle bit for bit on every case
(agreement), and its mutants -- each one a function below that replaces ONE operation -- must differ from the oracle on the
class meant for them (otherwise the device tests over the same cases could not tell a wrong kernel from a right one).

Three of the mutants the issue lists cannot be told apart from the gates' OUTPUTS by any input; the tests below assert that
instead of pretending otherwise:
  (g) fmin / fmax for std::min / std::max differ only for a NaN operand (and the sign of a zero).  The operands are the y's of
      the two segments and the two disparities.  A NaN left y makes fabs(sp_l.y - ep_l.y) > th false: dropped.  A NaN right y
      reaches sx through sp_r.y / ep_r.y: disp_s is NaN: dropped.  A NaN disparity fails disp >= min_disp: dropped.  A zero's
      sign matters only in a division, and the only quotient of two zeros is NaN either way.  Not even the overlap
      function's value differs: with one NaN right y both forms give spn == epn or NaN, and the overlap is 0.
  (i) the clamp `overlap > 1.f` is never taken: see overlap_ratio in stereo_gate_cases.py.
  (f) one place at a time: the three fabs tests see the same value (see horiz_th_edges), so `>=` in one of them is undone by
      `>` in another; only all three together (the mutant of the issue) change a decision."""
import math

import numpy as np
import pytest

from oracle import oracle as O

import stereo_gate_cases as C


def _oracle(c):
    with np.errstate(all="ignore"):
        return (O.stereo_point_gate if c.kind == "points" else O.stereo_line_gate)(*C.case_args(c))


def _bits(d):
    return np.ascontiguousarray(d, np.float64).reshape(-1).view(np.uint64)


def _differing_rows(a, b):
    """Rows whose decision or disparity BITS differ."""
    n = a[0].shape[0]
    return int(((a[0] != b[0]) | (_bits(a[1]).reshape(n, -1) != _bits(b[1]).reshape(n, -1)).any(1)).sum())


# ---- the mutants: one replaced operation each -----------------------------------------------------------------------------------
def mutant_a(c):
    """dy subtracted in double"""
    return C.restate(c, dict(dy=lambda a, b: float(a) - float(b)))


def mutant_b(c):
    """< for <= on dy"""
    return C.restate(c, dict(dy_le=lambda d, th: d < th))


def mutant_c_point(c):
    """> for >= on the point disparity"""
    return C.restate(c, dict(disp_ge=lambda d, md, which: d > md if which == "p" else d >= md))


def mutant_c_start(c):
    """> for >= on disp_s"""
    return C.restate(c, dict(disp_ge=lambda d, md, which: d > md if which == "s" else d >= md))


def mutant_c_end(c):
    """> for >= on disp_e"""
    return C.restate(c, dict(disp_ge=lambda d, md, which: d > md if which == "e" else d >= md))


def mutant_d(c):
    """0.01 for 0.01f"""
    return C.restate(c, dict(len_th=0.01))


def mutant_e(c):
    """>= for > on the overlap threshold"""
    return C.restate(c, dict(ov_gt=lambda o, th: o >= th))


def mutant_f(c):
    """>= for > on line_horiz_th, three places"""
    return C.restate(c, dict(hz_gt=lambda v, th, where: v >= th))


def _mutant_f_one(where):
    return lambda c: C.restate(c, dict(hz_gt=lambda v, th, w: v >= th if w == where else v > th))


def _fmin(a, b):
    return b if a != a else a if b != b else min(a, b)


def _fmax(a, b):
    return b if a != a else a if b != b else max(a, b)


def mutant_g(c):
    """fmin / fmax for std::min / std::max"""
    return C.restate(c, dict(dmin=_fmin, dmax=_fmax))


def mutant_h(c):
    """ex computed from the original sp_r"""
    return C.restate(c, dict(ex_reads_new=False))


def mutant_i(c):
    """the overlap clamp at 1 dropped"""
    return C.restate(c, dict(clamp=False))


def mutant_j(c):
    """<= for < on the disparity ratio"""
    return C.restate(c, dict(ratio_lt=lambda r, th: r <= th))


# mutant -> the (kind, class) meant for it
KILLERS = [(mutant_a, "points", "dy_float_keeps"), (mutant_a, "points", "dy_float_drops"), (mutant_b, "points", "dy_equal"),
           (mutant_c_point, "points", "disp_equal"), (mutant_c_start, "lines", "min_disp_edges"),
           (mutant_c_end, "lines", "min_disp_edges"), (mutant_d, "lines", "length_001f"), (mutant_e, "lines", "overlap_ratio"),
           (mutant_f, "lines", "horiz_th_edges"), (mutant_h, "lines", "ex_reads_new_sp"), (mutant_j, "lines", "disp_ratio")]


@pytest.fixture(scope="module")
def results():
    """name -> (oracle's result, restatement's result, per-row logs); computed once."""
    out = {}
    for c in C.all_cases():
        logs = []
        out[c.name] = (_oracle(c), C.restate(c, logs=logs), logs)
    return out


def test_shapes_of_the_cases():
    cs = C.all_cases()
    assert len({c.name for c in cs}) == len(cs)
    for kind, cls in C.classes():
        of = C.cases_of(kind, cls)
        variants = {c.variant for c in of}
        assert {(c.variant, c.n_l) for c in of} == {(v, n) for v in variants for n in C.SIZES}, cls
    for c in cs:
        assert c.f_l.dtype == c.f_r.dtype == np.float32 and c.m12.dtype == np.int32 and all(type(t) is float for t in c.th)
        assert c.f_l.shape == (c.n_l, 2 if c.kind == "points" else 4)
        n_r = c.f_r.shape[0]
        assert n_r == (0 if c.variant == "empty_right" else c.n_l + 3)
        waves = {p // 64 for p in c.rows}
        last = (c.n_l - 1) // 64
        assert 0 in waves and last in waves and (c.n_l - 1) in c.rows          # first wave, the last lane of the launch
        assert last < 2 or (last + 1) // 2 in waves                           # a middle wave
        if c.cls != "index_edges":                                            # a scan can produce the table
            m = c.m12[c.m12 >= 0]
            assert len(set(m.tolist())) == len(m) and (m < n_r).all() and (c.m12 >= -1).all()


def test_reach(results):
    """Every special row's log holds the outcomes its class names, and it is kept / dropped as the class says -- by the
    restatement alone.  At n_l = 1 only one special fits; at every other size all of them are there."""
    reached = {}
    for c in C.all_cases():
        (_, (out, disp, n), logs) = results[c.name]
        assert c.n_l == 1 or set(c.rows.values()) == set(range(len(c.specials))), c.name
        for p, j in c.rows.items():
            _, _, tags, kept, _ = c.specials[j]
            assert tags <= set(logs[p]), (c.name, p, j, sorted(tags - set(logs[p])), logs[p])
            assert kept is None or (out[p] >= 0) == kept, (c.name, p, j, logs[p])
            for t in tags:
                reached.setdefault((c.kind, c.cls), set()).add(t)
        if c.n_l >= 63 and c.variant != "empty_right":
            assert out[c.n_l - 1] >= 0 or not any(s[3] for s in c.specials), c.name
    for key in C.classes():
        print(key, sorted(reached[key]))
    # the point of each class, spelled out once more against the union of what its rows reached
    need = {("points", "dy_float_keeps"): {("dy_sides", "float_keeps"), ("dy_sign", "pos"), ("dy_sign", "neg")},
            ("points", "dy_float_drops"): {("dy_sides", "float_drops"), ("dy_sign", "pos"), ("dy_sign", "neg")},
            ("points", "dy_equal"): {("dy", "eq")}, ("points", "disp_equal"): {("disp", "eq"), ("disp", "-1ulp_f32")},
            ("points", "index_edges"): {("index", k) for k in ("n_r", "last", "first", "below", "above", "none")},
            ("points", "nan_inf_coords"): {("dy", "nan"), ("disp", "nan"), ("kept", "inf")},
            ("lines", "horiz_th_edges"): {(w, r) for w in ("hz_ov", "hz_l", "hz_r") for r in ("eq", "+1ulp", "-1ulp")},
            ("lines", "length_001f"): {("length", "eq"), ("length", "between"), ("length", "+1ulp")},
            ("lines", "overlap_branches"): {("ov_branch", b) for b in ("disjoint_above", "disjoint_below", "containing", "partial")} |
                                           {("epn_sln", "eq"), ("spn_eln", "eq")},
            ("lines", "overlap_ratio"): {("ov_ratio", "eq"), ("ov", "eq")},
            ("lines", "disp_ratio"): {("disp_ratio", "eq"), ("disp_ratio", "negative"), ("disp_ratio", "0/0")},
            ("lines", "min_disp_edges"): {("disp_s", "eq"), ("disp_e", "eq"), ("disp_s", "lt"), ("disp_e", "lt")},
            ("lines", "right_horizontal"): {("right_horizontal", "inf"), ("right_horizontal", "nan"), ("kept", "inf")},
            ("lines", "zero_length"): {("shape", "both_points")}, ("lines", "identical"): {("shape", "identical")},
            ("lines", "ex_reads_new_sp"): {("ex_dep", "bits"), ("ex_dep", "decision")},
            ("lines", "index_edges"): {("index", k) for k in ("n_r", "last", "first", "below", "above", "none")}}
    assert set(need) == set(C.classes())
    for key, tags in need.items():
        assert tags <= reached[key], (key, sorted(tags - reached[key]))


def test_no_case_takes_the_clamp(results):
    for c in C.all_cases():
        assert not any(("clamp", "taken") in lg for lg in results[c.name][2]), c.name


def test_restatement_equals_the_oracle_bit_for_bit(results):
    rows = 0
    for c in C.all_cases():
        ref, got, _ = results[c.name]
        assert np.array_equal(got[0], ref[0]), c.name
        assert np.array_equal(_bits(got[1]), _bits(ref[1])), c.name
        assert got[2] == ref[2] == int((ref[0] >= 0).sum()), c.name
        rows += c.n_l
    print(len(C.all_cases()), "cases,", rows, "rows")


@pytest.mark.parametrize("mutant,kind,cls", KILLERS, ids=[f"{m.__name__}-{cls}" for m, _, cls in KILLERS])
def test_mutant_restatements_differ_from_the_oracle(results, mutant, kind, cls):
    """On EVERY case of the class meant for it (every variant, every size) at least one row differs."""
    total = 0
    for c in C.cases_of(kind, cls):
        d = _differing_rows(mutant(c), results[c.name][0])
        total += d
        only = {mutant_b: ("th0", "th1"), mutant_e: ("th1", "th075"), mutant_f: ("eq",), mutant_j: ("r05", "r07", "neg")}.get(mutant)
        if only is None or c.variant in only:
            assert d > 0, f"{mutant.__doc__}: 0 differing rows on {c.name}"
    print(f"{mutant.__name__} ({mutant.__doc__}): {total} differing rows over the cases of {cls}")
    assert total > 0, f"{mutant.__doc__}: {total} differing rows on {cls}"


def test_mutant_h_flips_a_decision(results):
    for c in C.cases_of("lines", "ex_reads_new_sp"):
        if c.variant == "decision":
            got, ref = mutant_h(c), results[c.name][0]
            flipped = int((got[0] != ref[0]).sum())
            assert flipped >= 1, f"ex from the original sp_r: {flipped} decisions differ on {c.name}"


def _sweep_rows(seed, n):
    """Line rows over a grid of awkward values (NaN, +-inf, +-0, ties, integers) in all eight coordinates."""
    r = np.random.Generator(np.random.PCG64(seed))
    vals = np.array([math.nan, math.inf, -math.inf, 0.0, -0.0, 1.0, 16.0, 16.0, 48.0, 48.0, 32.0, 90.0, 100.0, 0.01, 0.125], np.float32)
    f_l, f_r = vals[r.integers(0, len(vals), (n, 4))], vals[r.integers(0, len(vals), (n, 4))]
    return C.Case("sweep", "sweep", "sweep", "lines", n, np.arange(n, dtype=np.int32), f_l, f_r, None, {}, [])


@pytest.mark.parametrize("th", [C.T0, (0.0, 0.0, -0.5, -1.0), (-math.inf, -1.0, -1.0, -math.inf)])
def test_equivalent_mutants_change_no_output(results, th):
    """(g), (i) and (f) in one place at a time: no row of any case and no row of a sweep over NaN / inf / zero / tie coordinates
    changes its decision or a disparity bit (the argument is in this file's docstring)."""
    sweep = _sweep_rows(5, 6000)._replace(th=th)
    ref = C.restate(sweep)
    assert _differing_rows(ref, _oracle(sweep)) == 0
    muts = [mutant_g, mutant_i] + [_mutant_f_one(w) for w in ("ov", "l", "r")]
    for m in muts:
        assert _differing_rows(m(sweep), ref) == 0
    if th is C.T0:
        for c in C.all_cases():
            if c.kind == "lines" and c.n_l in (65, 257):
                for m in muts:
                    assert _differing_rows(m(c), results[c.name][0]) == 0, c.name


def test_overlap_function_with_a_nan_row():
    """plo_line_segment_overlap_stereo itself with a NaN right y: std::min / std::max return by operand ORDER (NaN, NaN from
    a NaN first operand; the other value twice from a NaN second one), fmin / fmax the other value twice -- and the overlap
    is 0 in every one of these, so not even the function's value tells them apart."""
    L = O.lib().plo_line_segment_overlap_stereo
    for args in ((16.0, 48.0, math.nan, 40.0, 0.1), (16.0, 48.0, 20.0, math.nan, 0.1), (16.0, 48.0, math.nan, math.nan, 0.1),
                 (math.nan, 48.0, 20.0, 40.0, 0.1), (16.0, math.nan, 20.0, 40.0, 0.1)):
        ref = L(*args)
        assert _bits([ref])[0] == _bits([C.overlap_stereo(*args)])[0]
        assert _bits([C.overlap_stereo(*args, ops=dict(C.OPS, dmin=_fmin, dmax=_fmax))])[0] == _bits([ref])[0]


def test_float_dy_cannot_drop_what_exact_dy_keeps_under_a_float_threshold():
    """Why dy_float_drops uses thresholds that are not floats: rounding to nearest is monotone, so |fl(dy)| > th with th a float
    implies |dy| > th.  Checked here on the pairs most likely to break it: a.y within a few ulps of th, b.y tiny."""
    r = np.random.Generator(np.random.PCG64(1))
    for th in (1.0, 2.5, 0.5):
        u = np.float32(th) - np.nextafter(np.float32(th), np.float32(0))
        a = (np.float32(th) + r.integers(-4, 5, 200000).astype(np.float32) * u).astype(np.float32)
        b = (r.uniform(-3, 3, 200000) * float(u)).astype(np.float32)
        fl = np.abs((a - b).astype(np.float64)) <= th
        ex = np.abs(a.astype(np.float64) - b.astype(np.float64)) <= th
        assert not (ex & ~fl).any() and (fl & ~ex).sum() > 1000


def test_descriptors_scan_to_the_table():
    """The plan paths of the device tests make the table with a scan: oracle.match over the cases' descriptors returns m12."""
    for c in C.all_cases():
        if c.cls == "index_edges":
            continue
        d_l, d_r = C.descriptors(c)
        m, n = O.match(d_l, d_r, 0.75, C.scan_mutual(c))
        assert np.array_equal(m, c.m12) and n == int((c.m12 >= 0).sum()), c.name


def test_committed_fixture_is_what_the_oracle_gives(results):
    import os
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "stereo_gate_edges.npz"))
    names = [c.name for c in C.all_cases() if c.n_l in C.FIXTURE_SIZES]
    assert sorted(g["names"].tolist()) == sorted(names)
    for c in C.all_cases():
        if c.n_l in C.FIXTURE_SIZES:
            k = c.name
            assert np.array_equal(g[k + ":m12"], c.m12) and np.array_equal(g[k + ":th"], np.array(c.th))
            assert np.array_equal(g[k + ":f_l"].view(np.uint32), c.f_l.view(np.uint32))
            assert np.array_equal(g[k + ":f_r"].view(np.uint32), c.f_r.view(np.uint32))
            ref = results[k][0]
            assert np.array_equal(g[k + ":stereo"], ref[0]) and np.array_equal(_bits(g[k + ":disp"]), _bits(ref[1]))
            assert int(g[k + ":n"]) == ref[2]
