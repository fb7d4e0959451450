"""Named inputs that put the stereo gates (plslam_amd/csrc/stereo_gates_dev.hpp: point_gate_one, overlap_stereo,
line_gate_one; specification = the oracle's restatement, oracle/plslam_oracle.c plo_stereo_point_gate / plo_stereo_line_gate)
ON their thresholds, for tests/test_stereo_gate_cases_cpu.py (which checks from the input and a Python restatement alone that
each class reaches what it is named for, and that the mutants of the restatement are told apart) and for
tests/test_gpu_stereo_gate_edges.py (the same inputs through every way the gates run on the device).  numpy only.

A case is (kind, m12, f_l, f_r, thresholds): kind "points" / "lines", f_l / f_r float32 as the ABI takes them, thresholds
doubles -- (max_dist_epip, min_disp) or (min_disp, line_horiz_th, stereo_overlap_th, ls_min_disp_ratio).  Every class is built
at n_l in SIZES with n_r = n_l + 3: ordinary rows of stereo_points / stereo_lines (made injective, so that a descriptor scan can
produce the table), the rows of interest ("specials") written over them at the start of the first wave, of a middle wave and
at the very end of the last, partly filled one (n_l = 1 holds the class's first special).  One lane per feature and one atomic per wave: larger sizes add nothing.

Point classes
  dy_float_keeps   a.y = th + 1 float ulp, b.y in (ulp/2, ulp): the exact |dy| is above th, the float one IS th; both signs
  dy_float_drops   the other direction.  Rounding to nearest is monotone, so with a threshold that is itself a float (1.0, 2.5,
                   0.5) float |dy| > th implies exact |dy| > th: no input exists.  The class uses the three thresholds just
                   under the NEXT float (th + ulp - ulp/256): exact th + ulp - ulp/64 passes, its float th + ulp does not
  dy_equal         |dy| == th at th = 0 (also +0 against -0) and th = 1, one float ulp above
  disp_equal       disparity == min_disp and one float ulp below, min_disp 1, 0 (a denormal below: -1.4e-45), -5
  index_edges      m12 = n_r, n_r - 1, -2, INT_MIN, INT_MAX, -1, 0; and n_r == 0 with no right table at all
  nan_inf_coords   NaN, +-inf in pt.y / pt.x of either side (inf disparities are kept)
Line classes (base thresholds 1.0, 0.1, 0.75, 0.7)
  horiz_th_edges   |sp_l.y - ep_l.y| = 0.125 with line_horiz_th = 0.125 and one double ulp either side.  The three fabs tests
                   all see this one value: epl - spl and spl - epl are exact negatives, and sp_r.y / ep_r.y are overwritten
                   with the left rows before the last test reads them
  length_001f      length == 0.01f, 0.01f + 1 double ulp, 0.01f + 2^-40 (between 0.01f and 0.01), above 0.01
  overlap_branches disjoint on either side, containing, partial from above and below, epn == sln, spn == eln; also with a
                   negative overlap threshold, under which overlap 0 is kept -- but not the epn == sln row: there sp_l.y ==
                   ep_r.y, and ex, which reads the overwritten sp_r.y, is 0 / 0 where sx was finite
  overlap_ratio    overlap / length exactly 1 and a float ulp below, exactly 0.75; thresholds 1.0 and 0.75.  "Just above 1" does
                   not exist: overlap is 0, eln - sln with spn < sln, or min(eln, epn) - max(sln, spn), each a rounded a - b
                   with a <= eln and b >= spn, so it is <= length = fl(eln - spn) and the clamp never fires (NaN compares false)
  disp_ratio       min / max exactly ls_min_disp_ratio (0.5, 0.7), disparities of opposite sign (ratio -0.5, filtered, and kept
                   under a ratio threshold of -1), both zero (0 / 0)
  min_disp_edges   disp_s == min_disp with disp_e equal, a float ulp of x below, above; and the reverse
  right_horizontal sp_r.y == ep_r.y under a slanted left segment: +inf, NaN; under stereo_overlap_th = -0.5 a row KEPT with
                   disparities (+inf, +inf)
  zero_length      both segments points; also under line_horiz_th = -1 (0 / 0)
  identical        left == right: disparities (0, 0), 0 / 0, kept under min_disp = 0
  ex_reads_new_sp  rows whose second disparity changes its low bits if ex is computed from the ORIGINAL sp_r, and one whose
                   decision changes (min_disp = its true disp_e)
  index_edges      as for points
"""
from __future__ import annotations

import functools
import math
from collections import namedtuple

import numpy as np

F32 = np.float32
INT_MIN, INT_MAX = -2 ** 31, 2 ** 31 - 1
SIZES = (1, 63, 64, 65, 255, 256, 257, 513)
LEN_TH_F = float(F32(0.01))                    # the literal 0.01f widened to double: 0.009999999776482582
T0 = (1.0, 0.1, 0.75, 0.7)


def _rng(seed):
    return np.random.Generator(np.random.PCG64(seed))


# ---- the ordinary rows (shared with tests/test_stereo_gates.py) ---------------------------------------------------------------
def stereo_points(seed, n_l=1500, n_r=1500, width=752, height=480):
    """Left key points, right ones displaced by a disparity along x with sub-pixel noise in y; a match table that is
    mostly right, sometimes wrong, sometimes empty."""
    r = _rng(seed)
    kp_l = np.stack([r.uniform(0, width, n_l), r.uniform(0, height, n_l)], 1).astype(np.float32)
    src = r.permutation(max(n_l, n_r))[:n_r] % max(n_l, 1)
    disp = r.uniform(-3, 60, n_r)
    kp_r = (kp_l[src] - np.stack([disp, r.normal(0, 0.8, n_r)], 1)).astype(np.float32)
    m12 = np.full(n_l, -1, np.int32)
    m12[src] = np.arange(n_r)
    wrong = r.random(n_l) < 0.1
    m12[wrong] = r.integers(0, max(n_r, 1), int(wrong.sum()))
    m12[r.random(n_l) < 0.2] = -1
    return m12, kp_l, kp_r


def stereo_lines(seed, n_l=200, n_r=200, width=752, height=480):
    r = _rng(seed)
    a = np.stack([r.uniform(0, width, n_l), r.uniform(0, height, n_l)], 1)
    ang = r.uniform(0, np.pi, n_l)
    ln = r.uniform(5, 150, n_l)
    ln[r.random(n_l) < 0.05] = 0.0                                     # zero-length segments
    ang[r.random(n_l) < 0.1] = 0.0                                     # horizontal segments (dy = 0: division by zero)
    seg_l = np.concatenate([a, a + np.stack([np.cos(ang), np.sin(ang)], 1) * ln[:, None]], 1)
    src = r.permutation(max(n_l, n_r))[:n_r] % max(n_l, 1)
    d0, d1 = r.uniform(-2, 50, n_r), r.uniform(0.5, 1.5, n_r)
    seg_r = seg_l[src].copy()
    seg_r[:, 0] -= d0
    seg_r[:, 2] -= d0 * d1
    seg_r += r.normal(0, 0.7, seg_r.shape)
    cut = r.random(n_r) < 0.3                                          # right segment only partly overlapping in y
    seg_r[cut, 2:] = seg_r[cut, :2] + (seg_r[cut, 2:] - seg_r[cut, :2]) * r.uniform(0.1, 0.9, (int(cut.sum()), 1))
    m12 = np.full(n_l, -1, np.int32)
    m12[src] = np.arange(n_r)
    wrong = r.random(n_l) < 0.1
    m12[wrong] = r.integers(0, max(n_r, 1), int(wrong.sum()))
    m12[r.random(n_l) < 0.15] = -1
    return m12, seg_l.astype(np.float32), seg_r.astype(np.float32)


# ---- the restatement: one row at a time, Python floats (IEEE doubles), every comparison logged ---------------------------------
def rel(lhs, rhs):
    """Where lhs lies against rhs: 'nan', 'eq', '+1ulp' / '-1ulp' (one double ulp above / below), 'gt', 'lt'."""
    if lhs != lhs or rhs != rhs:
        return "nan"
    if lhs == rhs:
        return "eq"
    if lhs == math.nextafter(rhs, math.inf):
        return "+1ulp"
    if lhs == math.nextafter(rhs, -math.inf):
        return "-1ulp"
    return "gt" if lhs > rhs else "lt"


def ddiv(a, b):
    """a / b in IEEE double arithmetic (Python raises on a zero divisor)."""
    if b == 0.0 and b == b:
        if a != a or a == 0.0:
            return math.nan
        return math.copysign(math.inf, a) * math.copysign(1.0, b)
    return a / b


def std_min(a, b):
    return b if b < a else a


def std_max(a, b):
    return b if a < b else a


def f32_sub(a, b):
    """The float subtraction of the source (cv::Point2f arithmetic), widened to double."""
    return float(F32(a) - F32(b))


# what a mutant replaces: tests/test_stereo_gate_cases_cpu.py passes a dict with some of these keys
OPS = dict(dy=f32_sub,                                     # (a.y, b.y) -> dy as double
           dy_le=lambda d, th: d <= th,
           disp_ge=lambda d, md, which: d >= md,           # which: "p" (points), "s" / "e" (line end points)
           len_th=LEN_TH_F,
           ov_gt=lambda o, th: o > th,
           hz_gt=lambda v, th, where: v > th,              # where: "ov" (overlap_stereo), "l", "r" (the final condition)
           dmin=std_min, dmax=std_max,
           ex_reads_new=True,
           clamp=True,
           ratio_lt=lambda r, th: r < th)


def point_row(i2, a, kp_r, n_r, th, ops=OPS, log=None):
    """plo_stereo_point_gate's loop body -> (kept index or -1, disparity)."""
    say = log.append if log is not None else (lambda t: None)
    max_dist_epip, min_disp = th
    if i2 < 0 or i2 >= n_r:
        say(("index", "none" if i2 == -1 else "below" if i2 < 0 else "n_r" if i2 == n_r else "above"))
        return -1, 0.0
    say(("index", "last" if i2 == n_r - 1 else "first" if i2 == 0 else "in"))
    b = kp_r[i2]
    dy = ops["dy"](a[1], b[1])
    exact = float(a[1]) - float(b[1])
    say(("dy", rel(abs(f32_sub(a[1], b[1])), max_dist_epip)))
    say(("dy_sign", "nan" if exact != exact else "neg" if exact < 0 else "pos"))
    fl, ex = abs(f32_sub(a[1], b[1])) <= max_dist_epip, abs(exact) <= max_dist_epip
    if fl != ex:
        say(("dy_sides", "float_keeps" if fl else "float_drops"))
    if not ops["dy_le"](abs(dy), max_dist_epip):
        return -1, 0.0
    d = f32_sub(a[0], b[0])
    say(("disp", rel(d, min_disp)))
    if d == d and not math.isinf(d) and F32(d) == np.nextafter(F32(min_disp), F32(-np.inf)):
        say(("disp", "-1ulp_f32"))
    if not ops["disp_ge"](d, min_disp, "p"):
        return -1, 0.0
    say(("kept", "inf" if math.isinf(d) else "finite"))
    return i2, d


def overlap_stereo(spl_obs, epl_obs, spl_proj, epl_proj, line_horiz_th, ops=OPS, log=None):
    """plo_line_segment_overlap_stereo."""
    say = log.append if log is not None else (lambda t: None)
    dmin, dmax = ops["dmin"], ops["dmax"]
    overlap = 1.0
    say(("hz_ov", rel(abs(epl_obs - spl_obs), line_horiz_th)))
    if ops["hz_gt"](abs(epl_obs - spl_obs), line_horiz_th, "ov"):
        sln, eln = dmin(spl_obs, epl_obs), dmax(spl_obs, epl_obs)
        spn, epn = dmin(spl_proj, epl_proj), dmax(spl_proj, epl_proj)
        length = eln - spn
        say(("epn_sln", rel(epn, sln)))
        say(("spn_eln", rel(spn, eln)))
        if epn < sln or spn > eln:
            say(("ov_branch", "disjoint_below" if epn < sln else "disjoint_above"))
            overlap = 0.0
        elif epn > eln and spn < sln:
            say(("ov_branch", "containing"))
            overlap = eln - sln
        else:
            say(("ov_branch", "partial"))
            overlap = dmin(eln, epn) - dmax(sln, spn)
        say(("length", rel(length, LEN_TH_F)))
        if LEN_TH_F < length < 0.01:
            say(("length", "between"))
        if length > ops["len_th"]:
            overlap = ddiv(overlap, length)
        else:
            overlap = 0.0
        say(("ov_ratio", rel(overlap, 1.0)))
        if overlap > 1.0:
            say(("clamp", "taken"))
            if ops["clamp"]:
                overlap = 1.0
    return overlap


def line_row(i2, L, seg_r, n_r, th, ops=OPS, log=None):
    """plo_stereo_line_gate's loop body -> (kept index or -1, disp_s, disp_e)."""
    say = log.append if log is not None else (lambda t: None)
    min_disp, line_horiz_th, stereo_overlap_th, ls_min_disp_ratio = th
    if i2 < 0 or i2 >= n_r:
        say(("index", "none" if i2 == -1 else "below" if i2 < 0 else "n_r" if i2 == n_r else "above"))
        return -1, 0.0, 0.0
    say(("index", "last" if i2 == n_r - 1 else "first" if i2 == 0 else "in"))
    R = seg_r[i2]
    sp_l, ep_l = (float(L[0]), float(L[1])), (float(L[2]), float(L[3]))
    sp_r, ep_r = [float(R[0]), float(R[1])], [float(R[2]), float(R[3])]
    if sp_l == ep_l and sp_r == ep_r:
        say(("shape", "both_points"))
    if (sp_l, ep_l) == (tuple(sp_r), tuple(ep_r)):
        say(("shape", "identical"))
    overlap = overlap_stereo(sp_l[1], ep_l[1], sp_r[1], ep_r[1], line_horiz_th, ops, log)
    den = sp_r[1] - ep_r[1]
    sx = ddiv(sp_r[0] * (sp_l[1] - ep_r[1]) + ep_r[0] * (sp_r[1] - sp_l[1]), den)
    if den == 0.0 and abs(sp_l[1] - ep_l[1]) > 0.0:
        say(("right_horizontal", "nan" if sx != sx else "inf"))
    ex_old = ddiv(sp_r[0] * (ep_l[1] - ep_r[1]) + ep_r[0] * (sp_r[1] - ep_l[1]), den)      # from the ORIGINAL sp_r
    sp_r = [sx, sp_l[1]]
    ex_new = ddiv(sp_r[0] * (ep_l[1] - ep_r[1]) + ep_r[0] * (sp_r[1] - ep_l[1]), sp_r[1] - ep_r[1])
    if den != 0.0 and sp_r[1] - ep_r[1] == 0.0:
        say(("second_den", "0"))                           # sp_l.y == ep_r.y: only the second formula divides by zero
    if ex_new == ex_new and ex_old == ex_old and ex_new != ex_old:
        say(("ex_dep", "bits"))
    ex = ex_new if ops["ex_reads_new"] else ex_old
    ep_r = [ex, ep_l[1]]
    disp_s, disp_e = sp_l[0] - sp_r[0], ep_l[0] - ep_r[0]
    ratio = ddiv(ops["dmin"](disp_s, disp_e), ops["dmax"](disp_s, disp_e))
    say(("disp_ratio", rel(ratio, ls_min_disp_ratio)))
    if disp_s == 0.0 and disp_e == 0.0:
        say(("disp_ratio", "0/0"))
    if ratio < 0.0:
        say(("disp_ratio", "negative"))
    if ops["ratio_lt"](ratio, ls_min_disp_ratio):
        disp_s = disp_e = -1.0
    else:
        say(("disp_s", rel(disp_s, min_disp)))
        say(("disp_e", rel(disp_e, min_disp)))
        if ops["ex_reads_new"] and ex_old == ex_old and (ep_l[0] - ex_old >= min_disp) != (disp_e >= min_disp):
            say(("ex_dep", "decision"))
    say(("hz_l", rel(abs(sp_l[1] - ep_l[1]), line_horiz_th)))
    say(("hz_r", rel(abs(sp_r[1] - ep_r[1]), line_horiz_th)))
    say(("ov", rel(overlap, stereo_overlap_th)))
    if (ops["disp_ge"](disp_s, min_disp, "s") and ops["disp_ge"](disp_e, min_disp, "e") and
            ops["hz_gt"](abs(sp_l[1] - ep_l[1]), line_horiz_th, "l") and ops["hz_gt"](abs(sp_r[1] - ep_r[1]), line_horiz_th, "r") and
            ops["ov_gt"](overlap, stereo_overlap_th)):
        say(("kept", "inf" if math.isinf(disp_s) or math.isinf(disp_e) else "finite"))
        return i2, disp_s, disp_e
    return -1, 0.0, 0.0


def restate(case, ops=None, logs=None):
    """The whole case through the restatement -> (stereo_12, disp, n) shaped as the oracle's.  ops: replacements for entries of
    OPS (a mutant); logs: a list that receives one list of (comparison, outcome) per row."""
    o = dict(OPS)
    o.update(ops or {})
    n_l, n_r = case.m12.shape[0], case.f_r.shape[0]
    lines = case.kind == "lines"
    out = np.full(n_l, -1, np.int32)
    disp = np.zeros((n_l, 2) if lines else n_l, np.float64)
    f_l, f_r = case.f_l.tolist(), case.f_r.tolist()             # float32 values as Python floats: exact
    with np.errstate(all="ignore"):
        for i1 in range(n_l):
            lg = [] if logs is not None else None
            if lines:
                k, ds, de = line_row(int(case.m12[i1]), f_l[i1], f_r, n_r, case.th, o, lg)
                disp[i1] = (ds, de)
            else:
                k, d = point_row(int(case.m12[i1]), f_l[i1], f_r, n_r, case.th, o, lg)
                disp[i1] = d
            out[i1] = k
            if logs is not None:
                logs.append(lg)
    return out, disp, int((out >= 0).sum())


# ---- the classes -------------------------------------------------------------------------------------------------------------
def _up(x, k=1):
    x = F32(x)
    for _ in range(k):
        x = np.nextafter(x, F32(np.inf))
    return float(x)


def _ulp32(x):
    return _up(x) - float(F32(x))


# a special row: (left feature, right feature, tags its log must hold, kept?, m12 override or None)
def S(fl, fr, tags, kept, m=None):
    return (tuple(fl), tuple(fr), frozenset(tags), kept, m)


def _dy_keeps(th):
    u = _ulp32(th)
    rows = []
    for frac in (0.75, 0.515625, 0.984375):
        hi, lo = _up(th), frac * u
        rows.append(S((100.0, hi), (90.0, lo), {("dy_sides", "float_keeps"), ("dy", "eq"), ("dy_sign", "pos"), ("kept", "finite")}, True))
        rows.append(S((100.0, lo), (90.0, hi), {("dy_sides", "float_keeps"), ("dy", "eq"), ("dy_sign", "neg"), ("kept", "finite")}, True))
    return (th, 1.0), rows


def _dy_drops(th):
    u = _ulp32(th)
    th2 = th + u - u / 256                                    # a double just under the float above th
    hi, lo = _up(th, 2), u + u / 64
    rows = [S((100.0, hi), (90.0, lo), {("dy_sides", "float_drops"), ("dy_sign", "pos")}, False),
            S((100.0, lo), (90.0, hi), {("dy_sides", "float_drops"), ("dy_sign", "neg")}, False),
            S((100.0, _up(th)), (90.0, 0.0), {("dy", "gt")}, False),
            S((100.0, th), (90.0, 0.0), {("dy", "lt"), ("kept", "finite")}, True)]
    return (th2, 1.0), rows


def _point_classes():
    c = {}
    c["dy_float_keeps"] = {f"th{t}": _dy_keeps(t) for t in (1.0, 2.5, 0.5)}
    c["dy_float_drops"] = {f"under{t}": _dy_drops(t) for t in (1.0, 2.5, 0.5)}
    k, d = {("kept", "finite")}, set()
    c["dy_equal"] = {
        "th0": ((0.0, 1.0), [S((100, 123.25), (90, 123.25), {("dy", "eq")} | k, True),
                             S((100, 0.0), (90, -0.0), {("dy", "eq")} | k, True),
                             S((100, -0.0), (90, 0.0), {("dy", "eq")} | k, True),
                             S((100, 1e-45), (90, 0.0), {("dy", "gt")}, False),             # one denormal above 0
                             S((100, 123.25), (90, _up(123.25)), {("dy", "gt"), ("dy_sign", "neg")}, False)]),
        "th1": ((1.0, 1.0), [S((100, 51.0), (90, 50.0), {("dy", "eq"), ("dy_sign", "pos")} | k, True),
                             S((100, 50.0), (90, 51.0), {("dy", "eq"), ("dy_sign", "neg")} | k, True),
                             S((100, _up(51.0)), (90, 50.0), {("dy", "gt")}, False),
                             S((100, 50.0), (90, _up(51.0)), {("dy", "gt")}, False),
                             S((100, 3.0), (90, 2.0), {("dy", "eq")} | k, True)])}
    c["disp_equal"] = {
        "md1": ((1.0, 1.0), [S((100, 50), (99, 50), {("disp", "eq")} | k, True),
                             S((100, 50), (_up(99), 50), {("disp", "lt")}, False),
                             S((2.0, 50), (1.0, 50.5), {("disp", "eq")} | k, True),
                             S((1.5, 50), (_up(0.5), 50), {("disp", "-1ulp_f32")}, False)]),       # 1 - 2^-24
        "md0": ((1.0, 0.0), [S((100, 50), (100, 50), {("disp", "eq")} | k, True),
                             S((0.0, 50), (1e-45, 50), {("disp", "-1ulp_f32")}, False),     # -1.4e-45: a denormal float
                             S((100, 50), (_up(100), 50), {("disp", "lt")}, False),
                             S((-0.0, 50), (0.0, 50), {("disp", "eq")} | k, True)]),          # -0 >= 0
        "md-5": ((1.0, -5.0), [S((95, 50), (100, 50), {("disp", "eq")} | k, True),
                               S((95, 50), (_up(100), 50), {("disp", "lt")}, False),
                               S((1.0, 50), (6.0, 50), {("disp", "eq")} | k, True),
                               S((1.0, 50), (_up(6.0), 50), {("disp", "-1ulp_f32")}, False)])}
    good = ((100.0, 50.0), (90.0, 50.5))
    c["index_edges"] = {
        "edges": ((1.0, 1.0), [S(*good, {("index", "n_r")}, False, "n_r"), S(*good, {("index", "last")} | k, True, "n_r-1"),
                               S(*good, {("index", "below")}, False, -2), S(*good, {("index", "below")}, False, INT_MIN),
                               S(*good, {("index", "above")}, False, INT_MAX), S(*good, {("index", "none")}, False, -1),
                               S(*good, {("index", "first")} | k, True, 0)]),
        "empty_right": ((1.0, 1.0), [S(*good, {("index", "n_r")}, False, 0), S(*good, {("index", "none")}, False, -1),
                                     S(*good, {("index", "above")}, False, 5), S(*good, {("index", "above")}, False, INT_MAX),
                                     S(*good, {("index", "below")}, False, INT_MIN)])}
    nan, inf = math.nan, math.inf
    c["nan_inf_coords"] = {"kitti": ((1.0, 1.0), [
        S((100, nan), (90, 50), {("dy", "nan")}, False), S((100, 50), (90, nan), {("dy", "nan")}, False),
        S((100, inf), (90, 50), {("dy", "gt")}, False), S((100, inf), (90, inf), {("dy", "nan")}, False),
        S((100, -inf), (90, inf), {("dy", "gt")}, False), S((100, 50), (90, -inf), {("dy", "gt")}, False),
        S((nan, 50), (90, 50.5), {("disp", "nan")}, False), S((100, 50), (nan, 50.5), {("disp", "nan")}, False),
        S((inf, 50), (90, 50.5), {("kept", "inf")}, True), S((100, 50), (-inf, 50.5), {("kept", "inf")}, True),
        S((-inf, 50), (90, 50.5), {("disp", "lt")}, False), S((100, 50), (inf, 50.5), {("disp", "lt")}, False),
        S((inf, 50), (inf, 50.5), {("disp", "nan")}, False)])}
    return c


def _ex_rows():
    """Seeded search: kept rows whose disp_e changes its low bits when ex reads the original sp_r; the first one has the
    mutant's value BELOW the true one, so that min_disp = the true value flips its decision."""
    r = _rng(4242)
    th = (1.0, 0.1, 0.2, 0.3)
    rows, first = [], None
    while len(rows) < 4 or first is None:
        a = r.uniform(20, 400, 2)
        ang, ln = r.uniform(0.5, 2.6), r.uniform(20, 120)
        L = np.array([a[0], a[1], a[0] + math.cos(ang) * ln, a[1] + math.sin(ang) * ln], np.float32)
        R = (L - np.array([r.uniform(5, 40), r.normal(0, 0.7), r.uniform(5, 40), r.normal(0, 0.7)])).astype(np.float32)
        lg = []
        k, ds, de = line_row(0, L.tolist(), [R.tolist()], 1, th, OPS, lg)
        km, dsm, dem = line_row(0, L.tolist(), [R.tolist()], 1, th, dict(OPS, ex_reads_new=False))
        if k < 0 or km < 0 or ("ex_dep", "bits") not in lg:
            continue
        if first is None and dem < de:
            first = (L, R, de)
        elif len(rows) < 4:
            rows.append(S(L, R, {("ex_dep", "bits"), ("kept", "finite")}, True))
    L, R, de = first
    bits = (th, [S(L, R, {("ex_dep", "bits"), ("kept", "finite")}, True)] + rows)
    dec = ((de, 0.1, 0.2, 0.3), [S(L, R, {("ex_dep", "decision"), ("disp_e", "eq"), ("kept", "finite")}, True)] + [S(x[0], x[1], {("ex_dep", "bits")}, None) for x in rows])
    return {"bits": bits, "decision": dec}


def _line_classes():
    c = {}
    k = {("kept", "finite")}
    Lb = (100, 16, 100, 48)
    hzr = [((100, 16, 100, 16.125), (90, 16, 90, 16.125)), ((100, 16.125, 100, 16), (90, 16.125, 90, 16)),
           ((300, 200.125, 310, 200), (280, 200.125, 290, 200))]
    D = 0.125

    def hz(th, r, kept):
        t = {("hz_ov", r), ("hz_l", r), ("hz_r", r)} | (k if kept else set())
        return ((1.0, th, 0.75, 0.7), [S(a, b, t, kept) for a, b in hzr] + [S(Lb, (90, 16, 90, 48), {("hz_l", "gt")} | k, True)])
    c["horiz_th_edges"] = {"eq": hz(D, "eq", False), "th_below": hz(math.nextafter(D, 0.0), "+1ulp", True),
                           "th_above": hz(math.nextafter(D, 1.0), "-1ulp", False)}
    f01 = LEN_TH_F
    Ll = (100, 0, 100, f01)
    c["length_001f"] = {"f01": ((1.0, 0.001, 0.2, 0.7), [
        S(Ll, (90, -2.0 ** -40, 90, 0.005), {("length", "between")} | k, True),
        S(Ll, (90, 0, 90, 0.005), {("length", "eq")}, False),
        S(Ll, (90, -2.0 ** -59, 90, 0.005), {("length", "+1ulp")} | k, True),
        S(Ll, (90, -2.0 ** -30, 90, 0.005), {("length", "gt")} | k, True),
        S(Ll, (90, 2.0 ** -40, 90, 0.005), {("length", "lt")}, False)])}
    br = [(S(Lb, (90, 50, 90, 60), {("ov_branch", "disjoint_above")}, False), True),
          (S(Lb, (90, 2, 90, 10), {("ov_branch", "disjoint_below")}, False), True),
          (S(Lb, (90, 8, 90, 56), {("ov_branch", "containing")} | k, True), True),
          (S(Lb, (90, 32, 90, 64), {("ov_branch", "partial"), ("ov_ratio", "eq")} | k, True), True),
          (S(Lb, (90, 8, 90, 32), {("ov_branch", "partial"), ("ov_ratio", "lt")} | k, True), True),
          (S(Lb, (90, 56, 90, 8), {("ov_branch", "containing")} | k, True), True),           # the right segment upside down
          (S(Lb, (90, 8, 90, 16), {("epn_sln", "eq"), ("ov_branch", "partial")}, False), False),
          (S(Lb, (90, 48, 90, 64), {("spn_eln", "eq"), ("ov_branch", "partial")}, False), True)]
    c["overlap_branches"] = {"kitti": ((1.0, 0.1, 0.2, 0.7), [s for s, _ in br]),
                             "neg_ov": ((1.0, 0.1, -0.5, 0.7), [S(s[0], s[1], s[2] | (k if kp else {("second_den", "0")}), kp) for s, kp in br])}
    ovr = [((Lb, (90, 16, 90, 48)), "eq", 1.0), (((100, 16, 100, 46), (90, 6, 90, 50)), "lt", 0.75),
           ((Lb, (90, float(np.nextafter(F32(16), F32(0))), 90, 48)), "lt", None), ((Lb, (90, 16, 90, 80)), "eq", 1.0)]
    c["overlap_ratio"] = {
        "th1": ((1.0, 0.1, 1.0, 0.7), [S(a, b, {("ov_ratio", r)} | ({("ov", "eq")} if v == 1.0 else set()), False) for (a, b), r, v in ovr]),
        "th075": ((1.0, 0.1, 0.75, 0.7), [S(a, b, {("ov_ratio", r)} | ({("ov", "eq")} if v == 0.75 else k), v != 0.75)
                                          for (a, b), r, v in [ovr[1], ovr[0]] + ovr[2:]])}
    c["disp_ratio"] = {
        "r05": ((1.0, 0.1, 0.75, 0.5), [S(Lb, (90, 16, 95, 48), {("disp_ratio", "eq")} | k, True),
                                        S(Lb, (95, 16, 90, 48), {("disp_ratio", "eq")} | k, True),
                                        S(Lb, (90, 16, 105, 48), {("disp_ratio", "negative")}, False),
                                        S(Lb, (90, 16, _up(95), 48), {("disp_ratio", "lt")}, False)]),
        "r07": ((1.0, 0.1, 0.75, 0.7), [S(Lb, (90, 16, 93, 48), {("disp_ratio", "eq")} | k, True),
                                        S(Lb, (93, 16, 90, 48), {("disp_ratio", "eq")} | k, True),
                                        S(Lb, (90, 16, _up(93), 48), {("disp_ratio", "lt")}, False)]),
        "neg": ((-10.0, 0.1, 0.75, -1.0), [S(Lb, (105, 16, 95, 48), {("disp_ratio", "eq")} | k, True),          # -5 / 5 = -1
                                           S(Lb, (90, 16, 105, 48), {("disp_ratio", "negative"), ("disp_ratio", "gt")} | k, True),
                                           S(Lb, (105, 16, 90, 48), {("disp_ratio", "negative")} | k, True)]),
        "zero": ((0.0, 0.1, 0.75, 0.7), [S(Lb, (100, 16, 100, 48), {("disp_ratio", "0/0"), ("disp_ratio", "nan"), ("disp_s", "eq")} | k, True),
                                         S((-0.0, 16, 0.0, 48), (0.0, 16, 0.0, 48), {("disp_ratio", "0/0")} | k, True)])}
    c["min_disp_edges"] = {"md1": ((1.0, 0.1, 0.75, 0.3), [
        S(Lb, (99, 16, 99, 48), {("disp_s", "eq"), ("disp_e", "eq")} | k, True),
        S(Lb, (99, 16, _up(99), 48), {("disp_s", "eq"), ("disp_e", "lt")}, False),
        S(Lb, (_up(99), 16, 99, 48), {("disp_s", "lt"), ("disp_e", "eq")}, False),
        S(Lb, (99, 16, 98, 48), {("disp_s", "eq"), ("disp_e", "gt")} | k, True),
        S(Lb, (98, 16, 99, 48), {("disp_s", "gt"), ("disp_e", "eq")} | k, True)])}
    c["right_horizontal"] = {
        "kitti": (T0, [S(Lb, (90, 32, 95, 32), {("right_horizontal", "inf")}, False),
                       S(Lb, (90, 32, 90, 32), {("right_horizontal", "nan")}, False),
                       S(Lb, (95, 64, 90, 64), {("right_horizontal", "inf")}, False)]),
        "neg_ov": ((1.0, 0.1, -0.5, 0.7), [S(Lb, (95, 64, 90, 64), {("right_horizontal", "inf"), ("kept", "inf")}, True),
                                           S(Lb, (90, 0, 95, 0), {("right_horizontal", "inf"), ("kept", "inf")}, True),
                                           S(Lb, (90, 32, 95, 32), {("right_horizontal", "inf")}, False),
                                           S(Lb, (90, 64, 90, 64), {("right_horizontal", "nan")}, False)])}
    zl = [((100, 20, 100, 20), (90, 20, 90, 20)), ((100, 20, 100, 20), (90, 25, 90, 25)), ((0, 0, 0, 0), (0, 0, 0, 0))]
    c["zero_length"] = {"kitti": (T0, [S(a, b, {("shape", "both_points"), ("hz_l", "lt")}, False) for a, b in zl]),
                        "neg_hz": ((1.0, -1.0, -1.0, 0.7), [S(a, b, {("shape", "both_points"), ("hz_l", "gt")}, False) for a, b in zl])}
    idn = [(100, 16, 120, 48), (100, 16, 100, 48), (33.25, 400, 17.5, 100)]
    c["identical"] = {"md0": ((0.0, 0.1, 0.75, 0.7), [S(a, a, {("shape", "identical"), ("disp_ratio", "0/0")} | k, True) for a in idn]),
                      "md1": (T0, [S(a, a, {("shape", "identical"), ("disp_ratio", "0/0")}, False) for a in idn])}
    c["ex_reads_new_sp"] = _ex_rows()
    good = (Lb, (90, 16, 90, 48))
    c["index_edges"] = {
        "edges": (T0, [S(*good, {("index", "n_r")}, False, "n_r"), S(*good, {("index", "last")} | k, True, "n_r-1"),
                       S(*good, {("index", "below")}, False, -2), S(*good, {("index", "below")}, False, INT_MIN),
                       S(*good, {("index", "above")}, False, INT_MAX), S(*good, {("index", "none")}, False, -1),
                       S(*good, {("index", "first")} | k, True, 0)]),
        "empty_right": (T0, [S(*good, {("index", "n_r")}, False, 0), S(*good, {("index", "none")}, False, -1),
                             S(*good, {("index", "above")}, False, 5), S(*good, {("index", "above")}, False, INT_MAX),
                             S(*good, {("index", "below")}, False, INT_MIN)])}
    return c


Case = namedtuple("Case", "name cls variant kind n_l m12 f_l f_r th rows specials")
# rows: {left row -> index into specials}; specials: the class's (f_l, f_r, tags, kept, m12 override) list


def _build(kind, cls, variant, th, specials, n_l, seed):
    n_r = n_l + 3
    m12, f_l, f_r = (stereo_points if kind == "points" else stereo_lines)(seed, n_l, n_r)
    m12, f_l, f_r = m12.copy(), f_l.copy(), f_r.copy()
    K = len(specials)
    rows = {}
    # first wave, a middle wave, the end of the last wave -- there rotated so that the launch's LAST lane holds a kept row
    jk = max([j for j in range(K) if specials[j][3]], default=K - 1)
    for s0, first in ((0, 0), (64 * (((n_l + 63) // 64) // 2), 0), (n_l - K, jk + 1)) if n_l > 1 else ((0, 0),):
        for t in range(K):
            if 0 <= s0 + t < n_l:
                rows[s0 + t] = (first + t) % K
    index_class = cls == "index_edges"
    if not index_class:                                               # injective on its matched rows: a scan can produce it
        m12[list(rows)] = -1
        seen = set()
        for i in range(n_l):
            if m12[i] >= 0:
                if int(m12[i]) in seen:
                    m12[i] = -1
                seen.add(int(m12[i]))
        free = sorted(set(range(n_r)) - seen)
        _rng(seed + 1).shuffle(free)
    for p, j in sorted(rows.items()):
        fl, fr, _, _, m = specials[j]
        f_l[p] = fl
        if index_class:
            i2 = {"n_r": n_r, "n_r-1": n_r - 1}.get(m, m)
            if variant == "empty_right" and m == 0:
                i2 = 0
        else:
            i2 = free.pop()
        m12[p] = i2
        if 0 <= i2 < n_r:
            f_r[i2] = fr
    if variant == "empty_right":
        f_r = f_r[:0]
    return Case(f"{kind}/{cls}/{variant}/{n_l}", cls, variant, kind, n_l, m12, f_l, f_r, tuple(float(t) for t in th), rows, specials)


@functools.lru_cache(maxsize=None)
def all_cases():
    """Every class x variant x size, in a fixed order."""
    out = []
    for kind, classes in (("points", _point_classes()), ("lines", _line_classes())):
        for ci, (cls, variants) in enumerate(classes.items()):
            for vi, (variant, (th, specials)) in enumerate(variants.items()):
                for n_l in SIZES:
                    out.append(_build(kind, cls, variant, th, specials, n_l, 1000 * (ci + 1) + 37 * vi + n_l + (50000 if kind == "lines" else 0)))
    return tuple(out)


def classes():
    """[(kind, class name)] in order."""
    seen = []
    for c in all_cases():
        if (c.kind, c.cls) not in seen:
            seen.append((c.kind, c.cls))
    return seen


def cases_of(kind, cls):
    return [c for c in all_cases() if c.kind == kind and c.cls == cls]


def case_args(c):
    """What oracle.stereo_*_gate / Context.stereo_*_gate take."""
    return (c.m12, c.f_l, c.f_r) + c.th


FIXTURE_SIZES = (65, 257)                       # the sizes kept in tests/golden/stereo_gate_edges.npz


def descriptors(c, seed=0):
    """Distinct random 256-bit rows with d_r[m12[i]] = d_l[i] on the matched rows and fresh rows everywhere else: a mutual
    ratio-test scan of (d_l, d_r) returns exactly m12 (checked against oracle.match by the callers).  Not at n_l = 1: the
    column's consistency check has no second row to compare with and accepts nothing, so that size scans without it
    (scan_mutual)."""
    r = _rng(9000 + seed + c.n_l)
    n_r = c.f_r.shape[0]
    d_l = r.integers(0, 256, (c.n_l, 32), dtype=np.uint8)
    d_r = r.integers(0, 256, (n_r, 32), dtype=np.uint8)
    ok = c.m12 >= 0
    d_r[c.m12[ok]] = d_l[ok]
    return d_l, d_r


def scan_mutual(c):
    return c.n_l > 1
