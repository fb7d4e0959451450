"""Named inputs that put the map<->keyframe visibility pre-filter and gates (plslam_amd/csrc/map2kf_kernels.hip: inside(), k_visible,
k_visible_compact, K5 k_point_gate, K6 k_line_gate; specification = the oracle's restatement, oracle/plslam_oracle.c inside /
plo_map2kf_point_gate / plo_map2kf_line_gate, of src/mapHandler.cpp:549-551, :650-655, :601-613, :716-729) ON their
thresholds, for tests/test_map_gate_cases_cpu.py (which checks from the input and a Python restatement alone that each class
holds what it is named for, and that the mutants of the restatement are told apart) and for tests/test_gpu_map_gate_edges.py
(the same inputs through every way the code runs on the device).  numpy only.

A case is a local map of n landmarks (points n x 3, lines n x 6: start and end point) seen through a pose Twf, their candidate
flags, n + 3 keyframe features (points: the pixel pl; lines: the line equation le, and the segment the windowed matcher files)
of which three already carry a landmark (kf_idx != -1), the intended match m12 (landmark -> feature, injective unless the
class says otherwise) and the gate threshold.  Every class is built at n in SIZES under the two POSES: ordinary rows drawn as
test_gates_and_visibility_bit_exact draws them, the rows of interest ("specials") written over them at the start of the first
wave, of a middle wave and at the very end of the last, partly filled one (n = 1 holds the class's first special).  One lane
per landmark, 256-lane workgroups, a tile of 256 in k_visible_compact: larger sizes add nothing.  Boundary inputs are FOUND,
by walking one landmark coordinate over its nextafter neighbours under the restatement below; the builder raises when a class
finds none.

Visibility classes (points; lines with either end point as the special one, the other well inside)
  u_zero u_width v_zero v_height   the projected coordinate exactly on the bound (rejected), the neighbouring landmark one ulp
                    inside (kept) and the one one ulp outside (rejected)
  depth_zero        Pf.z == +0 with u = +inf, -inf, NaN; Pf.z == -0 (a pose whose translation is -0: identity only); Pf.z the
                    smallest positive denormal with X = Y = 0, so (u, v) = (cx, cy): kept (identity only); under the second pose
                    the landmarks whose Pf.z is exactly 0 and their neighbours one ulp of Z in front and behind
  behind_mirrored   z < 0 with (u, v) inside the image: only Pf(2) > 0 rejects it
  nan_inf_coords    NaN, +inf, -inf in each landmark coordinate
  line_one_end      (lines) one end well inside, the other on each of the four bounds, behind, at depth zero; both orders
  candidate_flags   flags 0, 1, 2, 255 on landmarks well inside (the code tests != 0); only the drivers take flags
  compaction_shapes all visible; none (no flag set / every landmark behind the camera); survivors only in the last workgroup;
                    only in the first; exactly one per workgroup
Window-centre classes (the fast drivers, run with a window of the cell itself)
  cell_boundary     u * inv_width exactly an integer k: cell k; the landmark one ulp of X below: cell k - 1; the same for v; a
                    projection one ulp inside the right / bottom border.  Each landmark's feature lies in the middle of ITS cell
  line_in_one_cell  (lines) both end points truncate to one cell: the direction between the integer cells is 0 / 0
Gate classes
  epip_equal        points: ey == 0, |ex| == th and ex == 0, |ey| == th for th 1.0 and 2.5, the 3-4-5 triple for th = 5.0 --
                    rejected; the same rows under th one double ulp up (error one ulp below th: kept) and down (rejected).
                    lines: e0 == th with e1 below, the reverse, both equal; under th one ulp up all three are kept
  signed_line_error (lines) e0 = -1000 with e1 below th: kept (the test is signed); e0 below th with e1 = +1000: rejected
  threshold_values  th = 0, -1, +inf, NaN.  Points: nothing passes under 0 or -1; lines: a row with both errors -2 passes under
                    -1; under +inf every finite error passes and a NaN error does not; under NaN nothing passes
  index_edges       m12 = -1, -2, INT_MIN, 0, n_kf - 1 (lone gate calls only: a scan never produces them)
  gate_no_depth_test  a matched landmark BEHIND the camera whose mirrored projection lies within th of its feature: kept by the
                    gate (the reference has no depth test there); one at depth zero: NaN error, rejected (lone gate calls only)
  association       ordinary rows and a few specials under th = 1.0, and under a threshold nothing passes (count 0)
"""
from __future__ import annotations

import functools
import math
from collections import namedtuple

import numpy as np

from plslam_amd import synth
from stereo_gate_cases import INT_MIN, SIZES, ddiv, rel

K = synth.EUROC
FX, FY, CX, CY = (float(K[k]) for k in ("fx", "fy", "cx", "cy"))
W, H = float(K["width"]), float(K["height"])
NAN, INF = math.nan, math.inf


def _rng(seed):
    return np.random.Generator(np.random.PCG64(seed))


def _pose(name):
    if name == "identity":
        return np.eye(4)
    if name == "identity_neg0":                      # the identity with a translation of -0: the only way to a Pf.z of -0
        T = np.eye(4)
        T[:3, 3] = -0.0
        return T
    return np.linalg.inv(synth.se3_exp([0.1, -0.05, 0.3, 0.01, 0.02, -0.01]))     # test_gates_and_visibility_bit_exact's


POSES = ("identity", "moved")


# ---- the restatement: one row at a time, Python floats (IEEE doubles), the kernels' operation order, every comparison logged ----
def xform(T, X):
    """(T[4i] x + T[4i+1] y + T[4i+2] z) + T[4i+3] -- se3_dev.hpp xform / xform44."""
    x, y, z = X
    return [(T[4 * i] * x + T[4 * i + 1] * y + T[4 * i + 2] * z) + T[4 * i + 3] for i in range(3)]


def project(P):
    return CX + ddiv(FX * P[0], P[2]), CY + ddiv(FY * P[1], P[2])


# what a mutant replaces
OPS = dict(u_lo=lambda u: u > 0, u_hi=lambda u: u < W, v_lo=lambda v: v > 0, v_hi=lambda v: v < H, depth=lambda z: z > 0.0,
           pt_lt=lambda e, th: e < th, ln_lt=lambda e, th: e < th, ln_err=lambda e: e, ln_both=lambda a, b: a and b,
           cell=lambda x: cvtt(x))


def inside(P, ops=OPS, log=None, end=""):
    say = log.append if log is not None else (lambda t: None)
    u, v = project(P)
    say((end + "u_lo", rel(u, 0.0)))
    say((end + "u_hi", rel(u, W)))
    say((end + "v_lo", rel(v, 0.0)))
    say((end + "v_hi", rel(v, H)))
    say((end + "depth", rel(P[2], 0.0)))
    if P[2] == 0.0:
        say((end + "depth_sign", "neg" if math.copysign(1.0, P[2]) < 0 else "pos"))
    if 0.0 < P[2] < 2.3e-308:
        say((end + "depth", "denormal"))
    if math.isinf(u) or math.isinf(v):
        say((end + "uv", "inf"))
    ok = ops["u_lo"](u) and ops["u_hi"](u) and ops["v_lo"](v) and ops["v_hi"](v) and ops["depth"](P[2])
    say((end + "inside", int(bool(ok))))
    return bool(ok)


INV_W, INV_H = 64 / W, 48 / H                       # the shipped grid: 64 x 48 cells over the image (fast_cfg)


def cvtt(v):
    """double -> int as the reference's build converts (cvttsd2si): truncation toward zero; NaN / out of range -> INT_MIN."""
    return int(v) if v == v and -2147483649.0 < v < 2147483648.0 else INT_MIN


def cells_row(kind, T, lm, ops=OPS, log=None):
    """pj_points / pj_lines (:554, :658) as k_project_cells / k_prepare_rows compute them: the cell of each projected end, and
    for a line the direction between the two INTEGER cells -> (cells, direction or None)."""
    say = log.append if log is not None else (lambda t: None)
    out = []
    for end, X in ((("", lm),) if kind == "points" else (("s.", lm[:3]), ("e.", lm[3:]))):
        u, v = project(xform(T, X))
        a, b = u * INV_W, v * INV_H
        for name, x in (("cell_u", a), ("cell_v", b)):
            if x == x and not math.isinf(x) and abs(x) < 1e9:
                say((end + name, rel(x, float(round(x)))))
        cell = (ops["cell"](a), ops["cell"](b))
        say((end + "cell", cell))
        out.append(cell)
    if kind == "points":
        return out, None
    vx, vy = float(out[1][0]) - float(out[0][0]), float(out[1][1]) - float(out[0][1])
    mag = math.sqrt(vx * vx + vy * vy)
    d = (ddiv(vx, mag), ddiv(vy, mag))
    say(("dir", "nan" if d[0] != d[0] else "unit"))
    return out, d


def vis_row(kind, T, lm, ops=OPS, log=None):
    """inside() of the point, or of both end points of the line."""
    if kind == "points":
        return int(inside(xform(T, lm), ops, log))
    a = inside(xform(T, lm[:3]), ops, log, "s.")
    b = inside(xform(T, lm[3:]), ops, log, "e.")
    return int(a and b)


def gate_row(kind, T, lm, i2, feat, th, ops=OPS, log=None):
    """The body of K5 / K6 for one row: 1 when the landmark keeps feature i2."""
    say = log.append if log is not None else (lambda t: None)
    if i2 < 0:
        say(("index", "none" if i2 == -1 else "below"))
        return 0
    say(("index", "first" if i2 == 0 else "last" if i2 == len(feat) - 1 else "in"))
    f = feat[i2]
    if kind == "points":
        Pf = xform(T, lm)
        u, v = project(Pf)
        ex, ey = u - f[0], v - f[1]
        err = math.sqrt(ex * ex + ey * ey)
        say(("err", rel(err, th)))
        say(("depth", rel(Pf[2], 0.0)))
        ok = ops["pt_lt"](err, th)
    else:
        sP, eP = xform(T, lm[:3]), xform(T, lm[3:])
        su, sv = project(sP)
        eu, ev = project(eP)
        e0 = f[0] * su + f[1] * sv + f[2]
        e1 = f[0] * eu + f[1] * ev + f[2]
        say(("e0", rel(e0, th)))
        say(("e1", rel(e1, th)))
        if e0 < 0 or e1 < 0:
            say(("sign", "neg"))
        say(("depth", rel(sP[2], 0.0)))
        e0, e1 = ops["ln_err"](e0), ops["ln_err"](e1)
        ok = ops["ln_both"](ops["ln_lt"](e0, th), ops["ln_lt"](e1, th))
    say(("kept", int(bool(ok))))
    return int(bool(ok))


# ---- finding the inputs ---------------------------------------------------------------------------------------------------------
def _T(pose):
    return [float(x) for x in _pose(pose).reshape(16)]


def _world(pose, pc):
    Tfw = np.linalg.inv(_pose(pose))
    w = Tfw[:3, :3] @ np.asarray(pc, float) + Tfw[:3, 3]
    return [float(x) for x in w]


def _at(pose, u, v, z):
    """A landmark that projects (nearly) to (u, v) at depth z; z < 0: behind the camera, mirrored."""
    return tuple(_world(pose, ((u - CX) / FX * z, (v - CY) / FY * z, z)))


def _uv(pose, lm):
    return project(xform(_T(pose), lm))


def _walk(pose, axis, value, target, seed, inside_is_above, zr=(0.5, 30.0), span=64, at=None):
    """Landmarks whose `value` (a function of the camera-frame point) is EXACTLY target: walk world coordinate `axis` over
    +-span ulps around a draw that nearly gets there.  -> (eq_in, in1, eq_out, out1): the landmark at target next to the inside,
    its neighbour one ulp further in, the landmark at target next to the outside, its neighbour one ulp further out."""
    r = _rng(seed)
    T = _T(pose)
    aim = target if at is None else at                         # (the image coordinate at which `value` is about target)
    for _ in range(2000):
        z = r.uniform(*zr)
        other = (r.uniform(150, 600), r.uniform(100, 380))
        if axis == 0:
            w = _world(pose, ((aim - CX) / FX * z, (other[1] - CY) / FY * z, z))
        elif axis == 1:
            w = _world(pose, ((other[0] - CX) / FX * z, (aim - CY) / FY * z, z))
        else:                                                  # depth: a point on the plane z = target
            w = _world(pose, ((other[0] - CX) / FX * z, (other[1] - CY) / FY * z, target))
        x = w[axis]
        for _k in range(span):
            x = math.nextafter(x, -INF)
        pts, vals = [], []
        for _k in range(2 * span + 1):
            p = list(w)
            p[axis] = x
            pts.append(tuple(p))
            vals.append(value(xform(T, p)))
            x = math.nextafter(x, INF)
        eq = [k for k, c in enumerate(vals) if c == target]
        if not eq or eq[0] == 0 or eq[-1] == 2 * span or eq[-1] - eq[0] + 1 != len(eq):
            continue
        lo, hi = vals[eq[0] - 1], vals[eq[-1] + 1]
        if not ((lo < target < hi) or (hi < target < lo)):
            continue
        up_is_above = hi > target
        if up_is_above == inside_is_above:                     # walking up the coordinate leads inside
            return pts[eq[-1]], pts[eq[-1] + 1], pts[eq[0]], pts[eq[0] - 1]
        return pts[eq[0]], pts[eq[0] - 1], pts[eq[-1]], pts[eq[-1] + 1]
    raise RuntimeError(f"map_gate_cases: no landmark found with the projection exactly at {target} (axis {axis}, pose {pose})")


# a special row.  lm: the landmark; feat: its feature (None: one that passes the gate if the projection is finite); flag: the
# candidate flag; m: an override of m12 (None: a fresh feature); vtags / gtags: what the visibility / gate log must hold;
# vis / kept: the expected inside() / gate result (None: not stated); ulp_of: (index of another special, coordinate) this one
# lies one ulp of that coordinate away from
Special = namedtuple("Special", "lm feat flag m vtags gtags vis kept ulp_of")


def S(lm, feat=None, flag=1, m=None, vtags=(), gtags=(), vis=None, kept=None, ulp_of=None):
    return Special(tuple(float(x) for x in lm), None if feat is None else tuple(float(x) for x in feat), int(flag), m,
                   frozenset(vtags), frozenset(gtags), vis, kept, ulp_of)


def _bound(pose, axis, target, inside_is_above, name, seed):
    val = (lambda P: project(P)[0]) if axis == 0 else (lambda P: project(P)[1])
    eq_in, in1, eq_out, out1 = _walk(pose, axis, val, target, seed, inside_is_above)
    return [S(eq_in, vtags={(name, "eq"), ("inside", 0)}, vis=False),
            S(in1, vtags={("inside", 1)}, vis=True, ulp_of=(0, axis)),
            S(eq_out, vtags={(name, "eq"), ("inside", 0)}, vis=False),
            S(out1, vtags={("inside", 0)}, vis=False, ulp_of=(2, axis))]


def _good(pose, j=0):
    """Landmarks well inside the image (a fixed family)."""
    return _at(pose, 180.0 + 37.0 * (j % 11), 120.0 + 23.0 * (j % 9), 3.0 + 1.7 * (j % 7))


def _depth_zero(pose):
    if pose == "identity":
        den = 5e-324
        return [S((1.0, 0.5, 0.0), vtags={("depth", "eq"), ("depth_sign", "pos"), ("uv", "inf"), ("inside", 0)}, vis=False),
                S((-1.0, 0.5, 0.0), vtags={("depth", "eq"), ("uv", "inf"), ("u_lo", "lt"), ("inside", 0)}, vis=False),
                S((0.0, 0.0, 0.0), vtags={("depth", "eq"), ("u_lo", "nan"), ("v_lo", "nan"), ("inside", 0)}, vis=False),
                S((1.0, 0.5, -0.0), vtags={("depth", "eq"), ("inside", 0)}, vis=False),
                S((0.0, 0.0, den), vtags={("depth", "denormal"), ("depth", "+1ulp"), ("inside", 1)}, vis=True),
                S((0.0, 0.0, -den), vtags={("depth", "-1ulp"), ("inside", 0)}, vis=False)]
    if pose == "identity_neg0":
        return [S((-1.0, -1.0, -0.0), vtags={("depth", "eq"), ("depth_sign", "neg"), ("uv", "inf"), ("inside", 0)}, vis=False),
                S((-0.0, -0.0, -0.0), vtags={("depth", "eq"), ("depth_sign", "neg"), ("u_lo", "nan"), ("inside", 0)}, vis=False),
                S((-1.0, -0.0, -0.0), vtags={("depth", "eq"), ("depth_sign", "neg"), ("v_lo", "nan"), ("inside", 0)}, vis=False)]
    eq_in, in1, eq_out, out1 = _walk(pose, 2, lambda P: P[2], 0.0, 77, True, span=256)
    return [S(eq_in, vtags={("depth", "eq"), ("inside", 0)}, vis=False),
            S(in1, vtags={("depth", "gt")}, ulp_of=(0, 2)),
            S(eq_out, vtags={("depth", "eq"), ("inside", 0)}, vis=False),
            S(out1, vtags={("depth", "lt"), ("inside", 0)}, vis=False, ulp_of=(2, 2))]


def _behind(pose):
    out = []
    for j, z in enumerate((-5.0, -0.75, -29.0)):
        lm = _at(pose, 200.0 + 150.0 * j, 140.0 + 90.0 * j, z)
        out.append(S(lm, vtags={("depth", "lt"), ("u_lo", "gt"), ("u_hi", "lt"), ("v_lo", "gt"), ("v_hi", "lt"), ("inside", 0)}, vis=False))
    return out


def _nan_inf(pose):
    out = []
    g = _good(pose, 3)
    for c in range(3):
        for bad in (NAN, INF, -INF):
            lm = list(g)
            lm[c] = bad
            out.append(S(lm, vtags={("inside", 0)}, vis=False))
    return out


def _as_lines(pose, specials, both=True):
    """Each point special as either end point of a line whose other end lies well inside."""
    out = []
    for j, s in enumerate(specials):
        g = _good(pose, 1 + (s.ulp_of[0] if s.ulp_of is not None else j))      # (a neighbour shares its partner's other end)
        for first in ((True, False) if both else (True,)):
            end = "s." if first else "e."
            lm = s.lm + g if first else g + s.lm
            up = None
            if s.ulp_of is not None:
                up = ((2 if both else 1) * s.ulp_of[0] + (0 if first else 1), s.ulp_of[1] + (0 if first else 3))
            out.append(S(lm, vtags={(end + t[0], t[1]) for t in s.vtags}, vis=s.vis, ulp_of=up))
    return out


def _visibility_classes(kind, pose):
    bounds = {"u_zero": _bound(pose, 0, 0.0, True, "u_lo", 11), "u_width": _bound(pose, 0, W, False, "u_hi", 12),
              "v_zero": _bound(pose, 1, 0.0, True, "v_lo", 13), "v_height": _bound(pose, 1, H, False, "v_hi", 14)}
    c = {k: {"b": (1.0, v)} for k, v in bounds.items()}
    c["depth_zero"] = {"b": (1.0, _depth_zero(pose))}
    if pose == "identity":
        c["depth_zero"]["neg0"] = (1.0, _depth_zero("identity_neg0"))
    c["behind_mirrored"] = {"b": (1.0, _behind(pose))}
    c["nan_inf_coords"] = {"b": (1.0, _nan_inf(pose))}
    if kind == "lines":
        one_end = [v[0] for v in bounds.values()] + _behind(pose)[:1] + _depth_zero(pose)[:1]
        for k in list(c):
            c[k] = {vn: (th, _as_lines("identity_neg0" if vn == "neg0" else pose, sp)) for vn, (th, sp) in c[k].items()}
        c["line_one_end"] = {"b": (1.0, _as_lines(pose, one_end))}
    flags = [S(_good(pose, j), flag=f, vtags={("inside", 1)}, vis=True) for j, f in enumerate((0, 1, 2, 255, 0, 128))]
    c["candidate_flags"] = {"b": (1.0, flags if kind == "points" else
                                  [S(s.lm + _good(pose, j + 5), flag=s.flag, vtags={("s.inside", 1), ("e.inside", 1)}, vis=True)
                                   for j, s in enumerate(flags)])}
    return c


def _cell_centre(cell):
    return ((cell[0] + 0.5) / INV_W, (cell[1] + 0.5) / INV_H)


def _window_classes(kind, pose):
    """cell_boundary, line_in_one_cell.  th = 20: a feature in the middle of its landmark's cell passes the point gate."""
    T = _T(pose)
    sp = []
    for axis, k, seed in ((0, 20, 41), (0, 41, 42), (1, 13, 43), (1, 30, 44)):
        val = (lambda P: project(P)[0] * INV_W) if axis == 0 else (lambda P: project(P)[1] * INV_H)
        eq_in, in1, eq_out, out1 = _walk(pose, axis, val, float(k), seed, True, at=k / (INV_W if axis == 0 else INV_H))
        name = "cell_u" if axis == 0 else "cell_v"
        base = len(sp)
        for j, (lm, on) in enumerate(((eq_in, True), (eq_out, True), (out1, False))):
            cell = cells_row("points", T, lm)[0][0]
            if cell[axis] != (k if on else k - 1):
                raise RuntimeError(f"map_gate_cases: cell_boundary {pose} axis {axis} k {k}: cell {cell}")
            sp.append(S(lm, _cell_centre(cell), vtags={("cell", cell), ("inside", 1)} | ({(name, "eq")} if on else set()), vis=True, kept=True,
                        ulp_of=(base + 1, axis) if j == 2 else None))
    for axis, target, name, seed in ((0, W, "u_hi", 12), (1, H, "v_hi", 14)):           # one ulp inside the right / bottom border
        lm = _bound(pose, axis, target, False, name, seed)[1].lm
        cell = cells_row("points", T, lm)[0][0]
        inside_grid = 0 <= cell[0] < 64 and 0 <= cell[1] < 48
        sp.append(S(lm, _cell_centre(cell) if inside_grid else (W - 1.0, H - 1.0), vtags={("cell", cell), ("inside", 1)}, vis=True))
    c = {"cell_boundary": {"b": (20.0, sp if kind == "points" else _as_lines(pose, sp))}}
    if kind == "lines":
        one = []
        for j, (u, v) in enumerate(((300.3, 200.2), (517.5, 95.5), (60.0, 400.0))):
            P, Q = _at(pose, u, v, 5.0 + j), _at(pose, u + 2.7, v + 2.8, 5.2 + j)
            cl = cells_row("lines", T, P + Q)[0]
            if cl[0] != cl[1]:
                raise RuntimeError(f"map_gate_cases: line_in_one_cell {pose}: {cl}")
            one.append(S(P + Q, vtags={("s.cell", cl[0]), ("e.cell", cl[1]), ("dir", "nan"), ("s.inside", 1), ("e.inside", 1)}, vis=True))
        c["line_in_one_cell"] = {"b": (20.0, one)}
    return c


def _exact_u(pose, th_list, seed):
    """A landmark well inside whose (u, v) are such that u -+ t and v -+ t are exact for every t in th_list (found, not solved)."""
    r = _rng(seed)
    for _ in range(500):
        lm = _at(pose, r.uniform(200, 500), r.uniform(120, 350), r.uniform(2, 20))
        u, v = _uv(pose, lm)
        if all((u - (u - t)) == t and ((u + t) - u) == t and (v - (v - t)) == t and ((v + t) - v) == t for t in th_list):
            return lm, u, v
    raise RuntimeError("map_gate_cases: no landmark with exact u - th")


def _with_th_neighbours(th, rows_at):
    """variants: the rows under th (error == th), th one ulp up (error one ulp below) and th one ulp down."""
    return {f"th{th}": (th, rows_at("eq", False)), f"th{th}_up": (math.nextafter(th, INF), rows_at("-1ulp", True)),
            f"th{th}_down": (math.nextafter(th, -INF), rows_at("+1ulp", False))}


def _gate_classes(kind, pose):
    c = {}
    good = [_good(pose, j) for j in range(12)]
    if kind == "points":
        v = {}
        for i, th in enumerate((1.0, 2.5)):
            lm, u, w = _exact_u(pose, (th,), 31 + i)

            def rows(r, kept, lm=lm, u=u, w=w, th=th):
                t = {("err", r), ("kept", int(kept))}
                return [S(lm, (u - th, w), gtags=t, vis=True, kept=kept), S(lm, (u + th, w), gtags=t, vis=True, kept=kept),
                        S(lm, (u, w - th), gtags=t, vis=True, kept=kept), S(lm, (u, w + th), gtags=t, vis=True, kept=kept),
                        S(lm, (u + 0.5 * th, w), gtags={("err", "lt"), ("kept", 1)}, vis=True, kept=True)]
            v.update(_with_th_neighbours(th, rows))
        lm, u, w = _exact_u(pose, (3.0, 4.0), 33)

        def rows5(r, kept):
            t = {("err", r), ("kept", int(kept))}
            return [S(lm, (u - 3.0, w - 4.0), gtags=t, vis=True, kept=kept), S(lm, (u + 3.0, w - 4.0), gtags=t, vis=True, kept=kept),
                    S(lm, (u - 4.0, w + 3.0), gtags=t, vis=True, kept=kept), S(lm, (u + 4.0, w + 3.0), gtags=t, vis=True, kept=kept)]
        v.update(_with_th_neighbours(5.0, rows5))
        c["epip_equal"] = v
        lm, u, w = _exact_u(pose, (0.5,), 34)
        zero = _depth_zero(pose)[0].lm
        zf = _uv(pose, zero)                                  # +-inf: the error against this feature is inf - inf
        assert math.isinf(zf[0]) or math.isinf(zf[1])

        def thr(k0, k05, kbig):
            return [S(lm, (u, w), gtags={("kept", int(k0))}, vis=True, kept=k0),
                    S(lm, (u - 0.5, w), gtags={("kept", int(k05))}, vis=True, kept=k05),
                    S(lm, (u - 1e6, w + 1e7), gtags={("kept", int(kbig))}, vis=True, kept=kbig),
                    S(zero, zf, gtags={("err", "nan"), ("kept", 0)}, kept=False)]
        c["threshold_values"] = {"th0": (0.0, thr(False, False, False)), "th-1": (-1.0, thr(False, False, False)),
                                 "thinf": (INF, thr(True, True, True)), "thnan": (NAN, thr(False, False, False))}
        gf = [tuple(x + 0.25 for x in _uv(pose, g)) for g in good]
        behind = _behind(pose)
        c["gate_no_depth_test"] = {"b": (1.0, [S(b.lm, tuple(x + 0.25 for x in _uv(pose, b.lm)), gtags={("depth", "lt"), ("err", "lt"), ("kept", 1)},
                                                 vis=False, kept=True) for b in behind] +
                                           [S(zero, zf, gtags={("depth", "eq"), ("err", "nan"), ("kept", 0)}, vis=False, kept=False)])}
    else:
        P, Q = _at(pose, 320.0, 200.0, 6.0), _at(pose, 290.0, 260.0, 7.0)
        su, eu = _uv(pose, P)[0], _uv(pose, Q)[0]
        v = {}
        for th in (1.0, 2.5):
            assert su - (su - th) == th and eu - (eu - th) == th and eu < su

            def rows(r, kept, th=th):
                t0, t1 = {("e0", r), ("kept", int(kept))}, {("e1", r), ("kept", int(kept))}
                return [S(P + Q, (1.0, 0.0, -(su - th)), gtags=t0 | {("e1", "lt")}, vis=True, kept=kept),
                        S(Q + P, (1.0, 0.0, -(su - th)), gtags=t1 | {("e0", "lt")}, vis=True, kept=kept),
                        S(P + P, (1.0, 0.0, -(su - th)), gtags=t0 | t1, vis=True, kept=kept),
                        S(P + Q, (1.0, 0.0, -(su - 0.5 * th)), gtags={("e0", "lt"), ("e1", "lt"), ("kept", 1)}, vis=True, kept=True)]
            v.update(_with_th_neighbours(th, rows))
        c["epip_equal"] = v
        A, B = _at(pose, 100.0, 200.0, 5.0), _at(pose, 650.0, 210.0, 5.0)
        ua, ub = _uv(pose, A)[0], _uv(pose, B)[0]
        c["signed_line_error"] = {"b": (1.0, [
            S(P + Q, (1.0, 0.0, -1000.0 - su), gtags={("e0", "lt"), ("e1", "lt"), ("sign", "neg"), ("kept", 1)}, vis=True, kept=True),
            S(Q + P, (1.0, 0.0, -1000.0 - eu), gtags={("sign", "neg"), ("kept", 1)}, vis=True, kept=True),
            S(A + B, (2.0, 0.0, 1000.0 - 2.0 * ub), gtags={("e0", "lt"), ("e1", "gt"), ("sign", "neg"), ("kept", 0)}, vis=True, kept=False),
            S(B + A, (2.0, 0.0, 1000.0 - 2.0 * ub), gtags={("e0", "gt"), ("e1", "lt"), ("sign", "neg"), ("kept", 0)}, vis=True, kept=False)])}
        assert abs(2.0 * ua + (1000.0 - 2.0 * ub)) > 50.0
        zero = _depth_zero(pose)[0].lm

        def thr(km2, k0, k05, kbig):
            return [S(P + Q, (0.0, 0.0, -2.0), gtags={("kept", int(km2))}, vis=True, kept=km2),
                    S(P + Q, (0.0, 0.0, 0.0), gtags={("kept", int(k0))}, vis=True, kept=k0),
                    S(P + Q, (0.0, 0.0, 0.5), gtags={("kept", int(k05))}, vis=True, kept=k05),
                    S(P + Q, (0.0, 0.0, 1e300), gtags={("kept", int(kbig))}, vis=True, kept=kbig),
                    S(zero + Q, (1.0, 1.0, 0.0), gtags={("depth", "eq"), ("kept", 0)}, kept=False)]
        c["threshold_values"] = {"th0": (0.0, thr(True, False, False, False)), "th-1": (-1.0, thr(True, False, False, False)),
                                 "thinf": (INF, thr(True, True, True, True)), "thnan": (NAN, thr(False, False, False, False))}
        good = [_good(pose, j) + _good(pose, j + 4) for j in range(12)]
        gf = [(0.0, 0.0, -1.0)] * 12
        b = _behind(pose)
        # behind the camera, the projections mirrored: l = (1, 0, -su') puts e0 at 0 and e1 at eu' - su'
        bu = [_uv(pose, x.lm)[0] for x in b]
        c["gate_no_depth_test"] = {"b": (1.0, [
            S(b[1].lm + b[0].lm, (1.0, 0.0, -bu[1]), gtags={("depth", "lt"), ("e0", "lt"), ("e1", "lt"), ("kept", 1)}, vis=False, kept=True),
            S(b[2].lm + b[1].lm, (1.0, 0.0, -bu[2]), gtags={("depth", "lt"), ("kept", 1)}, vis=False, kept=True),
            S(zero + zero, (1.0, 0.0, 0.0), gtags={("depth", "eq"), ("kept", 0)}, vis=False, kept=False),
            S((NAN,) + zero[1:] + zero, (1.0, 0.0, 0.0), gtags={("e0", "nan"), ("kept", 0)}, vis=False, kept=False)])}
    ok = {("kept", 1)}
    c["index_edges"] = {"b": (1.0, [S(good[0], gf[0], m=-1, gtags={("index", "none")}, kept=False),
                                    S(good[0], gf[0], m=-2, gtags={("index", "below")}, kept=False),
                                    S(good[0], gf[0], m=INT_MIN, gtags={("index", "below")}, kept=False),
                                    S(good[0], gf[0], m=0, gtags={("index", "first")} | ok, kept=True),
                                    S(good[1], gf[1], m="last", gtags={("index", "last")} | ok, kept=True)])}
    far = (-500.0, -500.0) if kind == "points" else (0.0, 0.0, 1e6)
    some = [S(good[j], gf[j], gtags=ok, vis=True, kept=True) for j in range(3)] + \
           [S(good[j], far, gtags={("kept", 0)}, vis=True, kept=False) for j in range(3, 5)]
    none = [S(s.lm, s.feat, gtags={("kept", 0)}, vis=True, kept=False) for s in some]
    c["association"] = {"mixed": (1.0, some), "none_pass": (0.0 if kind == "points" else -1e9, none)}
    return c


# ---- the cases ------------------------------------------------------------------------------------------------------------------
Case = namedtuple("Case", "name kind cls variant pose n Twf LM cand feat seg kf_idx m12 th rows specials driver")
# rows: {landmark row -> index into specials}; driver: the class can go through the drivers (m12 injective and in range)
DRIVER_ONLY = ("candidate_flags", "compaction_shapes")
NO_DRIVER = ("index_edges", "gate_no_depth_test")


def _ordinary(kind, pose, n, seed):
    """Landmarks, candidate flags, features and the intended matches as test_gates_and_visibility_bit_exact / test_map2kf.scene
    draw them.  n_kf = n + 3 features; three of them already carry a landmark."""
    r = _rng(seed)
    T = _pose(pose)
    n_kf = n + 3
    X = np.stack([r.uniform(-6, 6, n), r.uniform(-4, 4, n), r.uniform(-1, 30, n)], 1)
    E = X + r.uniform(-1, 1, (n, 3))
    with np.errstate(all="ignore"):
        def proj(Y):
            Yc = Y @ T[:3, :3].T + T[:3, 3]
            return np.nan_to_num(np.stack([CX + FX * Yc[:, 0] / Yc[:, 2], CY + FY * Yc[:, 1] / Yc[:, 2]], 1), posinf=0, neginf=0)
        p, q = proj(X), proj(E)
    kf_idx = np.full(n_kf, -1, np.int32)
    kf_idx[sorted({min(1, n_kf - 1), n_kf // 2, n_kf - 2})] = 7
    free = [int(j) for j in r.permutation(n_kf) if kf_idx[j] == -1]
    m12 = np.full(n, -1, np.int32)
    for i in range(n):
        if r.random() < 0.7 and len(free) > n_kf // 4:
            m12[i] = free.pop()
    cand = (r.random(n) < 0.9).astype(np.uint8)
    if kind == "points":
        feat = np.stack([r.uniform(0, W, n_kf), r.uniform(0, H, n_kf)], 1)
        ok = m12 >= 0
        feat[m12[ok]] = p[ok] + r.normal(0, 0.7, (int(ok.sum()), 2))
        return X, cand, feat, None, kf_idx, m12, free
    seg = np.concatenate([np.stack([r.uniform(0, W, n_kf), r.uniform(0, H, n_kf)], 1)] * 2, 1) + r.normal(0, 30, (n_kf, 4))
    feat = r.normal(0, 1, (n_kf, 3))
    feat /= np.linalg.norm(feat[:, :2], axis=1, keepdims=True)
    feat[:, 2] *= 200.0
    ok = m12 >= 0
    le = np.cross(np.concatenate([p, np.ones((n, 1))], 1), np.concatenate([q, np.ones((n, 1))], 1))
    nrm = np.sqrt(le[:, 0] ** 2 + le[:, 1] ** 2)
    le = le / np.where(nrm > 0, nrm, 1.0)[:, None]
    le[:, 2] += r.normal(0, 0.7, n)
    feat[m12[ok]] = le[ok]
    seg[m12[ok]] = np.clip(np.concatenate([p, q], 1)[ok], -SEG_LIMIT, SEG_LIMIT) + r.normal(0, 0.7, (int(ok.sum()), 4))
    return np.concatenate([X, E], 1), cand, feat, seg, kf_idx, m12, free


def _default_feat(kind, pose, lm):
    if kind == "lines":
        return (0.0, 0.0, -1.0)
    u, v = _uv(pose, lm)
    return (u + 0.25, v) if math.isfinite(u) and math.isfinite(v) else (100.0, 100.0)


# A keyframe segment is a pair of pixels: the windowed matcher's grid fill walks every Bresenham cell between its end points ON
# THE HOST, as the reference's getLineCoords does, so a coordinate of 1e19 (the projection of a landmark one ulp in front of
# depth zero) would keep it busy for 2^31 cells.  The segments of the cases stay within this many pixels of the origin.
SEG_LIMIT = 1.0e4


def _seg_for(kind, pose, lm):
    if kind != "lines":
        return None
    a, b = _uv(pose, lm[:3]), _uv(pose, lm[3:])
    return tuple(min(max(x, -SEG_LIMIT), SEG_LIMIT) if math.isfinite(x) else 0.0 for x in a + b)


def _build(kind, cls, variant, pose, th, specials, n, seed):
    LM, cand, feat, seg, kf_idx, m12, free = _ordinary(kind, pose, n, seed)
    n_kf = n + 3
    Kn = len(specials)
    rows = {}
    # first wave, a middle wave, the end of the last wave -- there rotated so that the launch's LAST lane holds a visible row
    jk = max([j for j in range(Kn) if specials[j].vis], default=Kn - 1)
    for s0, first in ((0, 0), (64 * (((n + 63) // 64) // 2), 0), (n - Kn, jk + 1)) if n > 1 else ((0, 0),):
        for t in range(Kn):
            if 0 <= s0 + t < n:
                rows[s0 + t] = (first + t) % Kn
    for p in rows:                                                    # the specials take fresh features
        if m12[p] >= 0:
            free.append(int(m12[p]))
            m12[p] = -1
    free = sorted(set(free))
    _rng(seed + 1).shuffle(free)
    for p, j in sorted(rows.items()):
        s = specials[j]
        LM[p] = s.lm
        cand[p] = s.flag
        f = s.feat if s.feat is not None else _default_feat(kind, pose, s.lm)
        if s.m is None:
            i2 = free.pop() if free else -1
        else:
            i2 = n_kf - 1 if s.m == "last" else s.m
        m12[p] = i2
        if 0 <= i2 < n_kf:
            feat[i2] = f
            if seg is not None:
                seg[i2] = _seg_for(kind, pose, s.lm)
    T = np.ascontiguousarray(_pose("identity_neg0" if variant == "neg0" else pose).reshape(16))
    return Case(f"{kind}/{cls}/{variant}/{pose}/{n}", kind, cls, variant, pose, n, T, LM, cand, feat, seg, kf_idx, m12, float(th),
                rows, tuple(specials), cls not in NO_DRIVER)


def _build_compaction(kind, variant, pose, n, seed):
    """compaction_shapes: the layout of the survivors of (flag != 0 and inside) over the workgroups of 256."""
    LM, cand, feat, seg, kf_idx, m12, free = _ordinary(kind, pose, n, seed)
    nb = (n + 255) // 256
    rows, specials = {}, []
    T = _T(pose)
    if variant in ("all", "last_wg", "first_wg", "one_per_wg"):
        keep = {"all": range(n), "last_wg": range(256 * (nb - 1), n), "first_wg": range(min(n, 256)),
                "one_per_wg": [min(n - 1, 256 * b + (17 + 80 * b) % 256) for b in range(nb)]}[variant]
        keep = set(keep)
        for i in range(n):
            if i in keep:
                g = _good(pose, i)
                LM[i] = g if kind == "points" else g + _good(pose, i + 3)
                cand[i] = 1 + (i % 3 == 0) * 254
                if m12[i] < 0 and free:
                    m12[i] = free.pop()
                if m12[i] >= 0:
                    feat[m12[i]] = _default_feat(kind, pose, LM[i])
                    if seg is not None:
                        seg[m12[i]] = _seg_for(kind, pose, tuple(LM[i]))
            elif variant != "all":
                cand[i] = 0 if i % 2 else cand[i]
                if i % 2 == 0:                                        # the others: flag set but behind the camera, or no flag
                    b = _at(pose, 300.0, 200.0, -4.0 - (i % 5))
                    LM[i] = b if kind == "points" else b + b
                    cand[i] = 1
    elif variant == "no_flag":
        cand[:] = 0
    elif variant == "all_behind":
        for i in range(n):
            b = _at(pose, 100.0 + i % 500, 200.0, -2.0 - (i % 7))
            LM[i] = b if kind == "points" else b + b
        cand[:] = 1
    vis = [int(cand[i] != 0 and vis_row(kind, T, [float(x) for x in LM[i]])) for i in range(n)]
    want = {"all": n, "last_wg": n - 256 * (nb - 1), "first_wg": min(n, 256), "one_per_wg": nb, "no_flag": 0, "all_behind": 0}[variant]
    if sum(vis) != want:
        raise RuntimeError(f"map_gate_cases: compaction_shapes/{variant}/{n}: {sum(vis)} survivors, {want} wanted")
    return Case(f"{kind}/compaction_shapes/{variant}/{pose}/{n}", kind, "compaction_shapes", variant, pose, n,
                np.ascontiguousarray(_pose(pose).reshape(16)), LM, cand, feat, seg, kf_idx, m12, 1.0, rows, tuple(specials), True)


@functools.lru_cache(maxsize=None)
def all_cases():
    """Every class x variant x pose x size, in a fixed order."""
    out = []
    for ki, kind in enumerate(("points", "lines")):
        for pi, pose in enumerate(POSES):
            classes = dict(_visibility_classes(kind, pose))
            classes.update(_gate_classes(kind, pose))
            classes.update(_window_classes(kind, pose))
            for ci, (cls, variants) in enumerate(classes.items()):
                for vi, (variant, (th, specials)) in enumerate(variants.items()):
                    if not specials:
                        raise RuntimeError(f"map_gate_cases: {kind}/{cls}/{variant}/{pose} is empty")
                    for n in SIZES:
                        out.append(_build(kind, cls, variant, pose, th, specials, n, 100000 * ki + 30000 * pi + 1000 * (ci + 1) + 37 * vi + n))
            for vi, variant in enumerate(("all", "no_flag", "all_behind", "last_wg", "first_wg", "one_per_wg")):
                for n in SIZES:
                    out.append(_build_compaction(kind, variant, pose, n, 100000 * ki + 30000 * pi + 29000 + 37 * vi + n))
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


# ---- the whole case through the restatement ----------------------------------------------------------------------------------
def restate_visible(c, ops=None, logs=None):
    """inside() of every landmark (no flags) -> uint8 mask; logs: one list of (comparison, outcome) per landmark."""
    o = dict(OPS, **(ops or {}))
    T = [float(x) for x in c.Twf]
    out = np.zeros(c.n, np.uint8)
    for i, lm in enumerate(c.LM.tolist()):
        lg = [] if logs is not None else None
        out[i] = vis_row(c.kind, T, lm, o, lg)
        if logs is not None:
            cells_row(c.kind, T, lm, o, lg)
            logs.append(lg)
    return out


def restate_cells(c, ops=None):
    """The window centres of every landmark -> list of cell lists (what the fast drivers compute for the LISTED landmarks)."""
    o = dict(OPS, **(ops or {}))
    T = [float(x) for x in c.Twf]
    with np.errstate(all="ignore"):
        return [cells_row(c.kind, T, lm, o)[0] for lm in c.LM.tolist()]


WINDOW_CLASSES = ("cell_boundary", "line_in_one_cell")


def window_of(c):
    """The window of the fast drivers for the case: the cell itself for the window-centre classes (a centre one cell off then
    misses its feature), the shipped 3 elsewhere."""
    return 0 if c.cls in WINDOW_CLASSES else 3


def restate_gate(c, ops=None, logs=None):
    """K5 / K6 over every landmark with m12 as the match table and every feature as the T side -> (mask, count)."""
    o = dict(OPS, **(ops or {}))
    T = [float(x) for x in c.Twf]
    feat = c.feat.tolist()
    out = np.zeros(c.n, np.uint8)
    for i, lm in enumerate(c.LM.tolist()):
        lg = [] if logs is not None else None
        out[i] = gate_row(c.kind, T, lm, int(c.m12[i]), feat, c.th, o, lg)
        if logs is not None:
            logs.append(lg)
    return out, int(out.sum())


MIN_MATCHES = 1


def restate_driver(c, ops=None):
    """The brute-force driver, GIVEN that the descriptor scan returns m12 on the listed landmarks (descriptors() makes it so):
    -> (map_to_kf, n_matches, the ascending list of the landmarks that pass flag and visibility)."""
    o = dict(OPS, **(ops or {}))
    vis = restate_visible(c, o)
    qi = [i for i in range(c.n) if c.cand[i] != 0 and vis[i]]
    table = np.full(c.n, -1, np.int32)
    n = 0
    if len(qi) > MIN_MATCHES and (c.kf_idx == -1).any():
        T = [float(x) for x in c.Twf]
        feat = c.feat.tolist()
        LM = c.LM.tolist()
        for i in qi:
            i2 = int(c.m12[i])
            if 0 <= i2 < len(feat) and c.kf_idx[i2] == -1 and gate_row(c.kind, T, LM[i], i2, feat, c.th, o):
                table[i] = i2
                n += 1
    return table, n, qi


def descriptors(c, seed=0):
    """Distinct random 256-bit rows with kf_desc[m12[i]] = med_desc[i] on the matched rows and fresh rows everywhere else:
    a mutual ratio-test scan of the listed landmarks against the unmatched features returns m12 (checked against the oracle's
    driver by the callers)."""
    r = _rng(7000 + seed + c.n)
    med = r.integers(0, 256, (c.n, 32), dtype=np.uint8)
    kfd = r.integers(0, 256, (c.n + 3, 32), dtype=np.uint8)
    ok = (c.m12 >= 0) & (c.m12 < c.n + 3)
    kfd[c.m12[ok]] = med[ok]
    return med, kfd


def fast_cfg(enabled=1, ws=3):
    return dict(enabled=enabled, grid_cols=64, grid_rows=48, ws=ws, inv_width=64 / W, inv_height=48 / H, nnr_grid=0.75, line_sim_th=0.75)


def driver_args(c):
    """(Twf, LM, med_desc, candidate, kf_desc, kf_feat, kf_idx): what oracle.map2kf_match / Context.map2kf_match take after
    (kind, cam) and before (nnr, mutual, max_epip, min_matches)."""
    med, kfd = descriptors(c)
    return (c.Twf, c.LM, med, c.cand, kfd, c.feat, c.kf_idx)


FIXTURE_SIZES = (65, 257)                       # the sizes whose reference outputs are recorded in tests/golden/ref_calls_golden.npz
