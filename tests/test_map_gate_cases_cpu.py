"""What the cases of tests/map_gate_cases.py cover is a condition on their inputs: the Python restatement alone must take each
class to the comparison outcome it is named for (membership), its mutants -- each one replaces ONE operation -- must be told
apart from it on a special row of the class meant for them (otherwise the device tests over the same cases could not tell a
wrong kernel from a right one), the C oracle must agree with it bit for bit on every case, on the lone functions and through
its drivers, and the oracle on these cases is pinned to the reference's own loops (src/mapHandler.cpp:545-558, :601-629,
:647-663, :716-749 compiled textually into oracle/_ref, or their recorded outputs in tests/golden/ref_calls_golden.npz)."""
import math

import numpy as np
import pytest

from oracle import oracle as O

import map_gate_cases as M
from test_oracle_pin import _reference

CAM = O.make_cam(**M.K)
KINDS_CLASSES = M.classes()


def _ids(kc):
    return f"{kc[0]}-{kc[1]}"


def test_every_class_is_built_at_every_size_under_both_poses():
    for kind, cls in KINDS_CLASSES:
        cs = M.cases_of(kind, cls)
        for pose in M.POSES:
            for n in M.SIZES:
                hit = [c for c in cs if c.pose == pose and c.n == n]
                assert hit, (kind, cls, pose, n)
                for c in hit:
                    assert c.LM.shape == (n, 3 if kind == "points" else 6) and c.feat.shape[0] == n + 3
                    assert cls == "compaction_shapes" or (c.rows and c.rows[0] == 0), c.name      # n = 1: the first special
                    assert c.seg is None or np.abs(c.seg).max() <= M.SEG_LIMIT + 10.0, c.name     # (segments are pixels)
                    if cls not in M.NO_DRIVER:                        # a scan can produce the table: injective, in range
                        m = c.m12[c.m12 >= 0]
                        assert len(set(m.tolist())) == len(m) and (m < n + 3).all() and (c.m12 >= -1).all(), c.name
                        assert (c.kf_idx[m] == -1).all(), c.name


@pytest.mark.parametrize("kc", KINDS_CLASSES, ids=_ids)
def test_membership(kc):
    """Every special row reaches the comparison outcomes it is named for, is decided as stated, and lies one ulp of one
    landmark coordinate from its neighbour where the class says so."""
    kind, cls = kc
    for c in M.cases_of(kind, cls):
        vlogs, glogs = [], []
        vis = M.restate_visible(c, logs=vlogs)
        mask, cnt = M.restate_gate(c, logs=glogs)
        assert cnt == int(mask.sum())
        place = {}
        for p, j in sorted(c.rows.items()):
            s = c.specials[j]
            assert tuple(c.LM[p]) == s.lm or all(a == b or (a != a and b != b) for a, b in zip(c.LM[p], s.lm)), (c.name, p)
            vt = set(vlogs[p])
            assert s.vtags <= vt, (c.name, p, sorted(s.vtags - vt))
            assert s.gtags <= set(glogs[p]), (c.name, p, sorted(s.gtags - set(glogs[p])), glogs[p])
            if s.vis is not None:
                assert bool(vis[p]) == s.vis, (c.name, p)
            if s.kept is not None:
                assert bool(mask[p]) == s.kept, (c.name, p)
            if s.m is None:
                assert c.m12[p] >= 0, (c.name, p)
            assert c.cand[p] == s.flag
            place.setdefault(j, p)
        for j, s in enumerate(c.specials):
            if s.ulp_of is not None:
                o, ax = c.specials[s.ulp_of[0]], s.ulp_of[1]
                assert all(a == b for k, (a, b) in enumerate(zip(s.lm, o.lm)) if k != ax)
                assert s.lm[ax] in (math.nextafter(o.lm[ax], math.inf), math.nextafter(o.lm[ax], -math.inf))
        if cls == "compaction_shapes":
            table, n, qi = M.restate_driver(c)
            assert qi == sorted(qi)
            nb = (c.n + 255) // 256
            per_wg = [sum(1 for i in qi if i // 256 == b) for b in range(nb)]
            want = {"all": [min(256, c.n - 256 * b) for b in range(nb)], "no_flag": [0] * nb, "all_behind": [0] * nb,
                    "last_wg": [0] * (nb - 1) + [c.n - 256 * (nb - 1)], "first_wg": [min(256, c.n)] + [0] * (nb - 1),
                    "one_per_wg": [1] * nb}[c.variant]
            assert per_wg == want, c.name
            if c.variant in ("no_flag", "all_behind"):
                assert n == 0 and (table == -1).all()


def test_u_zero_holds_the_projection_exactly_on_the_bound():
    """Spelt out once: special 0 of u_zero projects to u == 0.0 exactly, special 1 is its neighbour one ulp of X away and
    projects inside; the same for the right border."""
    for pose in M.POSES:
        T = M._T(pose)
        for cls, axis, target in (("u_zero", 0, 0.0), ("u_width", 0, M.W), ("v_zero", 1, 0.0), ("v_height", 1, M.H)):
            c = [x for x in M.cases_of("points", cls) if x.pose == pose][0]
            s0, s1 = c.specials[0], c.specials[1]
            assert M.project(M.xform(T, s0.lm))[axis] == target
            inner = M.project(M.xform(T, s1.lm))[axis]
            assert (inner > 0.0) if target == 0.0 else (inner < target)
            assert abs(inner - target) < 1e-9


# ---- the mutants: one replaced operation each -------------------------------------------------------------------------------
MUTANTS = {
    "u > 0 -> u >= 0": (dict(u_lo=lambda u: u >= 0), "vis", "u_zero"),
    "u < width -> u <= width": (dict(u_hi=lambda u: u <= M.W), "vis", "u_width"),
    "v > 0 -> v >= 0": (dict(v_lo=lambda v: v >= 0), "vis", "v_zero"),
    "v < height -> v <= height": (dict(v_hi=lambda v: v <= M.H), "vis", "v_height"),
    "the depth test dropped": (dict(depth=lambda z: True), "vis", "behind_mirrored"),
    "Pf.z > 0 -> Pf.z >= 0": (dict(depth=lambda z: z >= 0.0), "vis", "depth_zero"),
    "point gate < -> <=": (dict(pt_lt=lambda e, th: e <= th), "gate", "epip_equal"),
    "line gate < -> <=": (dict(ln_lt=lambda e, th: e <= th), "gate", "epip_equal"),
    "fabs on the line errors": (dict(ln_err=abs), "gate", "signed_line_error"),
    "&& -> || between the line errors": (dict(ln_both=lambda a, b: a or b), "gate", "signed_line_error"),
}


def test_every_mutant_is_told_apart_by_its_class(capsys):
    """Each mutant differs from the restatement on a SPECIAL row of the class meant for it, at every size and under both poses,
    for every kind it applies to (for the depth mutants on +-0: where the class holds a finite projection at depth zero -- none
    exists: x / 0 is never inside -- the neighbouring class kills it; asserted below).  Prints mutant -> classes."""
    killed, base = {}, {}
    for name, (ops, what, cls) in MUTANTS.items():
        for kind in ("points", "lines"):
            line_only = name.startswith(("line gate", "fabs", "&&"))
            if (line_only and kind == "points") or (name.startswith("point gate") and kind == "lines"):
                continue
            by, hit = set(), set()
            for c in M.all_cases():
                if c.kind != kind or not c.rows:
                    continue
                if (c.name, what) not in base:
                    base[(c.name, what)] = M.restate_visible(c) if what == "vis" else M.restate_gate(c)[0]
                a = base[(c.name, what)]
                b = M.restate_visible(c, ops) if what == "vis" else M.restate_gate(c, ops)[0]
                if any(a[p] != b[p] for p in c.rows):
                    by.add(c.cls)
                    if c.cls == cls:
                        hit.add((c.pose, c.n))
                        if c.driver and c.n > 2:                      # ... and the drivers' association shows it too
                            assert (M.restate_driver(c)[0] != M.restate_driver(c, ops)[0]).any(), c.name
            killed[(name, kind)] = sorted(by)
            if name != "Pf.z > 0 -> Pf.z >= 0":
                # (n = 1 holds one special, the class's first: it cannot serve every mutant of the class)
                assert hit >= {(p, n) for p in M.POSES for n in M.SIZES if n > 1}, (name, kind, sorted(hit))
    with capsys.disabled():
        for (name, kind), by in killed.items():
            print(f"\n  mutant [{kind}] {name} -> {', '.join(by) if by else '(no input can tell: see the docstring)'}", end="")
        print()
    for (name, kind), by in killed.items():
        cls = MUTANTS[name][2]
        if name == "Pf.z > 0 -> Pf.z >= 0":
            # a projection at depth +-0 is +-inf or NaN, which the four bounds reject whatever the depth test says: the mutant
            # computes the same function, and the class asserts that the depth-zero rows are rejected all the same
            assert by == [], by
        else:
            assert cls in by, (name, kind, by)


# ---- the oracle on every case -----------------------------------------------------------------------------------------------
def _o_visible(c):
    with np.errstate(all="ignore"):
        return (O.map_point_visible if c.kind == "points" else O.map_line_visible)(CAM, c.Twf, c.LM)


def _o_gate(c):
    with np.errstate(all="ignore"):
        return (O.map2kf_point_gate if c.kind == "points" else O.map2kf_line_gate)(CAM, c.Twf, c.LM, c.m12, c.feat, c.th)


@pytest.mark.parametrize("kc", KINDS_CLASSES, ids=_ids)
def test_oracle_agrees_with_the_restatement(kc):
    """oracle.map_*_visible, map2kf_*_gate, map2kf_match and map2kf_match_fast (fast matching off: the same road) against the
    restatement, bit for bit; through the drivers the descriptor scan must have produced the class's m12 (descriptors())."""
    kind, cls = kc
    for c in M.cases_of(kind, cls):
        assert np.array_equal(_o_visible(c), M.restate_visible(c)), c.name
        mask, cnt = _o_gate(c)
        rmask, rcnt = M.restate_gate(c)
        assert np.array_equal(mask, rmask) and cnt == rcnt, c.name
        if not c.driver:
            continue
        table, n, qi = M.restate_driver(c)
        got, gn = O.map2kf_match(kind, CAM, *M.driver_args(c), 0.75, True, c.th, M.MIN_MATCHES)
        assert np.array_equal(got, table) and gn == n == int((table >= 0).sum()), c.name
        got, gn, used = O.map2kf_match_fast(kind, CAM, *M.driver_args(c), 0.75, True, c.th, M.MIN_MATCHES, M.fast_cfg(enabled=0),
                                            kf_seg=c.seg)
        assert np.array_equal(got, table) and gn == n and used == int(len(qi) > M.MIN_MATCHES), c.name


# ---- the oracle pinned to the reference's own loops on these cases ---------------------------------------------------------
def _first(r):
    return None if r is None else r[0]


@pytest.mark.parametrize("kc", KINDS_CLASSES, ids=_ids)
def test_pinned_to_reference_source_text(kc):
    """The visibility pre-filter loop and the gate loop of the reference, compiled textually (oracle/_ref) or recorded
    (tests/golden/ref_calls_golden.npz, written by tests/golden/make_ref_calls_golden.py), on the cases of FIXTURE_SIZES: the
    mask of the landmarks selected, the mask of the landmarks that received the observation and the final `matches`."""
    kind, cls = kc
    checked = 0
    for c in M.cases_of(kind, cls):
        if c.n not in M.FIXTURE_SIZES:
            continue
        ref = _reference(f"map_edges/vis/{c.name}", lambda: _first(O.ref_map_visible(kind, CAM, c.Twf, c.LM, 1.0 / M.W, 1.0 / M.H)))
        assert np.array_equal(_o_visible(c), ref), c.name
        rmask, rcnt = _reference(f"map_edges/gate/{c.name}", lambda: O.ref_map2kf_gate(kind, CAM, c.Twf, c.LM, c.m12, c.feat, c.th))
        mask, cnt = _o_gate(c)
        assert np.array_equal(mask, rmask) and cnt == rcnt, c.name
        checked += 1
    assert checked >= 2 * len(M.FIXTURE_SIZES)


# ---- the window centres of the fast drivers ---------------------------------------------------------------------------------
CELL_MUTANTS = {
    "floor for the cells": dict(cell=lambda x: M.cvtt(math.floor(x)) if x == x and abs(x) < 2e9 else M.cvtt(x)),
    "round to nearest for the cells": dict(cell=lambda x: M.cvtt(float(round(x))) if x == x and abs(x) < 2e9 else M.cvtt(x)),
    "ceil for the cells": dict(cell=lambda x: M.cvtt(math.ceil(x)) if x == x and abs(x) < 2e9 else M.cvtt(x)),
    "the cell one to the left": dict(cell=lambda x: M.cvtt(x) - 1 if M.cvtt(x) != M.INT_MIN else M.INT_MIN),
}


def test_cell_mutants_and_what_floor_can_and_cannot_show(capsys):
    """The window centres are computed for the LISTED landmarks only: flag set and inside the image, so u * inv_width and
    v * inv_height are positive, where floor IS truncation.  No input of the map<->keyframe drivers can tell that mutant apart --
    asserted here over every listed landmark of every case, together with the fact that the mutant is a real one (it differs
    on landmarks that are NOT listed, whose projections are negative).  What a wrong cell looks like on the device is shown by the
    other three mutants, each told apart on a special row of cell_boundary at every size and under both poses."""
    told = {}
    for name, ops in CELL_MUTANTS.items():
        hit, off_list, by = set(), 0, set()
        for c in M.all_cases():
            listed = set(M.restate_driver(c)[2])
            a, b = M.restate_cells(c), M.restate_cells(c, ops)
            diff = [i for i in range(c.n) if a[i] != b[i]]
            off_list += sum(1 for i in diff if i not in listed)
            if any(i in listed and i in c.rows for i in diff):
                by.add(c.cls)
                if c.cls == "cell_boundary":
                    hit.add((c.kind, c.pose, c.n))
            if name == "floor for the cells":
                assert not any(i in listed for i in diff), c.name
        told[name] = sorted(by)
        if name == "floor for the cells":
            assert off_list > 0
        else:
            assert hit >= {(k, p, n) for k in ("points", "lines") for p in M.POSES for n in M.SIZES if n > 1}, (name, sorted(hit))
    with capsys.disabled():
        for name, by in told.items():
            print(f"\n  mutant {name} -> {', '.join(by) if by else '(equal to truncation on every listed landmark: see the docstring)'}", end="")
        print()


@pytest.mark.parametrize("pose", M.POSES)
def test_oracle_window_centres_are_the_restatements(pose):
    """The oracle exposes no window centres; its fast driver with a window of ONE cell does: every listed special of
    cell_boundary (points) is associated with the feature that lies in the middle of the cell the restatement computes -- and no
    longer when that feature is moved into the cell to the left.  min_matches = 0: the brute-force scan never replaces the grid."""
    for c in M.cases_of("points", "cell_boundary"):
        if c.pose != pose or c.n < 63:
            continue
        a = M.driver_args(c)
        table, n, used = O.map2kf_match_fast("points", CAM, *a, 0.75, True, c.th, 0, M.fast_cfg(ws=0), kf_seg=c.seg)
        assert used == 0
        cells = M.restate_cells(c)
        listed = set(M.restate_driver(c)[2])
        checked = 0
        for p, j in c.rows.items():
            if p not in listed or not (0 <= cells[p][0][0] < 64 and 0 <= cells[p][0][1] < 48):
                continue
            f = c.feat[c.m12[p]]
            assert (M.cvtt(f[0] * M.INV_W), M.cvtt(f[1] * M.INV_H)) == cells[p][0], (c.name, p)
            assert table[p] == c.m12[p], (c.name, p, cells[p])
            moved = c.feat.copy()
            moved[c.m12[p], 0] -= 1.0 / M.INV_W
            t2 = O.map2kf_match_fast("points", CAM, a[0], a[1], a[2], a[3], a[4], moved, a[6], 0.75, True, c.th, 0, M.fast_cfg(ws=0))[0]
            assert t2[p] != c.m12[p], (c.name, p)
            checked += 1
        assert checked >= 6, c.name
