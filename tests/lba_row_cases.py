"""Named inputs that put the local-BA rows (plslam_amd/csrc/lba_rows_dev.hpp: point_row, line_row with the iteration pass's
quirk, dmax_gt; K3 / K4 in lba.hip; specification = oracle/plslam_oracle.c plo_lba_point_rows / plo_lba_line_rows, of
src/mapHandler.cpp:1358-1407 and :1436-1516) ON the switches of their two std::max(homogTh, .) terms, for
tests/test_lba_row_cases_cpu.py (membership, mutants, oracle, reference pin, contract tolerance) and for
tests/test_gpu_lba_row_edges.py (every way the rows run on the device).  numpy only.

A case is N_SLOTS = 70 key-frame poses (slot 0 the identity, slot 1 the pose of test_gates_and_visibility_bit_exact, the rest
small motions), n landmarks (points n x 3, lines n x 6), n observations -- observation o sees landmark lm[o] from slot kf[o] --
and the threshold th.  Every class is built at n in SIZES (one lane per row, 256-lane workgroups; odd and even row counts for
the 3-wide and 6-wide stores: the class `tails` is these sizes and nothing else): ordinary rows drawn like synth.local_map's,
the rows of interest written over them at the start of the first wave, of a middle wave and at the end of the last one (n = 1
holds the class's first special).  Line cases are also run with compat_iter_pass (both end points read at stride 3, th the
literal 1e-7).  Inputs on a switch are FOUND under the restatement below (a walk over the nextafter neighbours of the
landmark's Z; th taken from the row's own residual), not solved for; the builder raises when it finds none.

  depth_sq_at_th   th = 2^-24: camera-frame depth exactly 2^-12 (z^2 == th: both sides of the max are the same number), one ulp
                   either side (k switches between 1 / th and 1 / z^2), the negative depths of the same sizes; under the
                   identity slot and, found by the walk, under slot 1.  Lines: P below with Q above, the reverse, both equal
  residual_at_th   th == the row's own residual norm, th one ulp up and one ulp down (the divisor switches between th and nrm);
                   the residual exactly 0: the observation ON the projection (points), e0 == 0, e1 == 0, both (lines) --
                   rows of signed zeros
  depth_zero       camera-frame depth +0 and -0: inf / NaN rows
  nan_inf          NaN, +inf, -inf in a landmark coordinate or in the observation: where the operand order of dmax_gt shows
  slot_edges       rows whose pose slot is 31, 32, 33 and 69 (the workgroup's LDS copy holds the first min(n_pose_slots, 32))
  tails            ordinary rows only
"""
from __future__ import annotations

import functools
import math
from collections import namedtuple

import numpy as np

from plslam_amd import synth
from stereo_gate_cases import SIZES, rel

K = synth.EUROC
FX, FY, CX, CY = (float(K[k]) for k in ("fx", "fy", "cx", "cy"))
NAN, INF = math.nan, math.inf
N_SLOTS = 70
TH24 = 2.0 ** -24
Z12 = 2.0 ** -12


def _rng(seed):
    return np.random.Generator(np.random.PCG64(seed))


@functools.lru_cache(maxsize=None)
def poses():
    """(N_SLOTS, 16): T_kf_w of every slot."""
    r = _rng(4)
    T = [np.eye(4), synth.se3_exp([0.1, -0.05, 0.3, 0.01, 0.02, -0.01])]
    for k in range(2, N_SLOTS):
        T.append(synth.se3_exp(np.concatenate([r.normal(0, 0.3, 3), r.normal(0, 0.03, 3)])))
    return np.ascontiguousarray(np.stack(T).reshape(N_SLOTS, 16))


# ---- the restatement: Python floats, the kernels' operation order ------------------------------------------------------------------
def dmax_gt(a, b):
    return a if a > b else b


OPS = dict(dmax=dmax_gt, k=lambda th, z2, dmax: ddiv(1.0, dmax(th, z2)), compat_stride=3)


def inv_pose(m):
    R = [0.0] * 9
    t = [0.0] * 3
    for i in range(3):
        R[3 * i], R[3 * i + 1], R[3 * i + 2] = m[i], m[4 + i], m[8 + i]
        t[i] = (-m[i]) * m[3] + (-m[4 + i]) * m[7] + (-m[8 + i]) * m[11]
    return R, t


def xform(R, t, X):
    x, y, z = X
    return [(R[3 * i] * x + R[3 * i + 1] * y + R[3 * i + 2] * z) + t[i] for i in range(3)]


def project(P):
    return CX + ddiv(FX * P[0], P[2]), CY + ddiv(FY * P[1], P[2])


def jac6(a, b, k, G):
    gx, gy, gz = G
    return [+k * a * gz, +k * b * gz, -k * (a * gx + b * gy), -k * (a * gx * gy + b * gy * gy + b * gz * gz),
            +k * (a * gx * gx + a * gz * gz + b * gx * gy), +k * (b * gx * gz - a * gy * gz)]


# Which NaN an operation generates or hands on (sign, payload) is the implementation's choice under IEEE 754, and the GPU's is
# not the host's: a row entry that is not a number is stored as ONE NaN, the positive quiet one (one_nan in lba_rows_dev.hpp and
# in the oracle), and so it is here.
GEN_NAN = math.nan
ONE_NAN_BITS = 0x7FF8000000000000


def one_nan(x):
    return math.nan if x != x else x


def ddiv(a, b):
    """a / b in IEEE double arithmetic (Python raises on a zero divisor)."""
    if b == 0.0:
        if a != a:
            return a
        if a == 0.0:
            return GEN_NAN
        return math.copysign(INF, a) * math.copysign(1.0, b)
    return a / b


def _sqrt(x):
    return math.sqrt(x) if x == x and x >= 0 else (x if x != x else GEN_NAN)


def point_row(th, T, X, ob, ops=OPS, log=None):
    """-> (J_pose[6], J_lm[3], r, w)."""
    say = log.append if log is not None else (lambda t: None)
    R, t = inv_pose(T)
    G = xform(R, t, X)
    pu, pv = project(G)
    dx, dy = ob[0] - pu, ob[1] - pv
    nrm = _sqrt(dx * dx + dy * dy)
    say(("z2", rel(G[2] * G[2], th)))
    say(("depth", rel(G[2], 0.0)))
    if G[2] == 0.0:
        say(("depth_sign", "neg" if math.copysign(1.0, G[2]) < 0 else "pos"))
    say(("nrm", rel(nrm, th)))
    if nrm == 0.0:
        say(("nrm", "zero"))
    k = ops["k"](th, G[2] * G[2], ops["dmax"])
    a, b = FX * dx, FY * dy
    Jc = jac6(a, b, k, G)
    den = ops["dmax"](th, nrm)
    Jp = [ddiv(c, den) for c in Jc]
    Jl = [ddiv(Jc[0] * R[j] + Jc[1] * R[3 + j] + Jc[2] * R[6 + j], den) for j in range(3)]
    w = ddiv(1.0, 1.0 + nrm * nrm)
    if not all(math.isfinite(v) for v in Jp + Jl + [nrm, w]):
        say(("row", "nonfinite"))
    return [one_nan(v) for v in Jp], [one_nan(v) for v in Jl], one_nan(nrm), one_nan(w)


def line_row(th, T, Pw, Qw, l, ops=OPS, log=None):
    """-> (J_pose[6], J_lm[6], r, w)."""
    say = log.append if log is not None else (lambda t: None)
    R, t = inv_pose(T)
    P, Q = xform(R, t, Pw), xform(R, t, Qw)
    pu, pv = project(P)
    qu, qv = project(Q)
    e0 = l[0] * pu + l[1] * pv + l[2]
    e1 = l[0] * qu + l[1] * qv + l[2]
    nrm = _sqrt(e0 * e0 + e1 * e1)
    say(("zP2", rel(P[2] * P[2], th)))
    say(("zQ2", rel(Q[2] * Q[2], th)))
    say(("depth", rel(P[2], 0.0)))
    if P[2] == 0.0:
        say(("depth_sign", "neg" if math.copysign(1.0, P[2]) < 0 else "pos"))
    say(("nrm", rel(nrm, th)))
    if nrm == 0.0:
        say(("nrm", "zero"))
    if e0 == 0.0:
        say(("e0", "zero"))
    if e1 == 0.0:
        say(("e1", "zero"))
    a, b = FX * e0, FY * e1
    kP = ops["k"](th, P[2] * P[2], ops["dmax"])
    kQ = ops["k"](th, Q[2] * Q[2], ops["dmax"])
    JP, JQ = jac6(a, b, kP, P), jac6(a, b, kQ, Q)
    den = ops["dmax"](th, nrm)
    Jl = [0.0] * 6
    for j in range(3):
        vp = JP[0] * R[j] + JP[1] * R[3 + j] + JP[2] * R[6 + j]
        vq = JQ[0] * R[j] + JQ[1] * R[3 + j] + JQ[2] * R[6 + j]
        Jl[j] = ddiv(vp * e0, den)
        Jl[3 + j] = ddiv(vq * e1, den)
    Jp = [ddiv(JP[c] * e0 + JQ[c] * e1, den) for c in range(6)]
    w = ddiv(1.0, 1.0 + nrm * nrm)
    if not all(math.isfinite(v) for v in Jp + Jl + [nrm, w]):
        say(("row", "nonfinite"))
    return [one_nan(v) for v in Jp], [one_nan(v) for v in Jl], one_nan(nrm), one_nan(w)


# ---- finding the inputs ---------------------------------------------------------------------------------------------------------
def _world(slot, pc):
    T = poses()[slot].reshape(4, 4)
    return tuple(float(x) for x in T[:3, :3] @ np.asarray(pc, float) + T[:3, 3])


def _depth(slot, X):
    R, t = inv_pose(poses()[slot].tolist())
    return xform(R, t, X)[2]


def _walk_depth(slot, target, seed, span=512):
    """(below, at, above): landmarks seen from `slot` at camera-frame depth exactly `target` and one ulp of the world Z either
    side, with depths strictly below / above."""
    r = _rng(seed)
    for _ in range(4000):
        w = list(_world(slot, (r.uniform(-0.1, 0.1) * target, r.uniform(-0.1, 0.1) * target, target)))
        z = w[2]
        for _k in range(span):
            z = math.nextafter(z, -INF)
        pts = []
        for _k in range(2 * span + 1):
            pts.append((w[0], w[1], z))
            z = math.nextafter(z, INF)
        d = [_depth(slot, p) for p in pts]
        eq = [k for k, v in enumerate(d) if v == target]
        if len(eq) != 1 or eq[0] in (0, 2 * span):
            continue
        k = eq[0]
        lo, hi = (pts[k - 1], pts[k + 1]) if d[k - 1] < target else (pts[k + 1], pts[k - 1])
        if _depth(slot, lo) < target < _depth(slot, hi):
            return lo, pts[k], hi
    raise RuntimeError(f"lba_row_cases: no landmark at depth exactly {target} from slot {slot}")


# a special row: the slot, the landmark (3 or 6 doubles), the observation (2 or 3), the tags its log must hold, and whether
# the row sits exactly on a dmax_gt switch (excluded from the contract-tolerance comparison)
Special = namedtuple("Special", "slot lm obs tags on_switch")


def S(slot, lm, obs, tags=(), on_switch=False):
    return Special(int(slot), tuple(float(x) for x in lm), tuple(float(x) for x in obs), frozenset(tags), on_switch)


def _obs_point(slot, X, off=(0.3, -0.2)):
    R, t = inv_pose(poses()[slot].tolist())
    u, v = project(xform(R, t, X))
    return (u + off[0], v + off[1])


def _generic(kind, slot, j=0):
    X = _world(slot, (0.4 - 0.13 * j, -0.3 + 0.07 * j, 4.0 + 1.3 * j))
    if kind == "points":
        return X, _obs_point(slot, X, (0.6 + 0.1 * j, -0.45))
    Q = _world(slot, (0.1 + 0.13 * j, 0.2, 5.0 + 0.9 * j))
    return X + Q, (0.6, -0.8, 180.0 + 3.0 * j)


def _nrm_of(kind, slot, lm, obs, th=1e-7):
    T = poses()[slot].tolist()
    return (point_row(th, T, lm, obs) if kind == "points" else line_row(th, T, lm[:3], lm[3:], obs))[2]


def _classes(kind):
    c = {}
    pts = kind == "points"
    # depth_sq_at_th
    sp = []
    for slot in (0, 1):
        for sign in (1.0, -1.0):
            if slot == 0:
                lo, at, hi = ((0.1 * Z12, -0.05 * Z12, sign * z) for z in (math.nextafter(Z12, 0.0), Z12, math.nextafter(Z12, 1.0)))
            else:
                lo, at, hi = _walk_depth(slot, sign * Z12, 21 + int(sign))
                if sign < 0:
                    lo, hi = hi, lo                                    # lo: |z| below 2^-12
            if pts:
                sp += [S(slot, at, _obs_point(slot, at), {("z2", "eq")}, True), S(slot, lo, _obs_point(slot, lo), {("z2", "lt")}),
                       S(slot, hi, _obs_point(slot, hi), {("z2", "gt")})]
            else:
                ob = (0.6, -0.8, 100.0)
                sp += [S(slot, lo + hi, ob, {("zP2", "lt"), ("zQ2", "gt")}), S(slot, hi + lo, ob, {("zP2", "gt"), ("zQ2", "lt")}),
                       S(slot, at + at, ob, {("zP2", "eq"), ("zQ2", "eq")}, True), S(slot, at + hi, ob, {("zP2", "eq"), ("zQ2", "gt")}, True)]
    c["depth_sq_at_th"] = {"b": (TH24, sp)}
    # residual_at_th
    v = {}
    for slot in (0, 1):
        lm, ob = _generic(kind, slot, 1)
        nrm = _nrm_of(kind, slot, lm, ob)
        R, t = inv_pose(poses()[slot].tolist())
        if pts:
            zero = [S(slot, lm, project(xform(R, t, lm)), {("nrm", "zero")})]
        else:
            pu, qu = project(xform(R, t, lm[:3]))[0], project(xform(R, t, lm[3:]))[0]
            zero = [S(slot, lm, (1.0, 0.0, -pu), {("e0", "zero")}), S(slot, lm, (1.0, 0.0, -qu), {("e1", "zero")}),
                    S(slot, lm[:3] + lm[:3], (1.0, 0.0, -pu), {("e0", "zero"), ("e1", "zero"), ("nrm", "zero")})]
        for name, th, r_, sw in (("eq", nrm, "eq", True), ("th_up", math.nextafter(nrm, INF), "-1ulp", False),
                                 ("th_down", math.nextafter(nrm, 0.0), "+1ulp", False)):
            v[f"{name}/slot{slot}"] = (th, [S(slot, lm, ob, {("nrm", r_)}, sw)] + zero)
    c["residual_at_th"] = v
    # depth_zero (identity slot: G == X exactly, and -0 only from all-negative products)
    if pts:
        dz = [S(0, (0.5, 0.25, 0.0), (300.0, 200.0), {("depth", "eq"), ("depth_sign", "pos"), ("row", "nonfinite")}),
              S(0, (-1.0, -1.0, -0.0), (300.0, 200.0), {("depth", "eq"), ("depth_sign", "neg"), ("row", "nonfinite")}),
              S(0, (0.0, 0.0, 0.0), (300.0, 200.0), {("depth", "eq"), ("row", "nonfinite")})]
        bad = []
        g, ob = _generic(kind, 1, 2)
        for cc in range(3):
            for b in (NAN, INF, -INF):
                x = list(g)
                x[cc] = b
                bad.append(S(1, x, ob, {("row", "nonfinite")}))
        for cc in range(2):
            for b in (NAN, INF, -INF):
                o = list(ob)
                o[cc] = b
                bad.append(S(1, g, o, {("row", "nonfinite")}))
    else:
        good = _generic(kind, 0, 2)[0]
        ob = (0.6, -0.8, 100.0)
        dz = [S(0, (0.5, 0.25, 0.0) + good[3:], ob, {("depth", "eq"), ("depth_sign", "pos"), ("row", "nonfinite")}),
              S(0, (-1.0, -1.0, -0.0) + good[3:], ob, {("depth", "eq"), ("depth_sign", "neg"), ("row", "nonfinite")}),
              S(0, good[:3] + (0.0, 0.0, 0.0), ob, {("row", "nonfinite")})]
        bad = []
        g, ob = _generic(kind, 1, 2)
        for cc in range(6):
            for b in (NAN, INF, -INF):
                x = list(g)
                x[cc] = b
                bad.append(S(1, x, ob, {("row", "nonfinite")}))
        for cc in range(3):
            for b in (NAN, INF):
                o = list(ob)
                o[cc] = b
                bad.append(S(1, g, o, {("row", "nonfinite")}))
    c["depth_zero"] = {"b": (1e-7, dz)}
    c["nan_inf"] = {"b": (1e-7, bad), "th_nan": (NAN, bad[:4] + [S(1, *_generic(kind, 1, 3))])}
    c["slot_edges"] = {"b": (1e-7, [S(s, *_generic(kind, s, j)) for j, s in enumerate((31, 32, 33, 69, 0, 30))])}
    c["tails"] = {"b": (1e-7, [S(2, *_generic(kind, 2, 1))])}
    return c


FINITE = ("depth_sq_at_th", "residual_at_th", "slot_edges", "tails")       # every row of these classes is finite

Case = namedtuple("Case", "name kind cls variant n T LM obs lm kf th rows specials")


def _ordinary(kind, n, seed):
    r = _rng(seed)
    T = poses().reshape(N_SLOTS, 4, 4)
    kf = r.integers(0, N_SLOTS, n).astype(np.int32)
    z = r.uniform(2.0, 30.0, n)
    pc = np.stack([r.uniform(-0.6, 0.6, n) * z, r.uniform(-0.4, 0.4, n) * z, z], 1)
    X = np.einsum("nij,nj->ni", T[kf, :3, :3], pc) + T[kf, :3, 3]
    uv = np.stack([CX + FX * pc[:, 0] / pc[:, 2], CY + FY * pc[:, 1] / pc[:, 2]], 1)
    lm = r.permutation(n).astype(np.int32)
    Xs = np.empty_like(X)
    Xs[lm] = X                                                         # observation o sees landmark lm[o]
    if kind == "points":
        return Xs, uv + r.normal(0, 1.0, (n, 2)), lm, kf
    qc = pc + r.uniform(-0.5, 0.5, (n, 3))
    Q = np.einsum("nij,nj->ni", T[kf, :3, :3], qc) + T[kf, :3, 3]
    uq = np.stack([CX + FX * qc[:, 0] / qc[:, 2], CY + FY * qc[:, 1] / qc[:, 2]], 1)
    le = np.cross(np.concatenate([uv, np.ones((n, 1))], 1), np.concatenate([uq, np.ones((n, 1))], 1))
    le /= np.maximum(np.linalg.norm(le[:, :2], axis=1, keepdims=True), 1e-12)
    le[:, 2] += r.normal(0, 1.0, n)
    Ls = np.empty((n, 6))
    Ls[lm] = np.concatenate([X, Q], 1)
    return Ls, le, lm, kf


def _build(kind, cls, variant, th, specials, n, seed):
    LM, obs, lm, kf = _ordinary(kind, n, seed)
    Kn = len(specials)
    rows = {}
    for s0 in ((0, 64 * (((n + 63) // 64) // 2), n - Kn) if n > 1 else (0,)):
        for t in range(Kn):
            if 0 <= s0 + t < n:
                rows[s0 + t] = t
    for p, j in sorted(rows.items()):
        s = specials[j]
        LM[lm[p]] = s.lm
        obs[p] = s.obs
        kf[p] = s.slot
    return Case(f"{kind}/{cls}/{variant}/{n}", kind, cls, variant, n, poses(), LM, obs, lm, kf, float(th), rows, tuple(specials))


@functools.lru_cache(maxsize=None)
def all_cases():
    out = []
    for ki, kind in enumerate(("points", "lines")):
        for ci, (cls, variants) in enumerate(_classes(kind).items()):
            for vi, (variant, (th, specials)) in enumerate(variants.items()):
                if not specials:
                    raise RuntimeError(f"lba_row_cases: {kind}/{cls}/{variant} is empty")
                for n in SIZES:
                    out.append(_build(kind, cls, variant, th, specials, n, 50000 * ki + 1000 * (ci + 1) + 37 * vi + n))
    return tuple(out)


def classes():
    seen = []
    for c in all_cases():
        if (c.kind, c.cls) not in seen:
            seen.append((c.kind, c.cls))
    return seen


def cases_of(kind, cls):
    return [c for c in all_cases() if c.kind == kind and c.cls == cls]


def restate(c, compat=False, ops=None, logs=None):
    """The whole case through the restatement -> (J_pose (n, 6), J_lm (n, 3 | 6), r, w) as float64 arrays."""
    o = dict(OPS, **(ops or {}))
    T = c.T.tolist()
    flat = c.LM.reshape(-1).tolist()
    obs = c.obs.tolist()
    pts = c.kind == "points"
    Jp, Jl = np.empty((c.n, 6)), np.empty((c.n, 3 if pts else 6))
    r, w = np.empty(c.n), np.empty(c.n)
    th = o.get("compat_th", 0.0000001) if (compat and not pts) else c.th      # (:1698 - :1741: a literal, not homogTh)
    for i in range(c.n):
        lg = [] if logs is not None else None
        l = int(c.lm[i])
        if pts:
            res = point_row(th, T[c.kf[i]], flat[3 * l:3 * l + 3], obs[i], o, lg)
        elif compat:
            st = o["compat_stride"]
            P = flat[st * l:st * l + 3]
            res = line_row(th, T[c.kf[i]], P, P, obs[i], o, lg)
        else:
            res = line_row(th, T[c.kf[i]], flat[6 * l:6 * l + 3], flat[6 * l + 3:6 * l + 6], obs[i], o, lg)
        Jp[i], Jl[i], r[i], w[i] = res
        if logs is not None:
            logs.append(lg)
    return Jp, Jl, r, w


def row_args(c):
    """(th, T_kf_w, landmarks, observations, lm, kf): what oracle.lba_*_rows / Context.lba_*_rows take after cam."""
    return (c.th, c.T, c.LM, c.obs, c.lm, c.kf)


FIXTURE_SIZES = (65, 257)
