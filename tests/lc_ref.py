"""Plain numpy restatement of MapHandler::isLoopClosure (src/mapHandler.cpp:3192-3300) and computeRelativePoseRobustGN
(:3566-3957): the checker of K25 (plslam_amd/csrc/loop_closure.hip).

It builds on the oracle: StVO::match (O.match), the Gauss-Newton system of one iteration (O.pose_gn_accumulate, a sequential
C restatement of :3595-3689 pinned to the reference's own text in tests/test_oracle_pin.py) and stvo-pl's SE(3) maps
(O.expmap_se3 / logmap_se3 / inverse_se3).  The 6 x 6 solve restates Eigen's ColPivHouseholderQR; the covariance test
restates Eigen's PartialPivLU inverse and takes the eigenvalues with numpy.linalg.eigvalsh of its lower triangle."""
from __future__ import annotations

import math

import numpy as np

from oracle import oracle as O

EPS = np.finfo(np.float64).eps          # numeric_limits<double>::epsilon()
CHI = math.sqrt(7.815)                   # :3728, :3750
CV_PI = 3.1415926535897932384626433832795


def std_max(a, b):
    """std::max(a, b) = (a < b) ? b : a -- max(NaN, x) is NaN, max(x, NaN) is x"""
    return b if a < b else a


def ratio(c, n):
    """100.0 * c / n with int n (:3273): 0 / 0 is NaN, c / 0 is inf"""
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(np.float64(100.0 * c) / np.float64(n))


def colpiv_qr_solve(H, g, log=None):
    """Eigen::ColPivHouseholderQR<MatrixXd>(H).solve(g) (ColPivHouseholderQR.h computeInPlace / _solve_impl, Eigen 3.3-3.4):
    column pivoting on the largest updated norm (first index on ties), Householder reflections as makeHouseholder builds
    them, the LAPACK norm downdate, the rank cut at (max col norm * eps)^2 / rows * (rows - k), and a column-major back
    substitution that skips zero right-hand entries (so H = 0, g = 0 gives x = 0).  log: a list that receives one
    dict(tr=the transposition list, rank=, recomputes=how often the downdate recomputed a norm) per call."""
    n = 6
    A = np.array(H, dtype=np.float64).reshape(6, 6).copy()
    nd = np.array([math.sqrt(float(np.sum(A[:, j] * A[:, j]))) for j in range(n)])
    nu = nd.copy()
    maxn = nu[0]
    for j in range(1, n):
        if nu[j] > maxn:
            maxn = nu[j]
    th_help = (maxn * EPS) * (maxn * EPS) / n
    down_th = math.sqrt(EPS)
    nz = n
    recomputes = 0
    tr = [0] * n
    hc = np.zeros(n)
    for k in range(n):
        b, bn = k, nu[k]
        for j in range(k + 1, n):
            if nu[j] > bn:
                b, bn = j, nu[j]
        if nz == n and bn * bn < th_help * (n - k):
            nz = k
        tr[k] = b
        if b != k:
            A[:, [k, b]] = A[:, [b, k]]
            nu[[k, b]] = nu[[b, k]]
            nd[[k, b]] = nd[[b, k]]
        v = A[k:, k]
        tail = float(np.sum(v[1:] * v[1:])) if n - k > 1 else 0.0
        c0 = v[0]
        if tail <= np.finfo(np.float64).tiny:
            tau, beta = 0.0, c0
            v[1:] = 0.0
        else:
            beta = math.sqrt(c0 * c0 + tail)
            if c0 >= 0.0:
                beta = -beta
            v[1:] = v[1:] / (c0 - beta)
            tau = (beta - c0) / beta
        hc[k] = tau
        v[0] = beta
        if n - k == 1:
            A[k, k + 1:] *= (1.0 - tau)
        elif tau != 0.0:
            for j in range(k + 1, n):
                t = float(np.sum(v[1:] * A[k + 1:, j])) + A[k, j]
                A[k, j] -= tau * t
                A[k + 1:, j] -= tau * v[1:] * t
        for j in range(k + 1, n):
            if nu[j] != 0.0:
                t = abs(A[k, j]) / nu[j]
                t = (1.0 + t) * (1.0 - t)
                t = 0.0 if t < 0.0 else t
                q = nu[j] / nd[j]
                if t * (q * q) <= down_th:
                    nd[j] = math.sqrt(float(np.sum(A[k + 1:, j] * A[k + 1:, j])))
                    nu[j] = nd[j]
                    recomputes += 1
                else:
                    nu[j] *= math.sqrt(t)
    perm = list(range(n))
    for k in range(n):
        perm[k], perm[tr[k]] = perm[tr[k]], perm[k]
    x = np.zeros(n)
    if log is not None:
        log.append(dict(tr=tuple(int(b) for b in tr), rank=int(nz), recomputes=recomputes))
    if nz == 0:
        return x, nz
    c = np.array(g, dtype=np.float64).reshape(6).copy()
    for k in range(nz):
        tau = hc[k]
        if n - k == 1:
            c[k] *= (1.0 - tau)
            continue
        if tau == 0.0:
            continue
        t = float(np.sum(A[k + 1:, k] * c[k + 1:])) + c[k]
        c[k] -= tau * t
        c[k + 1:] -= tau * A[k + 1:, k] * t
    for i in range(nz - 1, -1, -1):
        if c[i] != 0.0:
            c[i] /= A[i, i]
            c[:i] -= c[i] * A[:i, i]
    for i in range(n):
        x[perm[i]] = c[i] if i < nz else 0.0
    return x, nz


def lu_inverse(H, log=None):
    """Eigen's Matrix6d::inverse() = PartialPivLU(H).inverse(): partial pivoting (first largest |a|), no division when the
    pivot column is zero; a zero pivot gives inf / NaN entries, as in Eigen.  log: a list that receives one
    dict(swaps=[p - k: how far below row k its pivot row lay], zero_pivot=a pivot column was zero) per call."""
    A = np.array(H, dtype=np.float64).reshape(6, 6).copy()
    n = 6
    perm = []
    zero_pivot = False
    with np.errstate(all="ignore"):
        for k in range(n):
            p = k + int(np.argmax(np.abs(A[k:, k]))) if not np.isnan(A[k:, k]).any() else k
            big = abs(A[p, k])
            perm.append(p)
            if big != 0.0:
                if p != k:
                    A[[k, p]] = A[[p, k]]
                A[k + 1:, k] /= A[k, k]
            else:
                zero_pivot = True
            A[k + 1:, k + 1:] -= np.outer(A[k + 1:, k], A[k, k + 1:])
        inv = np.zeros((n, n))
        for col in range(n):
            b = np.zeros(n)
            b[col] = 1.0
            for k in range(n):
                b[k], b[perm[k]] = b[perm[k]], b[k]
            for i in range(n):
                b[i] -= float(np.dot(A[i, :i], b[:i]))
            for i in range(n - 1, -1, -1):
                b[i] = (b[i] - float(np.dot(A[i, i + 1:], b[i + 1:]))) / A[i, i]
            inv[:, col] = b
    if log is not None:
        log.append(dict(swaps=[int(p - k) for k, p in enumerate(perm)], zero_pivot=zero_pivot))
    return inv


def cov_max_eig(H, log=None):
    """DT_cov = H.inverse(); SelfAdjointEigenSolver(DT_cov).eigenvalues()(5) (:3880-3884; the solver reads the lower
    triangle).  NaN when the inverse is not finite."""
    inv = lu_inverse(H, log)
    if not np.isfinite(inv).all():
        return float("nan")
    return float(np.linalg.eigvalsh(inv, UPLO="L")[-1])


def point_residuals(cam, T, P, pl_obs):
    """||err_i|| of :3600-3603 / :3728 at T (vectorised; the oracle's row order)"""
    G = P @ T[:3, :3].T + T[:3, 3]
    u = cam.cx + cam.fx * G[:, 0] / G[:, 2]
    v = cam.cy + cam.fy * G[:, 1] / G[:, 2]
    dx, dy = u - pl_obs[:, 0], v - pl_obs[:, 1]
    return np.sqrt(dx * dx + dy * dy)


def line_residuals(cam, T, sPeP, le_obs):
    """||err_i|| of :3631-3640 / :3750"""
    out = []
    for end in (0, 3):
        G = sPeP[:, end:end + 3] @ T[:3, :3].T + T[:3, 3]
        u = cam.cx + cam.fx * G[:, 0] / G[:, 2]
        v = cam.cy + cam.fy * G[:, 1] / G[:, 2]
        out.append(le_obs[:, 0] * u + le_obs[:, 1] * v + le_obs[:, 2])
    return np.sqrt(out[0] * out[0] + out[1] * out[1])


def relpose_robust_gn(prm, cam, P, pl_obs, sPeP, le_obs, accumulate=None, log=None):
    """computeRelativePoseRobustGN (:3566-3957) on lc_points (P, pl_obs) / lc_lines (sPeP, le_obs), all inlier on entry.
    `accumulate(T, pt_inl, ls_inl) -> (H, g, e_sum, (N_p, N_l))` defaults to the oracle's C restatement of :3595-3689.
    log: a dict whose lists "qr" and "lu" receive what colpiv_qr_solve and lu_inverse report, in call order."""
    P, pl_obs = np.asarray(P, np.float64).reshape(-1, 3), np.asarray(pl_obs, np.float64).reshape(-1, 2)
    sPeP, le_obs = np.asarray(sPeP, np.float64).reshape(-1, 6), np.asarray(le_obs, np.float64).reshape(-1, 3)
    pt_inl = np.ones(P.shape[0], np.uint8)
    ls_inl = np.ones(sPeP.shape[0], np.uint8)
    ocam = O.make_cam(cam.fx, cam.fy, cam.cx, cam.cy)
    th = prm["homog_th"]
    if accumulate is None:
        def accumulate(T, pi, li):
            return O.pose_gn_accumulate(ocam, th, T, P, pl_obs, pi, sPeP, le_obs, li)
    T = np.eye(4)                                         # :3573
    H, g, e = np.zeros((6, 6)), np.zeros(6), 0.0          # :3575-3580
    err_prev = 999999999.9                                # :3583 -- once, for both stages
    trace, iters, stops = [], [0, 0], [None, None]
    res_at_outlier_pass = (np.zeros(0), np.zeros(0))
    for stage in (0, 1):
        for _ in range(prm["max_iters"] if stage == 0 else prm["max_iters_ref"]):
            H, g, e_sum, (n_p, n_l) = accumulate(T, pt_inl, ls_inl)
            iters[stage] += 1
            with np.errstate(divide="ignore", invalid="ignore"):
                e = float(np.float64(e_sum) / np.float64(n_l + n_p))       # :3679 e /= (N_l + N_p)
            trace.append(dict(stage=stage, T=T.copy(), H=H.copy(), g=g.copy(), e=e, n=(n_p, n_l), err_prev=err_prev))
            if abs(e - err_prev) < EPS or e < EPS:                       # :3682
                stops[stage] = "err_change" if abs(e - err_prev) < EPS else "err_small"
                break
            x, _ = colpiv_qr_solve(H, g, None if log is None else log.setdefault("qr", []))    # :3686-3687
            T = T @ O.inverse_se3(O.expmap_se3(x))                       # :3688
            trace[-1]["x"] = x
            if math.sqrt(float(np.sum(x * x))) < EPS:                    # :3691
                stops[stage] = "x_small"
                break
            err_prev = e                                                 # :3695
        if stage == 0:                                                   # :3721-3757
            rp = point_residuals(ocam, T, P[pt_inl > 0], pl_obs[pt_inl > 0])
            rl = line_residuals(ocam, T, sPeP[ls_inl > 0], le_obs[ls_inl > 0])
            res_at_outlier_pass = (point_residuals(ocam, T, P, pl_obs), line_residuals(ocam, T, sPeP, le_obs))
            pt_inl[np.flatnonzero(pt_inl)[rp > CHI]] = 0
            ls_inl[np.flatnonzero(ls_inl)[rl > CHI]] = 0
    x_inc = O.logmap_se3(T)                                             # :3874
    ok_res = e < prm["lc_res"]                                           # :3879
    eig = cov_max_eig(H, None if log is None else log.setdefault("lu", []))              # :3881-3885
    ok_unc = eig < prm["lc_unc"]
    N = P.shape[0] + sPeP.shape[0]
    n_inl = int(pt_inl.sum()) + int(ls_inl.sum())
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio_inl = float(np.float64(n_inl) / np.float64(N))             # :3900
    ok_inl = ratio_inl > prm["lc_inl"]                                   # :3901 (then :3903 lc_inl = true)
    t = math.sqrt(float(np.sum(x_inc[:3] * x_inc[:3])))                 # :3906
    r = math.sqrt(float(np.sum(x_inc[3:] * x_inc[3:]))) * 180.0 / CV_PI  # :3907
    ok_trs, ok_rot = t < prm["lc_trs"], r < prm["lc_rot"]
    is_lc = bool(ok_res and ok_unc and ok_trs and ok_rot)                # :3912
    pose_inc = O.logmap_se3(O.inverse_se3(O.expmap_se3(x_inc))) if is_lc else np.zeros(6)   # :3948
    return dict(is_lc=int(is_lc), gn_ran=1, iters_1=iters[0], iters_2=iters[1], stops=stops, e=e, cov_eig=eig,
                ratio_inliers=ratio_inl, t=t, r=r, ok_res=int(ok_res), ok_unc=int(ok_unc), ok_inl=int(ok_inl),
                ok_trs=int(ok_trs), ok_rot=int(ok_rot), x_inc=x_inc, T_inc=T, pose_inc=pose_inc, H=H, g=g,
                pt_inlier=pt_inl.astype(bool), ls_inlier=ls_inl.astype(bool), n_pt_inliers=int(pt_inl.sum()),
                n_ls_inliers=int(ls_inl.sum()), trace=trace, res_at_outlier_pass=res_at_outlier_pass)


def correspondences(m12, idx0, idx1):
    """:3225-3241 / :3251-3268: rows (kf0 idx, i1, kf1 idx, i2) in i1 order"""
    i1 = np.flatnonzero(np.asarray(m12) >= 0)
    i2 = np.asarray(m12)[i1]
    a = np.full(i1.shape[0], -1, np.int32) if idx0 is None else np.asarray(idx0, np.int32)[i1]
    b = np.full(i1.shape[0], -1, np.int32) if idx1 is None else np.asarray(idx1, np.int32)[i2]
    return np.stack([a, i1, b, i2], axis=1).astype(np.int32).reshape(-1, 4)


def is_loop_closure(prm, cam, kf0, kf1, log=None):
    """isLoopClosure(kf0, kf1) (:3192-3300) -> dict (the fields of plslam_lc_result, the correspondence rows and masks, the
    match tables, and the GN trace).  log: see relpose_robust_gn"""
    out = {}
    n_pt_0, n_pt_1 = len(kf0["P"]), len(kf1["P"])
    n_ls_0, n_ls_1 = len(kf0["sPeP"]), len(kf1["sPeP"])
    m12p = np.full(n_pt_0, -1, np.int32)
    m12l = np.full(n_ls_0, -1, np.int32)
    common_pt = common_ls = 0
    if prm["has_points"] and n_pt_1 and n_pt_0:                         # :3220-3223
        m12p, common_pt = O.match(kf0["pdesc"], kf1["pdesc"], prm["min_ratio_12_p"], bool(prm["mutual"]))
    if prm["has_lines"] and n_ls_1 and n_ls_0:                          # :3246-3249
        m12l, common_ls = O.match(kf0["ldesc"], kf1["ldesc"], prm["min_ratio_12_l"], bool(prm["mutual"]))
    pc = correspondences(m12p, kf0.get("pt_idx"), kf1.get("pt_idx"))
    lc = correspondences(m12l, kf0.get("ls_idx"), kf1.get("ls_idx"))
    assert pc.shape[0] == common_pt and lc.shape[0] == common_ls
    inl_pt = std_max(ratio(common_pt, n_pt_0), ratio(common_pt, n_pt_1))   # :3273
    inl_ls = std_max(ratio(common_ls, n_ls_0), ratio(common_ls, n_ls_1))   # :3274
    th = prm["lc_inlier_ratio"]
    if prm["has_points"] and prm["has_lines"]:                              # :3277-3291
        cond = inl_pt > th and inl_ls > th
    elif prm["has_points"]:
        cond = inl_pt > th
    elif prm["has_lines"]:
        cond = inl_ls > th
    else:
        cond = False
    out.update(m12_p=m12p, m12_l=m12l, common_pt=int(common_pt), common_ls=int(common_ls), inl_ratio_pt=inl_pt,
               inl_ratio_ls=inl_ls, pt_corr=pc, ls_corr=lc)
    if not cond:                                                            # :3298-3299
        out.update(is_lc=0, gn_ran=0, pt_inlier=np.ones(common_pt, bool), ls_inlier=np.ones(common_ls, bool),
                   n_pt_inliers=common_pt, n_ls_inliers=common_ls, iters_1=0, iters_2=0, trace=[])
        return out
    P = np.asarray(kf0["P"], np.float64).reshape(-1, 3)[pc[:, 1]]
    pl = np.asarray(kf1["pl"], np.float64).reshape(-1, 2)[pc[:, 3]]
    S = np.asarray(kf0["sPeP"], np.float64).reshape(-1, 6)[lc[:, 1]]
    le = np.asarray(kf1["le"], np.float64).reshape(-1, 3)[lc[:, 3]]
    out.update(relpose_robust_gn(prm, cam, P, pl, S, le, log=log))
    out["corr_inputs"] = (P, pl, S, le)
    return out


def reference_outputs(r):
    """what the reference leaves in lc_pt_idx / lc_ls_idx (:3914-3946): the inlier rows if a loop closure, all otherwise"""
    if r["is_lc"]:
        return r["pt_corr"][r["pt_inlier"]], r["ls_corr"][r["ls_inlier"]]
    return r["pt_corr"], r["ls_corr"]


# ---- the first Gauss-Newton system in long double ------------------------------------------------------------------------
LD = np.longdouble


def _jac6_ld(fgz2, a, b, gx, gy, gz):
    return np.array([+fgz2 * a * gz, +fgz2 * b * gz, -fgz2 * (gx * a + gy * b),
                     -fgz2 * (gx * gy * a + gy * gy * b + gz * gz * b), +fgz2 * (gx * gx * a + gz * gz * a + gx * gy * b),
                     +fgz2 * (gx * gz * b - gy * gz * a)], LD)


def first_system_ld(cam, th, P, pl, S, le, with_scale=False):
    """H, g and e of the first iteration (:3595-3689 at T_inc = I, every row an inlier) in np.longdouble (64-bit mantissa on
    x86-64), row by row as the source writes them: a point's err = project(P) - pl_obs, a line's err = (l . sp, l . ep), the
    Jacobian of ||err|| with gz^2 and ||err|| clamped from below by std::max(homog_th, .), Cauchy weight 1 / (1 + ||err||^2),
    H += J J^T w, g += J ||err|| w, e += ||err||^2 w, and e /= N_l + N_p (:3679) -- what plslam_lc_result holds in H, g, e
    after max_iters = 1, max_iters_ref = 0.  with_scale: also (sum of |term| per entry of H, of g): the scale of the rounding
    error of any fp64 summation order of these terms."""
    th = LD(th)
    fx, fy, cx, cy = LD(cam.fx), LD(cam.fy), LD(cam.cx), LD(cam.cy)
    H, g, e = np.zeros((6, 6), LD), np.zeros(6, LD), LD(0)
    Ha, ga = np.zeros((6, 6), LD), np.zeros(6, LD)
    P, pl = np.asarray(P, np.float64).reshape(-1, 3).astype(LD), np.asarray(pl, np.float64).reshape(-1, 2).astype(LD)
    S, le = np.asarray(S, np.float64).reshape(-1, 6).astype(LD), np.asarray(le, np.float64).reshape(-1, 3).astype(LD)

    def clamp(x):                                   # std::max(th, x) = th < x ? x : th
        return x if th < x else th

    def fold(J, r):
        nonlocal H, g, e, Ha, ga
        w = LD(1) / (LD(1) + r * r)
        H += np.outer(J, J) * w
        g += J * r * w
        e += r * r * w
        Ha += np.abs(np.outer(J, J) * w)
        ga += np.abs(J * r * w)

    for X, o in zip(P, pl):
        dx, dy = cx + fx * X[0] / X[2] - o[0], cy + fy * X[1] / X[2] - o[1]
        r = np.sqrt(dx * dx + dy * dy)
        fold(_jac6_ld(fx / clamp(X[2] * X[2]), dx, dy, X[0], X[1], X[2]) / clamp(r), r)
    for Q, l in zip(S, le):
        A, B = Q[:3], Q[3:]
        ds = l[0] * (cx + fx * A[0] / A[2]) + l[1] * (cy + fy * A[1] / A[2]) + l[2]
        de = l[0] * (cx + fx * B[0] / B[2]) + l[1] * (cy + fy * B[1] / B[2]) + l[2]
        r = np.sqrt(ds * ds + de * de)
        Js = _jac6_ld(fx / clamp(A[2] * A[2]), l[0], l[1], A[0], A[1], A[2])
        Je = _jac6_ld(fx / clamp(B[2] * B[2]), l[0], l[1], B[0], B[1], B[2])
        fold((Js * ds + Je * de) / clamp(r), r)
    with np.errstate(divide="ignore", invalid="ignore"):
        e = e / LD(P.shape[0] + S.shape[0])
    return (H, g, e, (Ha, ga)) if with_scale else (H, g, e)


def system_distance(H, g, e, ld):
    """How far an fp64 first system (H, g, e) lies from first_system_ld(..., with_scale=True): the largest
    |entry - long double| / sum of |term| over the entries of H and g, and |e - long double| / e (e's terms are positive)"""
    Hl, gl, el, (Ha, ga) = ld
    with np.errstate(divide="ignore", invalid="ignore"):
        d = np.concatenate([(np.abs(np.asarray(H, np.float64).reshape(6, 6).astype(LD) - Hl) / Ha).ravel(),
                            np.abs(np.asarray(g, np.float64).reshape(6).astype(LD) - gl) / ga, [abs(LD(e) - el) / el]])
    d = np.where(np.isnan(d), LD(0), d)             # 0 / 0: an entry without a term (H = 0 of a pair at rest)
    return float(np.max(d))


def dmax_sides(cam, th, T, P, pl_obs, sPeP, le_obs):
    """Which argument std::max(homog_th, .) returns in the rows of one system at T: per call site the number of rows that
    take (homog_th, the computed value) -- gz^2 of a point (:3607), gz^2 of a line's end points, ||err|| of a point (:3617),
    ||err|| of a line"""
    T = np.asarray(T, np.float64).reshape(4, 4)
    G = P @ T[:3, :3].T + T[:3, 3]
    ends = np.concatenate([sPeP[:, e:e + 3] @ T[:3, :3].T + T[:3, 3] for e in (0, 3)])
    rp, rl = point_residuals(cam, T, P, pl_obs), line_residuals(cam, T, sPeP, le_obs)

    def sides(v):
        return int(np.sum(~(th < v))), int(np.sum(th < v))

    return dict(pt_z2=sides(G[:, 2] * G[:, 2]), ls_z2=sides(ends[:, 2] * ends[:, 2]), pt_r=sides(rp), ls_r=sides(rl))
