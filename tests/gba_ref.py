"""A numpy restatement of MapHandler::levMarquardtOptimizationGBA (src/mapHandler.cpp:2101-2703), quirks included, written
for the tests of plslam_gba_optimize.  DESIGN.md section 5 lists the findings it rests on; tests/test_gba_cpu.py pins each one
to the reference's text and its first pass to the reference's own loops (oracle/).

  * err is divided by Npt_obs + Nls_obs, which stay 0 (:2121, :2230, :2356, :2635): +inf, or NaN for a zero sum.  The first
    pass's err is the sum from 0 (the reference leaves that double uninitialised, :2116).
  * Hmax is an int (:2359): lambda_0 = lambda_lba_lm * trunc(max |H(i,i)|).
  * The stops compare with numeric_limits<double>::epsilon() (:2637, :2667).
  * The first pass reads the stored T_kf_w everywhere and writes the pose x line cross blocks transposed into both triangles
    (:2349-2350); the iteration passes give points the estimate expmap_se3(X) of an optimised keyframe (:2411-2416) and lines the
    stored pose, both end points from the stride-3 block (:2520-2523), with the correct block in the lower triangle (:2628-2629).
    SimplicialLDLT reads the lower triangle only, so W below is always "the lower block as the pass writes it".
  * The solve is the Schur complement on the keyframe blocks and a blocked dense L D L^T of the reduced system; a landmark block
    that is not positive definite after damping (an unpivoted Gauss-Jordan meets a pivot <= 0) contributes nothing and gets a
    zero step -- the device's documented policy, where the reference's full-system LDL^T would carry non-finite values.

What is checked against something that is not this file: the first pass against the reference's own loops; schur_solve (both
pass kinds, on the arc and on the ragged / gapped / tumbling inputs of tests/gba_cases.py) against a Gaussian elimination of the
whole damped system in long double (tests/gba_dense.py, test_gba_cpu.py); expmap_se3 / logmap_se3 against the full formulas in
long double on both sides of their 1e-6 thresholds and at theta = 2.8.  The rows of the iteration pass and the LM schedule rest
on the reference's text alone."""
from __future__ import annotations

import numpy as np

EPS = np.finfo(np.float64).eps


# ---- stvo-pl's SE(3) maps (auxiliar.cpp), restated as the device does (plslam_amd/csrc/se3_dev.hpp) -----------------------
def _skew(w):
    return np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])


def expmap_se3(x):
    x = np.asarray(x, np.float64)
    T = np.eye(4)
    R, t = np.eye(3), x[:3].copy()
    theta = np.sqrt(x[3] * x[3] + x[4] * x[4] + x[5] * x[5])
    if not theta < 0.000001:
        s = _skew(x[3:] / theta)
        s2 = s @ s
        R = np.eye(3) + s * np.sin(theta) + s2 * (1.0 - np.cos(theta))
        V = np.eye(3) + s * (1.0 - np.cos(theta)) / theta + s2 * (theta - np.sin(theta)) / theta
        t = V @ x[:3]
    T[:3, :3], T[:3, 3] = R, t
    return T


def inverse_se3(T):
    o = np.eye(4)
    o[:3, :3] = T[:3, :3].T
    o[:3, 3] = -T[:3, :3].T @ T[:3, 3]
    return o


def logmap_se3(T):
    R = T[:3, :3]
    # the clamps as comparisons, as the device and the C oracle write them: a NaN passes through both, theta is NaN, the
    # test below fails and w stays 0 (Python's min / max would turn the NaN into -1, theta into pi and w into NaN)
    cosine = (R[0, 0] + R[1, 1] + R[2, 2] - 1.0) / 2.0
    cosine = 1.0 if cosine > 1.0 else -1.0 if cosine < -1.0 else cosine
    sine = np.sqrt(1.0 - cosine * cosine)
    sine = 1.0 if sine > 1.0 else -1.0 if sine < -1.0 else sine
    theta = np.arccos(cosine)
    w, V = np.zeros(3), np.eye(3)
    if theta > 0.000001:
        w = theta * np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]]) / (2.0 * sine)
        s = _skew(w / theta)
        V = np.eye(3) + s * (1.0 - cosine) / theta + s @ s * (theta - sine) / theta
    Vi = V if np.linalg.det(V) == 0.0 else np.linalg.inv(V)
    return np.concatenate([Vi @ T[:3, 3], w])


# ---- the rows (:2124-2228 points, :2233-2355 lines; the iteration pass :2400-2635) ----------------------------------------
def point_rows(cam, th, T, X, uv):
    """T (n, 4, 4) poses, X (n, 3), uv (n, 2) -> J_T (n, 6), J_X (n, 3), r (n,), w (n,)"""
    Ti = np.stack([inverse_se3(t) for t in T]) if T.shape[0] else T
    Xc = np.einsum("nab,nb->na", Ti[:, :3, :3], X) + Ti[:, :3, 3]
    gx, gy, gz = Xc[:, 0], Xc[:, 1], Xc[:, 2]
    prj = np.stack([cam.cx + cam.fx * gx / gz, cam.cy + cam.fy * gy / gz], 1)
    e = uv - prj
    r = np.sqrt(e[:, 0] ** 2 + e[:, 1] ** 2)
    gz2 = 1.0 / np.maximum(th, gz * gz)
    fxdx, fydy = cam.fx * e[:, 0], cam.fy * e[:, 1]
    J = np.stack([gz2 * fxdx * gz, gz2 * fydy * gz, -gz2 * (fxdx * gx + fydy * gy),
                  -gz2 * (fxdx * gx * gy + fydy * gy * gy + fydy * gz * gz),
                  gz2 * (fxdx * gx * gx + fxdx * gz * gz + fydy * gx * gy), gz2 * (fydy * gx * gz - fxdx * gy * gz)], 1)
    den = np.maximum(th, r)[:, None]
    JX = np.einsum("na,nab->nb", J[:, :3], Ti[:, :3, :3]) / den
    return J / den, JX, r, 1.0 / (1.0 + r * r)


def line_rows(cam, th, T, P, Q, l):
    Ti = np.stack([inverse_se3(t) for t in T]) if T.shape[0] else T
    R3, t3 = Ti[:, :3, :3], Ti[:, :3, 3]
    Pc = np.einsum("nab,nb->na", R3, P) + t3
    Qc = np.einsum("nab,nb->na", R3, Q) + t3
    pp = np.stack([cam.cx + cam.fx * Pc[:, 0] / Pc[:, 2], cam.cy + cam.fy * Pc[:, 1] / Pc[:, 2]], 1)
    qq = np.stack([cam.cx + cam.fx * Qc[:, 0] / Qc[:, 2], cam.cy + cam.fy * Qc[:, 1] / Qc[:, 2]], 1)
    e0 = l[:, 0] * pp[:, 0] + l[:, 1] * pp[:, 1] + l[:, 2]
    e1 = l[:, 0] * qq[:, 0] + l[:, 1] * qq[:, 1] + l[:, 2]
    r = np.sqrt(e0 * e0 + e1 * e1)
    fxlx, fyly = cam.fx * e0, cam.fy * e1
    den = np.maximum(th, r)

    def jac(G):
        gx, gy, gz = G[:, 0], G[:, 1], G[:, 2]
        gz2 = 1.0 / np.maximum(th, gz * gz)
        return np.stack([gz2 * fxlx * gz, gz2 * fyly * gz, -gz2 * (fxlx * gx + fyly * gy),
                         -gz2 * (fxlx * gx * gy + fyly * gy * gy + fyly * gz * gz),
                         gz2 * (fxlx * gx * gx + fxlx * gz * gz + fyly * gx * gy), gz2 * (fyly * gx * gz - fxlx * gy * gz)], 1)
    JP, JQ = jac(Pc), jac(Qc)
    JLp = np.einsum("na,nab->nb", JP[:, :3], R3) * e0[:, None] / den[:, None]
    JLq = np.einsum("na,nab->nb", JQ[:, :3], R3) * e1[:, None] / den[:, None]
    JT = (JP * e0[:, None] + JQ * e1[:, None]) / den[:, None]
    return JT, np.concatenate([JLp, JLq], 1), r, 1.0 / (1.0 + r * r)


class Problem:
    """The lists of globalBundleAdjustment (:1995-2099) as the plan takes them."""

    def __init__(self, cam, m, homog_th=1e-7):
        self.cam, self.th = cam, homog_th
        self.n_map, self.nkf = int(m["n_map_kf"]), len(m["kf_list"])
        self.npt, self.nls = int(m["npt"]), int(m["nls"])
        self.kf_list = np.asarray(m["kf_list"])
        self.T_map = np.asarray(m["T_kf_w"], np.float64).reshape(-1, 4, 4)
        po, lo = np.asarray(m["pt_obs"]).reshape(-1, 6), np.asarray(m["ls_obs"]).reshape(-1, 6)
        self.p_lm, self.p_map, self.p_kf = po[:, 1], po[:, 3], po[:, 4]
        self.l_lm, self.l_map, self.l_kf = lo[:, 1], lo[:, 3], lo[:, 4]
        self.uv = np.asarray(m["pt_uv"], np.float64).reshape(-1, 2)
        self.l = np.asarray(m["ls_l"], np.float64).reshape(-1, 3)

    def blocks(self, first, x_kf, Xw, Lw):
        """One pass's block-form normal equations (lower blocks as the pass writes them)."""
        nkf = self.nkf
        if first:
            Tp = self.T_map[self.p_map]
            P, Q = Lw[self.l_lm, :3], Lw[self.l_lm, 3:]
        else:
            Test = np.stack([expmap_se3(x) for x in x_kf]) if nkf else np.zeros((0, 4, 4))
            Tp = np.where((self.p_kf >= 0)[:, None, None], Test[np.maximum(self.p_kf, 0)], self.T_map[self.p_map])
            flat = Lw.reshape(-1)
            P = np.stack([flat[3 * self.l_lm + i] for i in range(3)], 1) if len(self.l_lm) else np.zeros((0, 3))
            Q = P.copy()
        Tl = self.T_map[self.l_map]
        pJT, pJX, pr, pw = point_rows(self.cam, self.th, Tp, Xw[self.p_lm], self.uv)
        lJT, lJL, lr, lw = line_rows(self.cam, self.th, Tl, P, Q, self.l)
        B = dict(Hp=np.zeros((nkf, 6, 6)), gp=np.zeros((nkf, 6)), Hpt=np.zeros((self.npt, 3, 3)), gpt=np.zeros((self.npt, 3)),
                 Hls=np.zeros((self.nls, 6, 6)), gls=np.zeros((self.nls, 6)))
        po, lo = self.p_kf >= 0, self.l_kf >= 0
        np.add.at(B["Hp"], self.p_kf[po], np.einsum("na,nb->nab", pJT, pJT)[po] * pw[po, None, None])
        np.add.at(B["gp"], self.p_kf[po], (pJT * pr[:, None])[po] * pw[po, None])
        np.add.at(B["Hpt"], self.p_lm, np.einsum("na,nb->nab", pJX, pJX) * pw[:, None, None])
        np.add.at(B["gpt"], self.p_lm, pJX * pr[:, None] * pw[:, None])
        np.add.at(B["Hp"], self.l_kf[lo], np.einsum("na,nb->nab", lJT, lJT)[lo] * lw[lo, None, None])
        np.add.at(B["gp"], self.l_kf[lo], (lJT * lr[:, None])[lo] * lw[lo, None])
        np.add.at(B["Hls"], self.l_lm, np.einsum("na,nb->nab", lJL, lJL) * lw[:, None, None])
        np.add.at(B["gls"], self.l_lm, lJL * lr[:, None] * lw[:, None])
        B["Wpt"] = np.einsum("nx,na->nxa", pJX, pJT) * pw[:, None, None] * po[:, None, None]
        if first:    # :2349-2350: H(line x, pose a) = J_L[a] J_T[x] w
            B["Wls"] = np.einsum("na,nx->nxa", lJL, lJT) * lw[:, None, None] * lo[:, None, None]
        else:        # :2629: the lower triangle holds J_L[x] J_T[a] w
            B["Wls"] = np.einsum("nx,na->nxa", lJL, lJT) * lw[:, None, None] * lo[:, None, None]
        B["err"] = float(np.sum(pr * pr * pw) + np.sum(lr * lr * lw))
        return B

    def full_H(self, B):
        """The dense H and g the pass assembles (both triangles symmetric: the first pass, or the lower triangle mirrored)."""
        nkf, npt, nls = self.nkf, self.npt, self.nls
        N = 6 * nkf + 3 * npt + 6 * nls
        H, g = np.zeros((N, N)), np.zeros(N)
        for k in range(nkf):
            H[6 * k:6 * k + 6, 6 * k:6 * k + 6] = B["Hp"][k]
        g[:6 * nkf] = B["gp"].reshape(-1)
        b0 = 6 * nkf
        for j in range(npt):
            H[b0 + 3 * j:b0 + 3 * j + 3, b0 + 3 * j:b0 + 3 * j + 3] = B["Hpt"][j]
        g[b0:b0 + 3 * npt] = B["gpt"].reshape(-1)
        b1 = b0 + 3 * npt
        for j in range(nls):
            H[b1 + 6 * j:b1 + 6 * j + 6, b1 + 6 * j:b1 + 6 * j + 6] = B["Hls"][j]
        g[b1:] = B["gls"].reshape(-1)
        for o in np.flatnonzero(self.p_kf >= 0):
            r, c = b0 + 3 * self.p_lm[o], 6 * self.p_kf[o]
            H[r:r + 3, c:c + 6] += B["Wpt"][o]
            H[c:c + 6, r:r + 3] += B["Wpt"][o].T
        for o in np.flatnonzero(self.l_kf >= 0):
            r, c = b1 + 6 * self.l_lm[o], 6 * self.l_kf[o]
            H[r:r + 6, c:c + 6] += B["Wls"][o]
            H[c:c + 6, r:r + 6] += B["Wls"][o].T
        return H, g


def gauss_jordan_inv(A):
    """(n, d, d) -> (inverse, ok): unpivoted Gauss-Jordan; ok = every pivot > 0 (the device's landmark policy)"""
    A = A.copy()
    n, d, _ = A.shape
    I = np.broadcast_to(np.eye(d), A.shape).copy()
    ok = np.ones(n, bool)
    for c in range(d):
        piv = A[:, c, c].copy()
        ok &= piv > 0.0
        ip = 1.0 / np.where(piv > 0.0, piv, 1.0)
        A[:, c, :] *= ip[:, None]
        I[:, c, :] *= ip[:, None]
        for a in range(d):
            if a == c:
                continue
            f = A[:, a, c].copy()
            A[:, a, :] -= f[:, None] * A[:, c, :]
            I[:, a, :] -= f[:, None] * I[:, c, :]
    I[~ok] = 0.0
    return I, ok


def ldlt_solve(S, b, nb=64):
    """Blocked right-looking L D L^T of the LOWER triangle of S, then L y = b, z = y / d, L^T x = z -> (x, bad pivots)."""
    n = S.shape[0]
    A = np.tril(S) + np.tril(S, -1).T
    L, d, bad = np.eye(n), np.zeros(n), 0
    for k0 in range(0, n, nb):
        k1 = min(n, k0 + nb)
        for j in range(k0, k1):
            dj = A[j, j]
            if not (dj != 0.0 and np.isfinite(dj)):
                bad += 1
            d[j] = dj
            l = A[j + 1:k1, j] / dj
            L[j + 1:k1, j] = l
            A[j + 1:k1, j + 1:k1] -= np.outer(l, l * dj)
        if k1 < n:
            X = np.linalg.solve(L[k0:k1, k0:k1], A[k1:, k0:k1].T).T
            L[k1:, k0:k1] = X / d[k0:k1]
            A[k1:, k1:] -= X @ L[k1:, k0:k1].T
    y = np.zeros(n)
    for k0 in range(0, n, nb):
        k1 = min(n, k0 + nb)
        y[k0:k1] = np.linalg.solve(L[k0:k1, k0:k1], b[k0:k1] - L[k0:k1, :k0] @ y[:k0])
    z = y / d
    x = np.zeros(n)
    for k1 in range(n, 0, -nb):
        k0 = max(0, k1 - nb)
        x[k0:k1] = np.linalg.solve(L[k0:k1, k0:k1].T, z[k0:k1] - L[k1:, k0:k1].T @ x[k1:])
    return x, bad


def schur_solve(P, B, lam):
    """The damped solve of one pass by Schur complement -> dict(dp (6 nkf), dx_pt (npt, 3), dx_ls (nls, 6), S, b, n_singular,
    n_bad)."""
    nkf = P.nkf

    def damp(H):
        d = np.einsum("nii->ni", H)
        Hd = H.copy()
        idx = np.arange(H.shape[1])
        Hd[:, idx, idx] = d + lam * d
        return Hd
    Vp, okp = gauss_jordan_inv(damp(B["Hpt"])) if P.npt else (np.zeros((0, 3, 3)), np.ones(0, bool))
    Vl, okl = gauss_jordan_inv(damp(B["Hls"])) if P.nls else (np.zeros((0, 6, 6)), np.ones(0, bool))
    S4 = np.zeros((nkf, nkf, 6, 6))
    Hp = damp(B["Hp"])
    for k in range(nkf):
        S4[k, k] = Hp[k]
    b = B["gp"].copy()
    for lm, kf, W, V, g in ((P.p_lm, P.p_kf, B["Wpt"], Vp, B["gpt"]), (P.l_lm, P.l_kf, B["Wls"], Vl, B["gls"])):
        sel = np.flatnonzero(kf >= 0)
        if sel.size == 0:
            continue
        Y = np.einsum("nxy,nya->nxa", V[lm[sel]], W[sel])
        t = np.einsum("nxy,ny->nx", V[lm[sel]], g[lm[sel]])
        np.add.at(b, kf[sel], -np.einsum("nxa,nx->na", W[sel], t))
        order = np.argsort(lm[sel], kind="stable")
        s2 = sel[order]
        lms = lm[s2]
        starts = np.flatnonzero(np.r_[True, lms[1:] != lms[:-1]])
        i1, i2 = [], []
        for a, e in zip(starts, np.r_[starts[1:], lms.size]):
            idx = order[a:e]
            i1.append(np.repeat(idx, idx.size))
            i2.append(np.tile(idx, idx.size))
        i1, i2 = np.concatenate(i1), np.concatenate(i2)
        C = np.einsum("pxa,pxb->pab", W[sel][i1], Y[i2])
        np.add.at(S4, (kf[sel][i1], kf[sel][i2]), -C)
    S = S4.transpose(0, 2, 1, 3).reshape(6 * nkf, 6 * nkf)
    dp, bad = ldlt_solve(S, b.reshape(-1))
    dpk = dp.reshape(nkf, 6)
    out = dict(dp=dp, S=S, b=b.reshape(-1), n_bad=bad, n_singular=int((~okp).sum() + (~okl).sum()))
    for name, lm, kf, W, V, g in (("dx_pt", P.p_lm, P.p_kf, B["Wpt"], Vp, B["gpt"]), ("dx_ls", P.l_lm, P.l_kf, B["Wls"], Vl,
                                                                                       B["gls"])):
        rhs = g.copy()
        sel = np.flatnonzero(kf >= 0)
        np.add.at(rhs, lm[sel], -np.einsum("nxa,na->nx", W[sel], dpk[kf[sel]]))
        out[name] = np.einsum("nxy,ny->nx", V, rhs)
    return out


def one_step(P, first, x_kf, Xw, Lw, lam):
    """One accepted solve from the given state -> (x_kf, Xw, Lw after it, the reduced matrix S of the solve)."""
    x = np.array(x_kf, np.float64).reshape(-1, 6).copy()
    B = P.blocks(first, x, np.asarray(Xw).reshape(-1, 3), np.asarray(Lw).reshape(-1, 6))
    s = schur_solve(P, B, lam)
    dp = s["dp"].reshape(-1, 6)
    for k in range(P.nkf):
        x[k] = logmap_se3(expmap_se3(x[k]) @ inverse_se3(expmap_se3(dp[k])))
    return x, np.asarray(Xw).reshape(-1, 3) + s["dx_pt"], np.asarray(Lw).reshape(-1, 6) + s["dx_ls"], s["S"]


def gba_lm(P, x_kf, Xw, Lw, lambda_lm=0.00001, lambda_k=10.0, max_iters=15):
    """levMarquardtOptimizationGBA -> dict(trace (one dict per solve, with the state after it, its reduced matrix S and its
    pose step dp), iters, stop_reason, hmax, the final x_kf / T / Xw / Lw)."""
    x = np.array(x_kf, np.float64).reshape(-1, 6).copy()
    X = np.array(Xw, np.float64).reshape(-1, 3).copy()
    Lm = np.array(Lw, np.float64).reshape(-1, 6).copy()
    trace = []

    def solve(B, lam, err_raw, err, apply):
        s = schur_solve(P, B, lam)
        dp = s["dp"].reshape(-1, 6)
        if apply:
            for k in range(P.nkf):
                Tc = expmap_se3(x[k]) @ inverse_se3(expmap_se3(dp[k]))
                x[k] = logmap_se3(Tc)
            X[:] += s["dx_pt"]
            Lm[:] += s["dx_ls"]
        dxn = float(np.sqrt(np.sum(s["dp"] ** 2) + np.sum(s["dx_pt"] ** 2) + np.sum(s["dx_ls"] ** 2)))
        trace.append(dict(lam=lam, err_raw=err_raw, err=err, dx_norm=dxn, n_singular=s["n_singular"], n_bad_pivots=s["n_bad"],
                          accepted=apply, x_kf=x.copy(), Xw=X.copy(), Lw=Lm.copy(), S=s["S"], dp=dp.copy()))
        return dxn

    with np.errstate(divide="ignore", invalid="ignore"):
        B = P.blocks(True, x, X, Lm)
        diag = np.concatenate([np.einsum("nii->ni", B["Hp"]).reshape(-1), np.einsum("nii->ni", B["Hpt"]).reshape(-1),
                               np.einsum("nii->ni", B["Hls"]).reshape(-1)])
        a = np.abs(diag)
        hmax = float(a[~np.isnan(a)].max()) if np.any(~np.isnan(a)) else 0.0
        lam = lambda_lm * float(np.trunc(hmax))
        err = np.float64(B["err"]) / np.float64(0.0)
        solve(B, lam, B["err"], float(err), True)
        err_prev = err
        stop, iters = 0, 1
        while iters < max_iters:
            B = P.blocks(False, x, X, Lm)
            err = np.float64(B["err"]) / np.float64(0.0)
            if abs(err - err_prev) < EPS or err < EPS:
                stop = 1
                break
            accept = not (err > err_prev)
            dxn = solve(B, lam, B["err"], float(err), accept)
            lam = lam * lambda_k if accept else lam / lambda_k
            if dxn < EPS:
                stop = 2
                break
            err_prev = err
            iters += 1
    return dict(trace=trace, iters=iters, stop_reason=stop, hmax=hmax, lam=lam, x_kf=x, Xw=X, Lw=Lm,
                T=np.stack([expmap_se3(v) for v in x]))
