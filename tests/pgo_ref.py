"""A numpy restatement of MapHandler::loopClosureOptimizationCovGraphG2O (src/mapHandler.cpp:4185-4410) up to
loopClosureFuseLandmarks(), written for the tests of plslam_pgo_* and plslam_lc_correct_map.  DESIGN.md section 5 ("Loop-closure
pose graph") lists what it rests on.

The graph (:4198-4290) and the write-back (:4298-4398) follow the reference's text, which tests/test_pgo_cpu.py pins.  The
optimiser is g2o's (SparseOptimizer + OptimizationAlgorithmLevenberg, EdgeSE3 / VertexSE3), which is neither in the reference
tree nor vendored here: what follows restates g2o's published source from a reading of it.  Every constant and branch of that
reading sits in G2O below, so that it can be corrected in one place once g2o is at hand ("parity unpinned").

Isometries are (R 3 x 3, t 3).  The solve is a dense numpy solve of the damped system; a failed solve (a non-finite result)
takes a zero step and chi' = DBL_MAX, as g2o's failed Cholmod does."""
from __future__ import annotations

import sys
from collections import deque

import numpy as np

from gba_ref import expmap_se3, inverse_se3, logmap_se3

DBL_MAX = sys.float_info.max

# g2o as read, not pinned: every recalled constant of the optimiser
G2O = dict(
    exp_small_theta=1e-5,        # SE3Quat::exp: below it R = I + Omega + Omega^2 and V = R
    log_d_threshold=0.99999,     # SE3Quat::log: above it the first-order branch
    rho_denominator_eps=1e-3,    # OptimizationAlgorithmLevenberg: scale = dx.(lambda dx + b) + 1e-3
    good_step_lower=1.0 / 3.0,   # lambda *= max(1/3, min(1 - (2 rho - 1)^3, 2/3))
    good_step_upper=2.0 / 3.0,
    max_trials=10,               # maxTrialsAfterFailure
)


def reverse_se3(x):
    x = np.asarray(x, np.float64)
    return np.concatenate([x[3:], x[:3]])


# ---- Eigen quaternions ------------------------------------------------------------------------------------------------------
def quat_from_R(R):
    """Eigen's Quaternion(const Matrix3&) -> (w, x, y, z)."""
    tr = R[0, 0] + R[1, 1] + R[2, 2]
    q = np.zeros(4)
    if tr > 0.0:
        t = np.sqrt(tr + 1.0)
        q[0] = 0.5 * t
        t = 0.5 / t
        q[1] = (R[2, 1] - R[1, 2]) * t
        q[2] = (R[0, 2] - R[2, 0]) * t
        q[3] = (R[1, 0] - R[0, 1]) * t
    else:
        i = 0
        if R[1, 1] > R[0, 0]:
            i = 1
        if R[2, 2] > R[i, i]:
            i = 2
        j, k = (i + 1) % 3, (i + 2) % 3
        t = np.sqrt(R[i, i] - R[j, j] - R[k, k] + 1.0)
        q[1 + i] = 0.5 * t
        t = 0.5 / t
        q[0] = (R[k, j] - R[j, k]) * t
        q[1 + j] = (R[j, i] + R[i, j]) * t
        q[1 + k] = (R[k, i] + R[i, k]) * t
    return q


def unit_quat(R):
    """The normalised quaternion of R with w >= 0 (SE3Quat::normalizeRotation, toCompactQuaternion)."""
    q = quat_from_R(R)
    q = q / np.sqrt(q @ q)
    return -q if q[0] < 0.0 else q


def R_from_quat(q):
    """Eigen's toRotationMatrix."""
    w, x, y, z = q
    tx, ty, tz = 2.0 * x, 2.0 * y, 2.0 * z
    twx, twy, twz = tx * w, ty * w, tz * w
    txx, txy, txz = tx * x, ty * x, tz * x
    tyy, tyz, tzz = ty * y, tz * y, tz * z
    return np.array([[1.0 - (tyy + tzz), txy - twz, txz + twy],
                     [txy + twz, 1.0 - (txx + tzz), tyz - twx],
                     [txz - twy, tyz + twx, 1.0 - (txx + tyy)]])


def skew(w):
    return np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])


# ---- g2o's SE3Quat / isometry mappings ---------------------------------------------------------------------------------------
def se3quat_exp(u):
    """SE3Quat::exp([omega; upsilon]) as an isometry."""
    u = np.asarray(u, np.float64)
    w, ups = u[:3], u[3:]
    theta = np.sqrt(w @ w)
    Om = skew(w)
    Om2 = Om @ Om
    if theta < G2O["exp_small_theta"]:
        R = np.eye(3) + Om + Om2
        V = R
    else:
        t2 = theta * theta
        R = np.eye(3) + np.sin(theta) / theta * Om + (1.0 - np.cos(theta)) / t2 * Om2
        V = np.eye(3) + (1.0 - np.cos(theta)) / t2 * Om + (theta - np.sin(theta)) / (t2 * theta) * Om2
    return R_from_quat(unit_quat(R)), V @ ups


def se3quat_log(X):
    """SE3Quat(estimate()).log(): R rebuilt from the normalised quaternion -> [omega; V^-1 t]."""
    R = R_from_quat(unit_quat(X[0]))
    t = X[1]
    d = 0.5 * (R[0, 0] + R[1, 1] + R[2, 2] - 1.0)
    dR = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    if d > G2O["log_d_threshold"]:
        w = 0.5 * dR
        Om = skew(w)
        Vinv = np.eye(3) - 0.5 * Om + Om @ Om / 12.0
    else:
        theta = np.arccos(d)
        w = theta / (2.0 * np.sqrt(1.0 - d * d)) * dR
        Om = skew(w)
        Vinv = np.eye(3) - 0.5 * Om + (1.0 - theta / (2.0 * np.tan(theta / 2.0))) / (theta * theta) * (Om @ Om)
    return np.concatenate([w, Vinv @ t])


def to_vector_mqt(X):
    return np.concatenate([X[1], unit_quat(X[0])[1:]])


def from_vector_mqt(v):
    v = np.asarray(v, np.float64)
    n = 1.0 - (v[3] * v[3] + v[4] * v[4] + v[5] * v[5])
    R = np.eye(3) if n < 0.0 else R_from_quat(np.array([np.sqrt(n), v[3], v[4], v[5]]))
    return R, v[:3].copy()


def iso_mul(A, B):
    return A[0] @ B[0], A[0] @ B[1] + A[1]


def iso_inv(A):
    return A[0].T, -(A[0].T @ A[1])


def iso_from_T(T):
    T = np.asarray(T, np.float64).reshape(4, 4)
    return T[:3, :3].copy(), T[:3, 3].copy()


# ---- EdgeSE3 -------------------------------------------------------------------------------------------------------------------
def edge_error(Z, Xi, Xj):
    """e = toVectorMQT(Z^-1 X_i^-1 X_j)."""
    return to_vector_mqt(iso_mul(iso_mul(iso_inv(Z), iso_inv(Xi)), Xj))


def edge_jacobians(Z, Xi, Xj):
    """Exact de / d delta_i and de / d delta_j at 0 under X <- X fromVectorMQT(delta).  With A = Z^-1, B = X_i^-1 X_j and
    E = A B = (R_E, t_E), q_E = (w, v) its unit quaternion (w >= 0):
      J_j = [[R_E, 0], [0, w I + [v]x]],   J_i = [[-R_A, 2 R_A [t_B]x], [0, -(w I - [v]x) R_A]]."""
    A = iso_inv(Z)
    B = iso_mul(iso_inv(Xi), Xj)
    E = iso_mul(A, B)
    q = unit_quat(E[0])
    w, v = q[0], q[1:]
    Ji, Jj = np.zeros((6, 6)), np.zeros((6, 6))
    Jj[:3, :3] = E[0]
    Jj[3:, 3:] = w * np.eye(3) + skew(v)
    Ji[:3, :3] = -A[0]
    Ji[:3, 3:] = 2.0 * A[0] @ skew(B[1])
    Ji[3:, 3:] = -(w * np.eye(3) - skew(v)) @ A[0]
    return Ji, Jj


# ---- the graph (:4198-4290) ----------------------------------------------------------------------------------------------------
def build_graph(kf_valid, full_graph, lc_idx, min_lm_ess_graph=75, min_lm_cov_graph=75):
    """-> dict(kf_curr, verts (kf_list, ids ascending), edges [(i, j, kind, lc_entry)] in creation order)."""
    kf_valid = np.asarray(kf_valid).astype(bool)
    lc_idx = np.asarray(lc_idx, np.int64).reshape(-1, 3)
    n = kf_valid.shape[0]
    if lc_idx.shape[0] == 0 or not kf_valid[0]:
        raise ValueError("no LC entry / keyframe 0 NULL")
    for a, b, _ in lc_idx:
        if not (0 <= a < n and 0 <= b < n and kf_valid[a] and kf_valid[b]):
            raise ValueError("LC entry names a NULL or out-of-range keyframe")
    kf_curr = int(lc_idx[:, 1].max())
    verts = [i for i in range(0, kf_curr + 1) if kf_valid[i]]
    edges = []
    for i in range(0, kf_curr + 1):
        for j in range(i + 1, kf_curr + 1):
            if kf_valid[i] and kf_valid[j] and (full_graph[i][j] >= min_lm_ess_graph or full_graph[i][j] >= min_lm_cov_graph
                                                or abs(i - j) == 1):
                edges.append((i, j, 0, -1))
    for k, (a, b, _) in enumerate(lc_idx):
        edges.append((int(a), int(b), 1, k))
    return dict(kf_curr=kf_curr, verts=verts, edges=edges)


def initial_estimates(g, T_kf_w, x_kf_w, lc_idx, lc_pose):
    """:4220-4249 (before computeInitialGuess)."""
    lc_idx = np.asarray(lc_idx, np.int64).reshape(-1, 3)
    X = {}
    for i in g["verts"]:
        is_lc_j, ident = False, 0
        for ident, (a, b, _) in enumerate(lc_idx):
            if a == i:
                break
            if b == i:
                is_lc_j = True
                break
        if is_lc_j:
            T = expmap_se3(lc_pose[ident]) @ np.asarray(T_kf_w[lc_idx[ident][0]]).reshape(4, 4)
            X[i] = se3quat_exp(reverse_se3(logmap_se3(T)))
        else:
            X[i] = se3quat_exp(reverse_se3(x_kf_w[i]))
    return X


def measurements(g, T_kf_w, lc_pose):
    Zs = []
    for (i, j, kind, k) in g["edges"]:
        if kind == 0:
            Tij = inverse_se3(np.asarray(T_kf_w[i]).reshape(4, 4)) @ np.asarray(T_kf_w[j]).reshape(4, 4)
            Zs.append(se3quat_exp(reverse_se3(logmap_se3(Tij))))
        else:
            Zs.append(se3quat_exp(reverse_se3(lc_pose[k])))
    return Zs


def incident_edges(g):
    inc = {v: [] for v in g["verts"]}
    for e, (i, j, _, _) in enumerate(g["edges"]):
        inc[i].append(e)
        inc[j].append(e)
    return inc


def bfs_tree(g):
    """computeInitialGuess: Dijkstra from the fixed vertex 0 with unit edge cost and FIFO ties, a BFS; the neighbours of a
    vertex in the order of its incident edges (creation order).  -> [(vertex, parent, edge)] in the order the propagator sets
    them, and the BFS level of each."""
    inc = incident_edges(g)
    seen = {0}
    order, level = [], {0: 0}
    q = deque([0])
    while q:
        u = q.popleft()
        for e in inc[u]:
            i, j = g["edges"][e][:2]
            z = j if i == u else i
            if z not in seen:
                seen.add(z)
                level[z] = level[u] + 1
                order.append((z, u, e))
                q.append(z)
    return order, level


def active_vertices(g):
    inc = incident_edges(g)
    return [v for v in g["verts"] if v != 0 and inc[v]]


# ---- the optimiser -------------------------------------------------------------------------------------------------------------
class Pgo:
    def __init__(self, kf_valid, full_graph, lc_idx, min_lm_ess_graph=75, min_lm_cov_graph=75):
        self.g = build_graph(kf_valid, full_graph, lc_idx, min_lm_ess_graph, min_lm_cov_graph)
        self.lc_idx = np.asarray(lc_idx, np.int64).reshape(-1, 3)
        self.kf_valid = np.asarray(kf_valid).astype(bool)
        self.active = active_vertices(self.g)
        self.col = {v: k for k, v in enumerate(self.active)}
        order, _ = bfs_tree(self.g)
        reached = {v for v, _, _ in order}
        if any(v not in reached for v in self.active):
            raise ValueError("an active vertex has no path to vertex 0")
        self.tree = order

    def chi2(self, X, Zs):
        return float(sum(float(e @ e) for e in (edge_error(Z, X[i], X[j]) for Z, (i, j, _, _) in zip(Zs, self.g["edges"]))))

    def system(self, X, Zs):
        n = 6 * len(self.active)
        H, b = np.zeros((n, n)), np.zeros(n)
        for Z, (i, j, _, _) in zip(Zs, self.g["edges"]):
            e = edge_error(Z, X[i], X[j])
            Ji, Jj = edge_jacobians(Z, X[i], X[j])
            ci, cj = self.col.get(i), self.col.get(j)
            for c, J in ((ci, Ji), (cj, Jj)):
                if c is not None:
                    H[6 * c:6 * c + 6, 6 * c:6 * c + 6] += J.T @ J
                    b[6 * c:6 * c + 6] -= J.T @ e
            if ci is not None and cj is not None:
                H[6 * ci:6 * ci + 6, 6 * cj:6 * cj + 6] += Ji.T @ Jj
                H[6 * cj:6 * cj + 6, 6 * ci:6 * ci + 6] += Jj.T @ Ji
        return H, b

    def apply(self, X, dx):
        Y = dict(X)
        for v, c in self.col.items():
            Y[v] = iso_mul(X[v], from_vector_mqt(dx[6 * c:6 * c + 6]))
        return Y

    def optimize(self, T_kf_w, x_kf_w, lc_pose, max_iters=100, lambda_init=1e-10, max_trials=None, solve=None):
        """-> dict(X0 (the :4220-4249 estimates), X (final), trace [dict(it, trial, lam, chi, chi_new, scale, rho, ok,
        accepted)], iterations, stop (0: ran out, 1: Terminate), chi_initial, chi_final)."""
        max_trials = G2O["max_trials"] if max_trials is None else max_trials
        T_kf_w = np.asarray(T_kf_w, np.float64).reshape(-1, 4, 4)
        Zs = measurements(self.g, T_kf_w, lc_pose)
        X0 = initial_estimates(self.g, T_kf_w, x_kf_w, self.lc_idx, lc_pose)
        X = dict(X0)
        for v, u, e in self.tree:                      # computeInitialGuess
            i, j = self.g["edges"][e][:2]
            X[v] = iso_mul(X[u], Zs[e]) if i == u else iso_mul(X[u], iso_inv(Zs[e]))
        chi_initial = self.chi2(X, Zs)
        trace = []
        lam, ni = lambda_init, 2.0
        stop, it = 0, 0
        n = 6 * len(self.active)
        for it in range(max_iters):
            chi = self.chi2(X, Zs)
            H, b = self.system(X, Zs)
            if it == 0:
                lam, ni = lambda_init, 2.0
            q = 0
            while True:
                Hd = H + lam * np.eye(n)
                dx = (solve or np.linalg.solve)(Hd, b) if n else np.zeros(0)
                ok = bool(np.all(np.isfinite(dx)))
                if not ok:
                    dx = np.zeros(n)
                Y = self.apply(X, dx)
                chi_new = self.chi2(Y, Zs) if ok else DBL_MAX
                scale = float(dx @ (lam * dx + b)) + G2O["rho_denominator_eps"]
                rho = (chi - chi_new) / scale
                lam_used = lam
                accepted = bool(rho > 0 and np.isfinite(chi_new))
                if accepted:
                    a = 1.0 - (2.0 * rho - 1.0) ** 3
                    lam *= max(G2O["good_step_lower"], min(a, G2O["good_step_upper"]))
                    ni = 2.0
                    X = Y
                else:
                    lam *= ni
                    ni *= 2.0
                trace.append(dict(it=it, trial=q, lam=lam_used, chi=chi, chi_new=chi_new, scale=scale, rho=rho, ok=ok,
                                  accepted=accepted))
                q += 1
                if not (rho < 0 and q < max_trials):
                    break
            if q == max_trials or rho == 0:
                stop = 1
                break
        iterations = (it + 1) if max_iters > 0 else 0
        return dict(X0=X0, X=X, trace=trace, iterations=iterations, stop=stop, chi_initial=chi_initial,
                    chi_final=self.chi2(X, Zs))


# ---- the write-back (:4298-4356) and the later keyframes (:4358-4398) ---------------------------------------------------------
def write_back(P, res, T_kf_w, x_kf_w):
    """-> (T_out (n, 4, 4), x_out (n, 6), T_corr (n, 4, 4), corrected (n,) bool).  A vertex's final estimate is the optimised one
    when it is active, its :4220-4249 estimate otherwise (vertex 0, isolated vertices).  NULL slots after kf_curr are skipped
    (the reference dereferences them) and keep their pose."""
    T_kf_w = np.asarray(T_kf_w, np.float64).reshape(-1, 4, 4)
    n = T_kf_w.shape[0]
    T_out, x_out = T_kf_w.copy(), np.asarray(x_kf_w, np.float64).reshape(n, 6).copy()
    T_corr = np.tile(np.eye(4), (n, 1, 1))
    corrected = np.zeros(n, bool)
    act = set(P.active)
    last = np.eye(4)
    for k in P.g["verts"]:
        Xk = res["X"][k] if k in act else res["X0"][k]
        x = reverse_se3(se3quat_log(Xk))
        Tk = expmap_se3(x)
        T_out[k] = Tk
        x_out[k] = logmap_se3(Tk)
        last = Tk @ inverse_se3(T_kf_w[k])
        T_corr[k] = last
        corrected[k] = True
    for k in range(P.g["kf_curr"] + 1, n):
        if not P.kf_valid[k]:
            continue
        T_out[k] = last @ T_kf_w[k]
        x_out[k] = logmap_se3(T_out[k])
        T_corr[k] = last
        corrected[k] = True
    return T_out, x_out, T_corr, corrected


def _rt(T, p):
    """R p + t in Eigen's order: ((r0 p0 + r1 p1) + r2 p2) + t, no contraction."""
    R, t = T[:3, :3], T[:3, 3]
    return ((R[:, 0] * p[..., 0:1] + R[:, 1] * p[..., 1:2]) + R[:, 2] * p[..., 2:3]) + t


def correct_landmarks(T_corr, corrected, anchor_ptr, anchor_idx, valid, X, med_dir, dir_ptr, dirs, line=False):
    """The map correction of :4306-4355 / :4364-4397 for one kind: every slot k with corrected[k], in slot order, transforms
    every valid landmark of its anchor list.  X (n, 3) or (n, 6) for lines (both end points), med_dir (n, 3), dirs (m, 3) with
    landmark j's entries at dir_ptr[j]:dir_ptr[j+1].  Returns new arrays."""
    X, med_dir, dirs = X.copy(), med_dir.copy(), dirs.copy()
    for k in range(len(anchor_ptr) - 1):
        if not corrected[k]:
            continue
        T = T_corr[k]
        for a in range(anchor_ptr[k], anchor_ptr[k + 1]):
            j = anchor_idx[a]
            if not valid[j]:
                continue
            if line:
                X[j, :3] = _rt(T, X[j, :3])
                X[j, 3:] = _rt(T, X[j, 3:])
            else:
                X[j] = _rt(T, X[j])
            med_dir[j] = _rt(T, med_dir[j])
            d0, d1 = dir_ptr[j], dir_ptr[j + 1]
            if d1 > d0:
                dirs[d0:d1] = _rt(T, dirs[d0:d1])
    return X, med_dir, dirs
