"""A solve of the global bundle adjustment's damped system that shares no structure with the device or with tests/gba_ref.py's
Schur complement: Gaussian elimination with partial pivoting over the whole N x N matrix in np.longdouble (64-bit mantissa on
x86-64; np.linalg does not take it), and stvo-pl's SE(3) maps by their full formulas in the same precision.  numpy only."""
from __future__ import annotations

import numpy as np

LD = np.longdouble


def solve_long_double(A, b):
    """x with A x = b, every operation in long double"""
    A = np.array(A, LD)
    x = np.array(b, LD)
    n = A.shape[0]
    for k in range(n):
        p = k + int(np.argmax(np.abs(A[k:, k])))
        if p != k:
            A[[k, p]] = A[[p, k]]
            x[[k, p]] = x[[p, k]]
        f = A[k + 1:, k] / A[k, k]
        nz = np.flatnonzero(f) + k + 1                       # rows that column k does not reach stay as they are
        A[nz, k + 1:] -= np.outer(f[nz - k - 1], A[k, k + 1:])
        x[nz] -= f[nz - k - 1] * x[k]
    for k in range(n - 1, -1, -1):
        x[k] = (x[k] - A[k, k + 1:] @ x[k + 1:]) / A[k, k]
    return x


def damped_system(P, B, lam):
    """The whole system of one pass as SimplicialLDLT factors it: H + lam diag(H), g"""
    H, g = P.full_H(B)
    return H + lam * np.diag(np.diag(H)), g


def _skew(w):
    z = LD(0)
    return np.array([[z, -w[2], w[1]], [w[2], z, -w[0]], [-w[1], w[0], z]], LD)


def expmap_ld(x):
    """exp of se(3), Rodrigues' formulas at every angle but 0 itself"""
    x = np.array(x, LD)
    th = np.sqrt(x[3] * x[3] + x[4] * x[4] + x[5] * x[5])
    T = np.eye(4, dtype=LD)
    if th == 0:
        T[:3, 3] = x[:3]
        return T
    s = _skew(x[3:] / th)
    s2 = s @ s
    # 1 - cos and theta - sin without cancellation: 2 sin^2(theta / 2), and the series below 1e-2 (its next term is theta^8 / 9!)
    omc = 2 * np.sin(th / 2) ** 2
    tms = th - np.sin(th) if th > LD(1e-2) else th ** 3 / 6 * (1 - th ** 2 / 20 * (1 - th ** 2 / 42))
    T[:3, :3] = np.eye(3, dtype=LD) + s * np.sin(th) + s2 * omc
    V = np.eye(3, dtype=LD) + s * omc / th + s2 * tms / th
    T[:3, 3] = V @ x[:3]
    return T


def logmap_ld(T):
    """log of SE(3) for angles in (0, pi): the angle from atan2 of the antisymmetric part and the trace"""
    T = np.array(T, LD)
    R = T[:3, :3]
    a = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]], LD) / 2      # sin(theta) axis
    sn = np.sqrt(a @ a)
    th = np.arctan2(sn, (R[0, 0] + R[1, 1] + R[2, 2] - 1) / 2)
    if sn == 0:
        return np.concatenate([T[:3, 3], np.zeros(3, LD)])
    w = a / sn * th
    s = _skew(w / th)
    omc = 2 * np.sin(th / 2) ** 2
    tms = th - np.sin(th) if th > LD(1e-2) else th ** 3 / 6 * (1 - th ** 2 / 20 * (1 - th ** 2 / 42))
    V = np.eye(3, dtype=LD) + s * omc / th + s @ s * tms / th
    return np.concatenate([solve_long_double(V, T[:3, 3]), w])


def inverse_ld(T):
    o = np.eye(4, dtype=LD)
    o[:3, :3] = T[:3, :3].T
    o[:3, 3] = -T[:3, :3].T @ T[:3, 3]
    return o
