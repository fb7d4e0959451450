// dense6_dev.hpp -- two one-lane 6 x 6 routines in fp64, the matrix in registers: the solve of a Gauss-Newton step as Eigen's
// ColPivHouseholderQR does it, and the largest eigenvalue of the inverse (the pose covariance).  Used by the loop-closure
// check's lane 0 (loop_closure.hip); nothing in here knows about loop closure.
#pragma once

#include <hip/hip_runtime.h>

#include <cfloat>

namespace plslam {

// ---- x = ColPivHouseholderQR(H).solve(g), Eigen 3.3 / 3.4 (ColPivHouseholderQR.h computeInPlace, _solve_impl;
// Householder.h makeHouseholder, applyHouseholderOnTheLeft; the column-major triangular solve, which skips a zero rhs
// entry).  One lane; every loop has a compile-time trip count and is unrolled, so the matrix (column-major
// A[6 * col + row]), the norms and the reflector coefficients stay in registers: a pivot column is exchanged by predicated
// swaps, never by a run-time index.
__device__ __forceinline__ void colpiv_qr_solve(const double Hm[36], const double gv[6], double x[6])
{
    constexpr int n = 6;
    double A[36], nu[6], nd[6], hc[6], c[6];
    int tr[6], perm[6];
#pragma unroll
    for (int j = 0; j < n; ++j)
#pragma unroll
        for (int i = 0; i < n; ++i) A[6 * j + i] = Hm[6 * i + j];
    double maxn = 0.0;
#pragma unroll
    for (int j = 0; j < n; ++j) {
        double q = 0.0;
#pragma unroll
        for (int i = 0; i < n; ++i) q += A[6 * j + i] * A[6 * j + i];
        nd[j] = sqrt(q);
        nu[j] = nd[j];
        if (j == 0 || nu[j] > maxn) maxn = nu[j];               // maxCoeff: the first of the largest
    }
    const double th_help = (maxn * DBL_EPSILON) * (maxn * DBL_EPSILON) / (double)n;
    const double downdate_th = sqrt(DBL_EPSILON);
    int nz = n;
#pragma unroll
    for (int k = 0; k < n; ++k) {
        int b = k;
        double bn = nu[k];
#pragma unroll
        for (int j = k + 1; j < n; ++j) {
            const bool gt = nu[j] > bn;
            bn = gt ? nu[j] : bn;
            b = gt ? j : b;
        }
        if (nz == n && bn * bn < th_help * (double)(n - k)) nz = k;
        tr[k] = b;
#pragma unroll
        for (int j = k + 1; j < n; ++j) {      // selects, not branches: b is per lane
            const bool sw = j == b;
#pragma unroll
            for (int i = 0; i < n; ++i) {
                const double u = A[6 * k + i], v = A[6 * j + i];
                A[6 * k + i] = sw ? v : u;
                A[6 * j + i] = sw ? u : v;
            }
            double u = nu[k], v = nu[j];
            nu[k] = sw ? v : u;
            nu[j] = sw ? u : v;
            u = nd[k]; v = nd[j];
            nd[k] = sw ? v : u;
            nd[j] = sw ? u : v;
        }
        // makeHouseholderInPlace on A[k:, k]
        double tail = 0.0;
#pragma unroll
        for (int i = k + 1; i < n; ++i) tail += A[6 * k + i] * A[6 * k + i];
        const double c0 = A[6 * k + k];
        double tau, beta;
        if (tail <= DBL_MIN) {
            tau = 0.0;
            beta = c0;
#pragma unroll
            for (int i = k + 1; i < n; ++i) A[6 * k + i] = 0.0;
        } else {
            beta = sqrt(c0 * c0 + tail);
            if (c0 >= 0.0) beta = -beta;
            const double den = c0 - beta;
#pragma unroll
            for (int i = k + 1; i < n; ++i) A[6 * k + i] = A[6 * k + i] / den;
            tau = (beta - c0) / beta;
        }
        hc[k] = tau;
        A[6 * k + k] = beta;
        // applyHouseholderOnTheLeft on A[k:, k+1:]
        if (n - k == 1) {
            // no column right of the last one
        } else if (tau != 0.0) {
#pragma unroll
            for (int j = k + 1; j < n; ++j) {
                double t = 0.0;
#pragma unroll
                for (int i = k + 1; i < n; ++i) t += A[6 * k + i] * A[6 * j + i];
                t += A[6 * j + k];
                A[6 * j + k] -= tau * t;
#pragma unroll
                for (int i = k + 1; i < n; ++i) A[6 * j + i] -= tau * A[6 * k + i] * t;
            }
        }
        // the column norms' downdate (LAPACK xGEQPF / xGEQP3)
#pragma unroll
        for (int j = k + 1; j < n; ++j) {
            if (nu[j] != 0.0) {
                double t = fabs(A[6 * j + k]) / nu[j];
                t = (1.0 + t) * (1.0 - t);
                t = t < 0.0 ? 0.0 : t;
                const double q = nu[j] / nd[j];
                const double t2 = t * (q * q);
                if (t2 <= downdate_th) {
                    double s2 = 0.0;
#pragma unroll
                    for (int i = k + 1; i < n; ++i) s2 += A[6 * j + i] * A[6 * j + i];
                    nd[j] = sqrt(s2);
                    nu[j] = nd[j];
                } else {
                    nu[j] *= sqrt(t);
                }
            }
        }
    }
#pragma unroll
    for (int i = 0; i < n; ++i) perm[i] = i;
#pragma unroll
    for (int k = 0; k < n; ++k)
#pragma unroll
        for (int j = k + 1; j < n; ++j)
        {
            const bool sw = tr[k] == j;
            const int u = perm[k], v = perm[j];
            perm[k] = sw ? v : u;
            perm[j] = sw ? u : v;
        }
#pragma unroll
    for (int i = 0; i < n; ++i) c[i] = gv[i];
#pragma unroll
    for (int k = 0; k < n; ++k) {               // c = H_{nz-1} ... H_0 c
        if (k >= nz) break;
        const double tau = hc[k];
        if (n - k == 1) { c[k] *= (1.0 - tau); continue; }
        if (tau == 0.0) continue;
        double t = 0.0;
#pragma unroll
        for (int i = k + 1; i < n; ++i) t += A[6 * k + i] * c[i];
        t += c[k];
        c[k] -= tau * t;
#pragma unroll
        for (int i = k + 1; i < n; ++i) c[i] -= tau * A[6 * k + i] * t;
    }
#pragma unroll
    for (int i = n - 1; i >= 0; --i) {          // R[0:nz, 0:nz] upper triangular, column by column
        if (i < nz && c[i] != 0.0) {
            c[i] /= A[6 * i + i];
            const double ci = c[i];
#pragma unroll
            for (int r = 0; r < i; ++r) c[r] -= ci * A[6 * i + r];
        }
    }
#pragma unroll
    for (int j = 0; j < n; ++j) x[j] = 0.0;
#pragma unroll
    for (int i = 0; i < n; ++i)
#pragma unroll
        for (int j = 0; j < n; ++j)
            x[j] = (perm[i] == j && i < nz) ? c[i] : x[j];          // nz == 0: x = 0 (_solve_impl)
}

// ---- the largest eigenvalue of H.inverse() (Eigen: PartialPivLU for a 6 x 6; SelfAdjointEigenSolver reads the lower
// triangle).  NaN if the inverse has a non-finite entry (Eigen's solver then returns NaN eigenvalues).  One lane, in
// registers, as the solve above.
__device__ __forceinline__ double cov_max_eig(const double Hm[36])
{
    constexpr int n = 6;
    double A[36];                                // row-major LU
    int perm[6];
#pragma unroll
    for (int k = 0; k < 36; ++k) A[k] = Hm[k];
#pragma unroll
    for (int k = 0; k < n; ++k) {
        int p = k;
        double big = fabs(A[6 * k + k]);
#pragma unroll
        for (int i = k + 1; i < n; ++i) {
            const bool gt = fabs(A[6 * i + k]) > big;
            big = gt ? fabs(A[6 * i + k]) : big;
            p = gt ? i : p;
        }
        perm[k] = p;
        if (big != 0.0) {
#pragma unroll
            for (int q = k + 1; q < n; ++q) {
                const bool sw = q == p;
#pragma unroll
                for (int j = 0; j < n; ++j) {
                    const double u = A[6 * k + j], v = A[6 * q + j];
                    A[6 * k + j] = sw ? v : u;
                    A[6 * q + j] = sw ? u : v;
                }
            }
#pragma unroll
            for (int i = k + 1; i < n; ++i) A[6 * i + k] /= A[6 * k + k];
        }
#pragma unroll
        for (int i = k + 1; i < n; ++i)
#pragma unroll
            for (int j = k + 1; j < n; ++j) A[6 * i + j] -= A[6 * i + k] * A[6 * k + j];
    }
    double S[36];
#pragma unroll
    for (int col = 0; col < n; ++col) {
        double b[6];
#pragma unroll
        for (int i = 0; i < n; ++i) b[i] = i == col ? 1.0 : 0.0;
#pragma unroll
        for (int k = 0; k < n; ++k)             // the row transpositions
#pragma unroll
            for (int q = k + 1; q < n; ++q)
            {
                const bool sw = perm[k] == q;
                const double u = b[k], v = b[q];
                b[k] = sw ? v : u;
                b[q] = sw ? u : v;
            }
#pragma unroll
        for (int i = 0; i < n; ++i)
#pragma unroll
            for (int j = 0; j < i; ++j) b[i] -= A[6 * i + j] * b[j];
#pragma unroll
        for (int i = n - 1; i >= 0; --i) {
#pragma unroll
            for (int j = i + 1; j < n; ++j) b[i] -= A[6 * i + j] * b[j];
            b[i] /= A[6 * i + i];
        }
        // column `col` of the inverse; the eigen solver reads the lower triangle: S(i, j) = S(j, i) = inv(max, min)
#pragma unroll
        for (int i = col; i < n; ++i) { S[6 * i + col] = b[i]; S[6 * col + i] = b[i]; }
    }
    bool finite = true;
#pragma unroll
    for (int k = 0; k < 36; ++k) finite = finite && isfinite(S[k]);
    if (!finite) return __builtin_nan("");
    // cyclic Jacobi; converges quadratically -- 30 sweeps is far beyond what a 6 x 6 needs
#pragma unroll 1
    for (int sweep = 0; sweep < 30; ++sweep) {
        double off = 0.0, dia = 0.0;
#pragma unroll
        for (int i = 0; i < n; ++i)
#pragma unroll
            for (int j = 0; j < n; ++j) {
                if (i != j) off += S[6 * i + j] * S[6 * i + j];
                else dia += S[6 * i + j] * S[6 * i + j];
            }
        if (!(off > 1e-34 * dia)) break;
#pragma unroll
        for (int p = 0; p < n - 1; ++p)
#pragma unroll
            for (int q = p + 1; q < n; ++q) {
                const double apq = S[6 * p + q];
                if (apq == 0.0) continue;
                const double tau = (S[6 * q + q] - S[6 * p + p]) / (2.0 * apq);
                const double t = (tau >= 0.0 ? 1.0 : -1.0) / (fabs(tau) + sqrt(1.0 + tau * tau));
                const double c = 1.0 / sqrt(1.0 + t * t), sn = t * c;
#pragma unroll
                for (int k = 0; k < n; ++k) {   // S <- J^T S J
                    const double akp = S[6 * k + p], akq = S[6 * k + q];
                    S[6 * k + p] = c * akp - sn * akq;
                    S[6 * k + q] = sn * akp + c * akq;
                }
#pragma unroll
                for (int k = 0; k < n; ++k) {
                    const double apk = S[6 * p + k], aqk = S[6 * q + k];
                    S[6 * p + k] = c * apk - sn * aqk;
                    S[6 * q + k] = sn * apk + c * aqk;
                }
            }
    }
    double m = S[0];
#pragma unroll
    for (int i = 1; i < n; ++i) m = S[6 * i + i] > m ? S[6 * i + i] : m;
    return m;
}

}  // namespace plslam
