// K25 -- MapHandler::isLoopClosure (src/mapHandler.cpp:3192-3300) with computeRelativePoseRobustGN (:3566-3957): the check
// a loop-closure candidate keyframe goes through, in ONE workgroup of 256 lanes, fp64, no FMA contraction.
//   1. gather: the correspondences of the two match tables (run before this kernel by the match plan) in i1 order, as
//      :3225-3241 / :3251-3268 build lc_points / lc_lines and lc_pt_idx / lc_ls_idx -- a ballot prefix per 256-row chunk;
//   2. the inlier-ratio gate (:3273-3293; std::max(a, b) = a < b ? b : a, 0 / 0 = NaN, NaN fails '>');
//   3. the robust Gauss-Newton: max_iters iterations, the outlier pass (||err_i|| > sqrt(7.815)), max_iters_ref
//      iterations, err_prev carried across the stages (:3583).  Per iteration every lane folds the observations tid,
//      tid + 256, ... into registers (K17's row math, pose_gn_dev.hpp) and the 256 partials are summed in K17's tree
//      (pairs (t, t + st), st = 128 ... 1; the last six levels as wave shuffles): the system is bit-identical to K17's at the
//      same T_inc.  Lane 0 then normalises e, applies the two stop tests, solves the 6 x 6 system (Eigen's
//      ColPivHouseholderQR restated) and updates T_inc = T_inc * inverse_se3(expmap_se3(x_inc)) -- in LDS;
//   4. the decision (:3874-3951): lc_res on the last assembled e, lc_unc on the largest eigenvalue of H^-1 (Eigen's
//      PartialPivLU inverse; cyclic Jacobi on its lower triangle), lc_inl computed and then forced true (:3903), the
//      translation / rotation tests on logmap_se3(T_inc), and pose_inc on success.
// Every correspondence is read from global memory (L2) on every pass: nothing is staged in LDS, so the counts are bounded
// only by PLSLAM_LC_MAX_FEATURES.  No atomics on doubles; the result does not depend on scheduling.
//
// K54 -- the same check for B candidates in one launch: workgroup b copies record b of a device-resident LcArgs table
// into LDS and runs lc_problem(), the text K25 runs on its one record.  Nothing is shared between workgroups, so a
// record's result is the single call's bit for bit wherever it sits in the table.  The match tables of the whole batch come
// from ONE match plan (plslam_lc_batch, below), which is rebuilt only when its problem list changes.
#include <cfloat>
#include <cstring>
#include <new>
#include <vector>

#include "match_plan.hpp"
#include "pose_gn_dev.hpp"
#include "se3_dev.hpp"

namespace plslam {
namespace {

constexpr int LC_THREADS = 256;
constexpr int LC_RED = 2 * GN_TERMS;     // points' then lines' partial sums per lane

struct LcArgs {
    GnCam K;
    double th;
    const double* P;          // kf0 stereo_pt[i]->P  (n_pt0 x 3)   [identity: lc_points[k]->P]
    const double* pl;         // kf1 stereo_pt[i]->pl (n_pt1 x 2)   [identity: ->pl_obs]
    const int32_t* pt_idx0;   // may be null (-1)
    const int32_t* pt_idx1;
    const double* sPeP;       // kf0 (n_ls0 x 6)
    const double* le;         // kf1 (n_ls1 x 3)
    const int32_t* ls_idx0;
    const int32_t* ls_idx1;
    const int32_t* m12_p;     // the match tables (n_pt0 / n_ls0 entries); null: the kind was not matched
    const int32_t* m12_l;
    int32_t n_pt0, n_pt1, n_ls0, n_ls1;
    int32_t identity;         // plslam_relpose_robust_gn: correspondence k is (k, k), no gate
    int32_t has_points, has_lines, max_iters, max_iters_ref;
    double lc_inlier_ratio, lc_res, lc_unc, lc_inl, lc_trs, lc_rot;
    int32_t* pt_corr;         // n_pt0 x 4
    uint8_t* pt_inl;
    int32_t* ls_corr;
    uint8_t* ls_inl;
    plslam_lc_result* res;
};

struct LcShared {
    double red[LC_RED][LC_THREADS / 2];
    double T[16];                   // T_inc, row-major
    double H[36], g[6];             // the last assembled system (row-major)
    double e, err_prev;
    int32_t wsum[4];
    int32_t cnt[2];
    int32_t n_corr[2];
    int32_t go;                     // 1: run / continue
    int32_t ran;                    // the gate passed: GN runs
    int32_t iters[2];
    int64_t clk0, clk_serial;       // lane 0's diagnostics (kept here, not in registers live across the kernel)
};

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

// correspondences of one kind in i1 order -> rows (idx0[i1], i1, idx1[i2], i2), inlier flags 1; returns their count.
// corr may be null where correspondence k is (k, k) (the batched GN on the caller's correspondences keeps no rows)
__device__ __forceinline__ int32_t gather_kind(LcShared& s, const int32_t* m12, int identity, int32_t n0, int32_t n1,
                                               const int32_t* idx0, const int32_t* idx1, int32_t* corr, uint8_t* inl)
{
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    int32_t total = 0;
    if (!identity && !m12) return 0;
    for (int32_t base = 0; base < n0; base += LC_THREADS) {
        const int32_t i1 = base + tid;
        int32_t i2 = -1;
        if (i1 < n0) i2 = identity ? i1 : g_(m12)[i1];
        const bool f = i2 >= 0 && i2 < n1;
        const uint64_t bal = __ballot(f);
        const int below = __popcll(bal & ((uint64_t(1) << lane) - 1));
        if (lane == 0) s.wsum[wv] = __popcll(bal);
        __syncthreads();
        int32_t off = total;
        for (int w = 0; w < wv; ++w) off += s.wsum[w];
        const int32_t chunk = s.wsum[0] + s.wsum[1] + s.wsum[2] + s.wsum[3];
        if (f) {
            const int32_t k = off + below;
            if (corr) {
                g_(corr)[4 * (size_t)k] = idx0 ? g_(idx0)[i1] : -1;
                g_(corr)[4 * (size_t)k + 1] = i1;
                g_(corr)[4 * (size_t)k + 2] = idx1 ? g_(idx1)[i2] : -1;
                g_(corr)[4 * (size_t)k + 3] = i2;
            }
            g_(inl)[k] = 1;
        }
        total += chunk;
        __syncthreads();
    }
    return total;
}

// rows (i1, i2) of correspondence k
__device__ __forceinline__ void corr_rows(const int32_t* corr, int32_t k, int32_t& i1, int32_t& i2)
{
    if (corr) {
        i1 = g_(corr)[4 * (size_t)k + 1];
        i2 = g_(corr)[4 * (size_t)k + 3];
    } else {
        i1 = i2 = k;
    }
}

__device__ __forceinline__ void load_T(const LcShared& s, double Tm[12])
{
#pragma unroll
    for (int i = 0; i < 12; ++i) Tm[i] = s.T[i];
}

// one Gauss-Newton system at s.T over the current inliers: lane 0 returns with H, g, e summed (e not yet normalised) and
// s.cnt = (N_p, N_l).  K17's lane assignment and tree.
__device__ __forceinline__ void assemble(LcShared& s, const LcArgs& a, int32_t ncp, int32_t ncl)
{
    const int tid = threadIdx.x;
    double Tm[12];
    load_T(s, Tm);
    double ap[GN_TERMS], al[GN_TERMS];
#pragma unroll
    for (int k = 0; k < GN_TERMS; ++k) ap[k] = al[k] = 0.0;
    int np = 0, nl = 0;
    for (int32_t k = tid; k < ncp; k += LC_THREADS) {
        if (!g_(a.pt_inl)[k]) continue;
        int32_t i1, i2;
        corr_rows(a.pt_corr, k, i1, i2);
        const double X[3] = {g_(a.P)[3 * (size_t)i1], g_(a.P)[3 * (size_t)i1 + 1], g_(a.P)[3 * (size_t)i1 + 2]};
        gn_point_row(a.K, a.th, Tm, X, g_(a.pl)[2 * (size_t)i2], g_(a.pl)[2 * (size_t)i2 + 1], ap);
        ++np;
    }
    for (int32_t k = tid; k < ncl; k += LC_THREADS) {
        if (!g_(a.ls_inl)[k]) continue;
        int32_t i1, i2;
        corr_rows(a.ls_corr, k, i1, i2);
        double SE[6], l[3];
#pragma unroll
        for (int q = 0; q < 6; ++q) SE[q] = g_(a.sPeP)[6 * (size_t)i1 + q];
#pragma unroll
        for (int q = 0; q < 3; ++q) l[q] = g_(a.le)[3 * (size_t)i2 + q];
        gn_line_row(a.K, a.th, Tm, SE, l, al);
        ++nl;
    }
    if (tid < 2) s.cnt[tid] = 0;
    __syncthreads();
    if (np) atomicAdd(&s.cnt[0], np);
    if (nl) atomicAdd(&s.cnt[1], nl);
    // st = 128 and 64 through LDS: lane t (< st) adds lane t + st's partials
    for (int st = LC_THREADS / 2; st >= 64; st >>= 1) {
        if (tid >= st && tid < 2 * st) {
#pragma unroll
            for (int k = 0; k < GN_TERMS; ++k) { s.red[k][tid - st] = ap[k]; s.red[GN_TERMS + k][tid - st] = al[k]; }
        }
        __syncthreads();
        if (tid < st) {
#pragma unroll
            for (int k = 0; k < GN_TERMS; ++k) { ap[k] = ap[k] + s.red[k][tid]; al[k] = al[k] + s.red[GN_TERMS + k][tid]; }
        }
        __syncthreads();
    }
    if (tid < 64) {                               // st = 32 ... 1 inside wave 0: lane t adds lane t + st
#pragma unroll
        for (int st = 32; st > 0; st >>= 1) {
#pragma unroll
            for (int k = 0; k < GN_TERMS; ++k) {
                ap[k] = ap[k] + __shfl_down(ap[k], st, 64);
                al[k] = al[k] + __shfl_down(al[k], st, 64);
            }
        }
        if (tid == 0) {
            int k = 0;
#pragma unroll
            for (int i = 0; i < 6; ++i)
#pragma unroll
                for (int j = i; j < 6; ++j) {
                    const double v = ap[k] + al[k];
                    s.H[6 * i + j] = v;
                    s.H[6 * j + i] = v;
                    ++k;
                }
#pragma unroll
            for (int i = 0; i < 6; ++i) s.g[i] = ap[21 + i] + al[21 + i];
            s.e = ap[27] + al[27];
        }
    }
}

// lane 0, after assemble(): :3681-3702 / :3860-3871.  Returns 0 when the loop breaks.
__device__ __forceinline__ int gn_step(LcShared& s)
{
    s.e /= (double)(s.cnt[1] + s.cnt[0]);
    if (fabs(s.e - s.err_prev) < DBL_EPSILON || s.e < DBL_EPSILON) return 0;
    double Hm[36], gv[6], x[6], E[16], Ei[16], T[16], Tn[16];
#pragma unroll
    for (int i = 0; i < 36; ++i) Hm[i] = s.H[i];
#pragma unroll
    for (int i = 0; i < 6; ++i) gv[i] = s.g[i];
    colpiv_qr_solve(Hm, gv, x);
    expmap_se3(x, E);
    inverse_se3(E, Ei);
#pragma unroll
    for (int i = 0; i < 16; ++i) T[i] = s.T[i];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
            Tn[4 * i + j] = ((T[4 * i] * Ei[j] + T[4 * i + 1] * Ei[4 + j]) + T[4 * i + 2] * Ei[8 + j]) + T[4 * i + 3] * Ei[12 + j];
#pragma unroll
    for (int i = 0; i < 16; ++i) s.T[i] = Tn[i];
    double xs = 0.0;
#pragma unroll
    for (int i = 0; i < 6; ++i) xs += x[i] * x[i];
    if (sqrt(xs) < DBL_EPSILON) return 0;
    s.err_prev = s.e;
    return 1;
}

// :3721-3757: ||err_i|| > sqrt(7.815) at the stage-1 T_inc clears the flag
__device__ __forceinline__ void outlier_pass(LcShared& s, const LcArgs& a, int32_t ncp, int32_t ncl)
{
    const int tid = threadIdx.x;
    const double chi = sqrt(7.815);
    double Tm[12];
    load_T(s, Tm);
    for (int32_t k = tid; k < ncp; k += LC_THREADS) {
        if (!g_(a.pt_inl)[k]) continue;
        int32_t i1, i2;
        corr_rows(a.pt_corr, k, i1, i2);
        const double X[3] = {g_(a.P)[3 * (size_t)i1], g_(a.P)[3 * (size_t)i1 + 1], g_(a.P)[3 * (size_t)i1 + 2]};
        double G[3], dx, dy;
        if (gn_point_residual(a.K, Tm, X, g_(a.pl)[2 * (size_t)i2], g_(a.pl)[2 * (size_t)i2 + 1], G, dx, dy) > chi)
            g_(a.pt_inl)[k] = 0;
    }
    for (int32_t k = tid; k < ncl; k += LC_THREADS) {
        if (!g_(a.ls_inl)[k]) continue;
        int32_t i1, i2;
        corr_rows(a.ls_corr, k, i1, i2);
        double SE[6], l[3], S[3], E[3], ds, de;
#pragma unroll
        for (int q = 0; q < 6; ++q) SE[q] = g_(a.sPeP)[6 * (size_t)i1 + q];
#pragma unroll
        for (int q = 0; q < 3; ++q) l[q] = g_(a.le)[3 * (size_t)i2 + q];
        if (gn_line_residual(a.K, Tm, SE, l, S, E, ds, de) > chi) g_(a.ls_inl)[k] = 0;
    }
}

// one problem, one workgroup: everything K25 and K54 compute.  a: the problem's record, already in LDS and visible to
// every lane (the arguments are read from LDS where they are used: held in registers, their ~50 scalars stay live across the
// whole kernel and spill beside the solve's uniform state)
__device__ __forceinline__ void lc_problem(LcShared& s, const LcArgs& a)
{
    const int tid = threadIdx.x;
    if (tid == 0) {
        s.clk0 = wall_clock64();
        s.clk_serial = 0;
    }
    const int32_t ncp = gather_kind(s, a.m12_p, a.identity, a.n_pt0, a.n_pt1, a.pt_idx0, a.pt_idx1, a.pt_corr, a.pt_inl);
    const int32_t ncl = gather_kind(s, a.m12_l, a.identity, a.n_ls0, a.n_ls1, a.ls_idx0, a.ls_idx1, a.ls_corr, a.ls_inl);
    if (tid == 0) {
        plslam_lc_result* R = a.res;
        // :3273-3293 (n_pt_0 ... are the keyframes' feature counts; int / int promoted as in the source)
        const double rp0 = 100.0 * ncp / a.n_pt0, rp1 = 100.0 * ncp / a.n_pt1;
        const double rl0 = 100.0 * ncl / a.n_ls0, rl1 = 100.0 * ncl / a.n_ls1;
        const double rpt = a.identity ? 0.0 : (rp0 < rp1 ? rp1 : rp0), rls = a.identity ? 0.0 : (rl0 < rl1 ? rl1 : rl0);
        bool cond = false;
        if (a.has_points && a.has_lines) cond = rpt > a.lc_inlier_ratio && rls > a.lc_inlier_ratio;
        else if (a.has_points) cond = rpt > a.lc_inlier_ratio;
        else if (a.has_lines) cond = rls > a.lc_inlier_ratio;
        if (a.identity) cond = true;
        g_(&R->common_pt)[0] = ncp;
        g_(&R->common_ls)[0] = ncl;
        g_(&R->inl_ratio_pt)[0] = rpt;
        g_(&R->inl_ratio_ls)[0] = rls;
        s.go = cond ? 1 : 0;
        s.ran = s.go;
#pragma unroll
        for (int i = 0; i < 16; ++i) s.T[i] = (i % 5 == 0) ? 1.0 : 0.0;
#pragma unroll
        for (int i = 0; i < 36; ++i) s.H[i] = 0.0;
#pragma unroll
        for (int i = 0; i < 6; ++i) s.g[i] = 0.0;
        s.e = 0.0;
        s.err_prev = 999999999.9;
        s.iters[0] = s.iters[1] = 0;
    }
    __syncthreads();
    if (s.ran) {
        for (int stage = 0; stage < 2; ++stage) {
            const int32_t iters = stage ? a.max_iters_ref : a.max_iters;
            for (int32_t it = 0; it < iters; ++it) {
                assemble(s, a, ncp, ncl);
                if (tid == 0) {
                    const int64_t c = wall_clock64();
                    ++s.iters[stage];
                    s.go = gn_step(s);
                    s.clk_serial += wall_clock64() - c;
                }
                __syncthreads();
                if (!s.go) break;
            }
            if (stage == 0) {
                outlier_pass(s, a, ncp, ncl);
                __syncthreads();
            }
        }
    }
    // inliers after the outlier pass (:3913-3925)
    if (tid < 2) s.cnt[tid] = 0;
    __syncthreads();
    int np = 0, nl = 0;
    for (int32_t k = tid; k < ncp; k += LC_THREADS) np += g_(a.pt_inl)[k] != 0;
    for (int32_t k = tid; k < ncl; k += LC_THREADS) nl += g_(a.ls_inl)[k] != 0;
    if (np) atomicAdd(&s.cnt[0], np);
    if (nl) atomicAdd(&s.cnt[1], nl);
    __syncthreads();
    if (tid != 0) return;
    const int64_t c = wall_clock64();
    double T[16], x[6] = {0, 0, 0, 0, 0, 0}, pose[6] = {0, 0, 0, 0, 0, 0};
#pragma unroll
    for (int i = 0; i < 16; ++i) T[i] = s.T[i];
    int is_lc = 0, ok_res = 0, ok_unc = 0, ok_inl = 0, ok_trs = 0, ok_rot = 0;
    double eig = 0.0, ratio = 0.0, t = 0.0, r = 0.0;
    const bool run = s.ran != 0;            // read here, not held across the loops (a lane mask: it would spill)
    if (run) {
        logmap_se3(T, x);
        ok_res = s.e < a.lc_res;
        double Hm[36];
#pragma unroll
        for (int i = 0; i < 36; ++i) Hm[i] = s.H[i];
        eig = cov_max_eig(Hm);
        ok_unc = eig < a.lc_unc;
        ratio = double(s.cnt[0] + s.cnt[1]) / double(ncp + ncl);
        ok_inl = ratio > a.lc_inl;
        t = sqrt(x[0] * x[0] + x[1] * x[1] + x[2] * x[2]);
        r = sqrt(x[3] * x[3] + x[4] * x[4] + x[5] * x[5]) * 180.0 / 3.1415926535897932384626433832795;
        ok_trs = t < a.lc_trs;
        ok_rot = r < a.lc_rot;
        is_lc = ok_res && ok_unc && ok_trs && ok_rot;         // lc_inl = true (:3903)
        if (is_lc) {
            double E[16], Ei[16];
            expmap_se3(x, E);
            inverse_se3(E, Ei);
            logmap_se3(Ei, pose);
        }
    }
    const int64_t c1 = wall_clock64();
    plslam_lc_result* R = a.res;
    g_(&R->is_lc)[0] = is_lc;
    g_(&R->gn_ran)[0] = run ? 1 : 0;
    g_(&R->n_pt_inliers)[0] = s.cnt[0];
    g_(&R->n_ls_inliers)[0] = s.cnt[1];
    g_(&R->iters_1)[0] = s.iters[0];
    g_(&R->iters_2)[0] = s.iters[1];
    g_(&R->ok_res)[0] = ok_res;
    g_(&R->ok_unc)[0] = ok_unc;
    g_(&R->ok_inl)[0] = ok_inl;
    g_(&R->ok_trs)[0] = ok_trs;
    g_(&R->ok_rot)[0] = ok_rot;
    g_(&R->reserved)[0] = 0;
    g_(&R->e)[0] = s.e;
    g_(&R->cov_eig)[0] = eig;
    g_(&R->ratio_inliers)[0] = ratio;
    g_(&R->t)[0] = t;
    g_(&R->r)[0] = r;
    for (int i = 0; i < 6; ++i) {
        g_(R->x_inc)[i] = x[i];
        g_(R->pose_inc)[i] = pose[i];
        g_(R->g)[i] = s.g[i];
    }
    for (int i = 0; i < 16; ++i) g_(R->T_inc)[i] = T[i];
    for (int i = 0; i < 36; ++i) g_(R->H)[i] = s.H[i];
    g_(&R->clk_serial)[0] = s.clk_serial + (c1 - c);
    g_(&R->clk_total)[0] = c1 - s.clk0;
}

__global__ void __launch_bounds__(LC_THREADS) k_loop_closure(LcArgs ka)
{
    __shared__ LcShared s;
    __shared__ LcArgs a;
    if (threadIdx.x == 0) a = ka;
    __syncthreads();
    lc_problem(s, a);
}

static_assert(sizeof(LcArgs) % 8 == 0, "K54 copies its record in 8-byte words");

// K54: workgroup b runs record b.  pt_off / ls_off (both or neither; B + 1 offsets in device memory): the records are
// identity problems over concatenated arrays -- record b's P, pl, sPeP, le and masks are the bases, and its rows are
// [off[b], off[b + 1]) (a count outside [0, PLSLAM_LC_MAX_FEATURES] is taken as 0: the offsets are the producer's, unseen by
// the host)
__global__ void __launch_bounds__(LC_THREADS) k_loop_closure_batched(const LcArgs* tab, const int32_t* pt_off, const int32_t* ls_off)
{
    __shared__ LcShared s;
    __shared__ LcArgs a;
    const int tid = threadIdx.x;
    constexpr int W = (int)(sizeof(LcArgs) / 8);
    if (tid < W) reinterpret_cast<uint64_t*>(&a)[tid] = g_(reinterpret_cast<const uint64_t*>(tab))[(size_t)blockIdx.x * W + tid];
    __syncthreads();
    if (tid == 0 && pt_off) {
        const int32_t po = g_(pt_off)[blockIdx.x], lo = g_(ls_off)[blockIdx.x];
        int32_t np = g_(pt_off)[blockIdx.x + 1] - po, nl = g_(ls_off)[blockIdx.x + 1] - lo;
        if (np < 0 || np > PLSLAM_LC_MAX_FEATURES || po < 0 || !a.P) np = 0;          // (a kind without arrays has no rows)
        if (nl < 0 || nl > PLSLAM_LC_MAX_FEATURES || lo < 0 || !a.sPeP) nl = 0;
        a.P += 3 * (size_t)po; a.pl += 2 * (size_t)po; a.pt_inl += po;
        a.sPeP += 6 * (size_t)lo; a.le += 3 * (size_t)lo; a.ls_inl += lo;
        a.n_pt0 = a.n_pt1 = np;
        a.n_ls0 = a.n_ls1 = nl;
    }
    __syncthreads();
    lc_problem(s, a);
}

struct LcDev {             // device pointers of one call
    const uint8_t *pd0, *pd1, *ld0, *ld1;
    LcArgs a;
};

int check_params(const plslam_lc_params* p)
{
    PLSLAM_REQUIRE(p != nullptr, PLSLAM_EINVAL);
    PLSLAM_REQUIRE(p->max_iters >= 0 && p->max_iters <= PLSLAM_LC_MAX_ITERS, PLSLAM_EINVAL);
    PLSLAM_REQUIRE(p->max_iters_ref >= 0 && p->max_iters_ref <= PLSLAM_LC_MAX_ITERS, PLSLAM_EINVAL);
    return PLSLAM_OK;
}

int check_kf(const plslam_lc_keyframe* k)
{
    PLSLAM_REQUIRE(k != nullptr && k->n_pt >= 0 && k->n_ls >= 0, PLSLAM_EINVAL);
    PLSLAM_REQUIRE(k->n_pt == 0 || (k->pdesc && k->P && k->pl), PLSLAM_EINVAL);
    PLSLAM_REQUIRE(k->n_ls == 0 || (k->ldesc && k->sPeP && k->le), PLSLAM_EINVAL);
    PLSLAM_REQUIRE(k->n_pt <= PLSLAM_LC_MAX_FEATURES && k->n_ls <= PLSLAM_LC_MAX_FEATURES, PLSLAM_ERANGE);
    return PLSLAM_OK;
}

void fill_args(LcArgs& a, const plslam_lc_params* p)
{
    a.K = GnCam{p->cam.fx, p->cam.fy, p->cam.cx, p->cam.cy};
    a.th = p->homog_th;
    a.has_points = p->has_points ? 1 : 0;
    a.has_lines = p->has_lines ? 1 : 0;
    a.max_iters = p->max_iters;
    a.max_iters_ref = p->max_iters_ref;
    a.lc_inlier_ratio = p->lc_inlier_ratio;
    a.lc_res = p->lc_res;
    a.lc_unc = p->lc_unc;
    a.lc_inl = p->lc_inl;
    a.lc_trs = p->lc_trs;
    a.lc_rot = p->lc_rot;
}

// the two match problems of :3222-3223 / :3248-3249 (run only where the source calls match()) and K25, on ctx->stream.
// m12: the context's table scratch (n_pt0 + n_ls0 entries + 2 counters)
int enqueue_verify(plslam_ctx* ctx, const plslam_lc_params* p, const plslam_lc_keyframe* k0, const plslam_lc_keyframe* k1,
                   LcArgs& a)
{
    int rc;
    const bool mp = p->has_points && k0->n_pt > 0 && k1->n_pt > 0;
    const bool ml = p->has_lines && k0->n_ls > 0 && k1->n_ls > 0;
    Carver ct;
    const size_t oP = ct.take((size_t)k0->n_pt * 4), oL = ct.take((size_t)k0->n_ls * 4), oC = ct.take(8);
    if ((rc = ctx->lc_tab.reserve(ct.off))) return rc;
    char* tb = ctx->lc_tab.as<char>();
    plslam_match_problem pr[2];
    memset(pr, 0, sizeof(pr));
    int np = 0;
    if (mp) {
        pr[np].d1 = k0->pdesc; pr[np].d2 = k1->pdesc; pr[np].n1 = k0->n_pt; pr[np].n2 = k1->n_pt;
        pr[np].nnr = p->min_ratio_12_p; pr[np].mutual = p->mutual ? 1 : 0;
        pr[np].matches_12 = (int32_t*)(tb + oP); pr[np].n_matches = (int32_t*)(tb + oC);
        ++np;
    }
    if (ml) {
        pr[np].d1 = k0->ldesc; pr[np].d2 = k1->ldesc; pr[np].n1 = k0->n_ls; pr[np].n2 = k1->n_ls;
        pr[np].nnr = p->min_ratio_12_l; pr[np].mutual = p->mutual ? 1 : 0;
        pr[np].matches_12 = (int32_t*)(tb + oL); pr[np].n_matches = (int32_t*)(tb + oC) + 1;
        ++np;
    }
    if (np && (rc = match_problems_lc(ctx, pr, np))) return rc;
    fill_args(a, p);
    a.P = k0->P; a.pl = k1->pl; a.pt_idx0 = k0->pt_idx; a.pt_idx1 = k1->pt_idx;
    a.sPeP = k0->sPeP; a.le = k1->le; a.ls_idx0 = k0->ls_idx; a.ls_idx1 = k1->ls_idx;
    a.m12_p = mp ? (const int32_t*)(tb + oP) : nullptr;
    a.m12_l = ml ? (const int32_t*)(tb + oL) : nullptr;
    a.n_pt0 = k0->n_pt; a.n_pt1 = k1->n_pt; a.n_ls0 = k0->n_ls; a.n_ls1 = k1->n_ls;
    a.identity = 0;
    hipLaunchKernelGGL(k_loop_closure, dim3(1), dim3(LC_THREADS), 0, ctx->stream, a);
    PLSLAM_HIP_CHECK(hipGetLastError());
    return PLSLAM_OK;
}

// the _dev forms run on the context's stream, behind what the caller's stream holds on entry and in front of what it is given
// next (ctx->lc_ev; the caller holds ctx->mu)
int fence_enter(plslam_ctx* ctx, hipStream_t us)
{
    if (!us || us == ctx->stream) return PLSLAM_OK;
    for (hipEvent_t& e : ctx->lc_ev)
        if (!e) PLSLAM_HIP_CHECK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    PLSLAM_HIP_CHECK(hipEventRecord(ctx->lc_ev[0], us));
    PLSLAM_HIP_CHECK(hipStreamWaitEvent(ctx->stream, ctx->lc_ev[0], 0));
    return PLSLAM_OK;
}

int fence_leave(plslam_ctx* ctx, hipStream_t us)
{
    if (!us || us == ctx->stream) return PLSLAM_OK;
    PLSLAM_HIP_CHECK(hipEventRecord(ctx->lc_ev[1], ctx->stream));
    PLSLAM_HIP_CHECK(hipStreamWaitEvent(us, ctx->lc_ev[1], 0));
    return PLSLAM_OK;
}

}  // namespace
}  // namespace plslam

// B candidates per call (K54).  Every buffer only grows; the match plan is kept while its problem list stays the same.
struct plslam_lc_batch {
    plslam_ctx* ctx = nullptr;
    plslam_lc_params p{};
    int32_t max_pairs = 0;
    plslam_match_plan* plan = nullptr;
    std::vector<plslam_match_problem> plan_probs;   // what `plan` holds; empty: none
    std::vector<plslam_match_problem> probs;        // this call's list
    std::vector<plslam::LcArgs> h_args;             // K54's table (pageable: the copy call stages it before it returns)
    std::vector<plslam_lc_keyframe> d_kf;           // the host form's device records
    plslam::DevBuf tab, args;                       // the match tables + counters; K54's table
    plslam::DevBuf in, out;                         // the host form's keyframe image and outputs
    plslam::HostBuf pin_in, pin_out;
};

namespace plslam {
namespace {

int check_batch(const plslam_lc_batch* bt, const plslam_lc_keyframe* kf0, const plslam_lc_keyframe* kf1, int32_t B)
{
    int rc;
    PLSLAM_REQUIRE(bt != nullptr, PLSLAM_EINVAL);
    PLSLAM_REQUIRE(B >= 0 && B <= bt->max_pairs, PLSLAM_EINVAL);
    PLSLAM_REQUIRE(B == 0 || (kf0 && kf1), PLSLAM_EINVAL);
    for (int32_t b = 0; b < B; ++b)
        if ((rc = check_kf(kf0 + b)) || (rc = check_kf(kf1 + b))) return rc;
    return PLSLAM_OK;
}

// the match problems of every pair as ONE plan (per pair what enqueue_verify sets; a kind the source would not match is
// skipped) and K54 over the B records, on ctx->stream.  Pair b's rows start at row sum_{b' < b} kf0[b'].n_pt (n_ls).
int enqueue_batch(plslam_lc_batch* bt, const plslam_lc_keyframe* kf0, const plslam_lc_keyframe* kf1, int32_t B,
                  plslam_lc_result* res, int32_t* pc, uint8_t* pi, int32_t* lc, uint8_t* li)
{
    int rc;
    plslam_ctx* ctx = bt->ctx;
    const plslam_lc_params* p = &bt->p;
    size_t sp = 0, sl = 0;
    for (int32_t b = 0; b < B; ++b) { sp += (size_t)kf0[b].n_pt; sl += (size_t)kf0[b].n_ls; }
    Carver ct;
    const size_t oP = ct.take(sp * 4), oL = ct.take(sl * 4), oC = ct.take((size_t)B * 8);
    if ((rc = bt->tab.reserve(ct.off))) return rc;
    if ((rc = bt->args.reserve((size_t)B * sizeof(LcArgs)))) return rc;
    char* tb = bt->tab.as<char>();
    bt->probs.clear();
    bt->h_args.assign((size_t)B, LcArgs{});
    size_t rp = 0, rl = 0;
    for (int32_t b = 0; b < B; ++b) {
        const plslam_lc_keyframe *k0 = kf0 + b, *k1 = kf1 + b;
        const bool mp = p->has_points && k0->n_pt > 0 && k1->n_pt > 0;
        const bool ml = p->has_lines && k0->n_ls > 0 && k1->n_ls > 0;
        plslam_match_problem q;
        memset(&q, 0, sizeof(q));
        q.mutual = p->mutual ? 1 : 0;
        if (mp) {
            q.d1 = k0->pdesc; q.d2 = k1->pdesc; q.n1 = k0->n_pt; q.n2 = k1->n_pt; q.nnr = p->min_ratio_12_p;
            q.matches_12 = (int32_t*)(tb + oP) + rp; q.n_matches = (int32_t*)(tb + oC) + bt->probs.size();
            bt->probs.push_back(q);
        }
        if (ml) {
            q.d1 = k0->ldesc; q.d2 = k1->ldesc; q.n1 = k0->n_ls; q.n2 = k1->n_ls; q.nnr = p->min_ratio_12_l;
            q.matches_12 = (int32_t*)(tb + oL) + rl; q.n_matches = (int32_t*)(tb + oC) + bt->probs.size();
            bt->probs.push_back(q);
        }
        LcArgs& a = bt->h_args[(size_t)b];
        fill_args(a, p);
        a.P = k0->P; a.pl = k1->pl; a.pt_idx0 = k0->pt_idx; a.pt_idx1 = k1->pt_idx;
        a.sPeP = k0->sPeP; a.le = k1->le; a.ls_idx0 = k0->ls_idx; a.ls_idx1 = k1->ls_idx;
        a.m12_p = mp ? (const int32_t*)(tb + oP) + rp : nullptr;
        a.m12_l = ml ? (const int32_t*)(tb + oL) + rl : nullptr;
        a.n_pt0 = k0->n_pt; a.n_pt1 = k1->n_pt; a.n_ls0 = k0->n_ls; a.n_ls1 = k1->n_ls;
        a.identity = 0;
        a.res = res + b;
        a.pt_corr = pc ? pc + 4 * rp : nullptr; a.pt_inl = pi ? pi + rp : nullptr;
        a.ls_corr = lc ? lc + 4 * rl : nullptr; a.ls_inl = li ? li + rl : nullptr;
        rp += (size_t)k0->n_pt;
        rl += (size_t)k0->n_ls;
    }
    if (!bt->probs.empty()) {
        const bool same = bt->plan && bt->plan_probs.size() == bt->probs.size() &&
                          memcmp(bt->plan_probs.data(), bt->probs.data(), bt->probs.size() * sizeof(plslam_match_problem)) == 0;
        if (!same) {
            bt->plan_probs.clear();
            if ((rc = match_plan_rebuild(ctx, &bt->plan, bt->probs.data(), (int32_t)bt->probs.size()))) return rc;
            bt->plan_probs = bt->probs;
        }
        if ((rc = match_plan_enqueue(bt->plan, ctx->stream))) return rc;
    }
    PLSLAM_HIP_CHECK(hipMemcpyAsync(bt->args.p, bt->h_args.data(), (size_t)B * sizeof(LcArgs), hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(k_loop_closure_batched, dim3((unsigned)B), dim3(LC_THREADS), 0, ctx->stream, bt->args.as<LcArgs>(),
                       (const int32_t*)nullptr, (const int32_t*)nullptr);
    PLSLAM_HIP_CHECK(hipGetLastError());
    return PLSLAM_OK;
}

}  // namespace
}  // namespace plslam

extern "C" {

int plslam_loop_closure_verify(plslam_ctx* ctx, const plslam_lc_params* params, const plslam_lc_keyframe* kf0,
                               const plslam_lc_keyframe* kf1, plslam_lc_result* result, int32_t* pt_corr, uint8_t* pt_inlier,
                               int32_t* ls_corr, uint8_t* ls_inlier)
{
    using namespace plslam;
    int rc;
    PLSLAM_REQUIRE(ctx && result, PLSLAM_EINVAL);
    if ((rc = check_params(params)) || (rc = check_kf(kf0)) || (rc = check_kf(kf1))) return rc;
    std::lock_guard<std::mutex> lk(ctx->mu);
    DeviceGuard guard(ctx->device);
    hipStream_t s = ctx->stream;
    StreamSyncOnError sync_on_error(s);
    // one page-locked image of both keyframes -> one upload
    const plslam_lc_keyframe* K[2] = {kf0, kf1};
    Carver ci;
    size_t o[2][8];
    for (int q = 0; q < 2; ++q) {
        const size_t np = (size_t)K[q]->n_pt, nl = (size_t)K[q]->n_ls;
        o[q][0] = ci.take(np * 32); o[q][1] = ci.take(np * 24); o[q][2] = ci.take(np * 16); o[q][3] = ci.take(np * 4);
        o[q][4] = ci.take(nl * 32); o[q][5] = ci.take(nl * 48); o[q][6] = ci.take(nl * 24); o[q][7] = ci.take(nl * 4);
    }
    const size_t n0p = (size_t)kf0->n_pt, n0l = (size_t)kf0->n_ls;
    Carver co;
    const size_t oR = co.take(sizeof(plslam_lc_result)), oPC = co.take(n0p * 16), oPI = co.take(n0p), oLC = co.take(n0l * 16),
                 oLI = co.take(n0l);
    if ((rc = ctx->pin_in.reserve(ci.off + 256))) return rc;
    if ((rc = ctx->lc_in.reserve(ci.off + 256))) return rc;
    if ((rc = ctx->pin_out.reserve(co.off))) return rc;
    if ((rc = ctx->lc_out.reserve(co.off))) return rc;
    char* h = ctx->pin_in.as<char>();
    char* d = ctx->lc_in.as<char>();
    plslam_lc_keyframe D[2];
    for (int q = 0; q < 2; ++q) {
        const plslam_lc_keyframe& k = *K[q];
        const size_t np = (size_t)k.n_pt, nl = (size_t)k.n_ls;
        if (np) {
            memcpy(h + o[q][0], k.pdesc, np * 32); memcpy(h + o[q][1], k.P, np * 24); memcpy(h + o[q][2], k.pl, np * 16);
            if (k.pt_idx) memcpy(h + o[q][3], k.pt_idx, np * 4);
        }
        if (nl) {
            memcpy(h + o[q][4], k.ldesc, nl * 32); memcpy(h + o[q][5], k.sPeP, nl * 48); memcpy(h + o[q][6], k.le, nl * 24);
            if (k.ls_idx) memcpy(h + o[q][7], k.ls_idx, nl * 4);
        }
        D[q].n_pt = k.n_pt; D[q].n_ls = k.n_ls;
        D[q].pdesc = (const uint8_t*)(d + o[q][0]); D[q].P = (const double*)(d + o[q][1]); D[q].pl = (const double*)(d + o[q][2]);
        D[q].pt_idx = k.pt_idx ? (const int32_t*)(d + o[q][3]) : nullptr;
        D[q].ldesc = (const uint8_t*)(d + o[q][4]); D[q].sPeP = (const double*)(d + o[q][5]); D[q].le = (const double*)(d + o[q][6]);
        D[q].ls_idx = k.ls_idx ? (const int32_t*)(d + o[q][7]) : nullptr;
    }
    if (ci.off) PLSLAM_HIP_CHECK(hipMemcpyAsync(d, h, ci.off, hipMemcpyHostToDevice, s));
    char* od = ctx->lc_out.as<char>();
    LcArgs a{};
    a.res = (plslam_lc_result*)(od + oR);
    a.pt_corr = (int32_t*)(od + oPC); a.pt_inl = (uint8_t*)(od + oPI);
    a.ls_corr = (int32_t*)(od + oLC); a.ls_inl = (uint8_t*)(od + oLI);
    if ((rc = enqueue_verify(ctx, params, &D[0], &D[1], a))) return rc;
    PLSLAM_HIP_CHECK(hipMemcpyAsync(ctx->pin_out.p, od, co.off, hipMemcpyDeviceToHost, s));
    PLSLAM_HIP_CHECK(hipStreamSynchronize(s));
    sync_on_error.dismiss();
    const char* ho = ctx->pin_out.as<char>();
    memcpy(result, ho + oR, sizeof(plslam_lc_result));
    const size_t ncp = (size_t)result->common_pt, ncl = (size_t)result->common_ls;
    if (pt_corr && ncp) memcpy(pt_corr, ho + oPC, ncp * 16);
    if (pt_inlier && ncp) memcpy(pt_inlier, ho + oPI, ncp);
    if (ls_corr && ncl) memcpy(ls_corr, ho + oLC, ncl * 16);
    if (ls_inlier && ncl) memcpy(ls_inlier, ho + oLI, ncl);
    return PLSLAM_OK;
}

int plslam_loop_closure_verify_dev(plslam_ctx* ctx, const plslam_lc_params* params, const plslam_lc_keyframe* kf0,
                                   const plslam_lc_keyframe* kf1, plslam_lc_result* result, int32_t* pt_corr,
                                   uint8_t* pt_inlier, int32_t* ls_corr, uint8_t* ls_inlier, void* stream)
{
    using namespace plslam;
    int rc;
    PLSLAM_REQUIRE(ctx && result, PLSLAM_EINVAL);
    if ((rc = check_params(params)) || (rc = check_kf(kf0)) || (rc = check_kf(kf1))) return rc;
    PLSLAM_REQUIRE(kf0->n_pt == 0 || (pt_corr && pt_inlier), PLSLAM_EINVAL);
    PLSLAM_REQUIRE(kf0->n_ls == 0 || (ls_corr && ls_inlier), PLSLAM_EINVAL);
    std::lock_guard<std::mutex> lk(ctx->mu);
    DeviceGuard guard(ctx->device);
    hipStream_t us = static_cast<hipStream_t>(stream);
    if ((rc = fence_enter(ctx, us))) return rc;
    LcArgs a{};
    a.res = result;
    a.pt_corr = pt_corr; a.pt_inl = pt_inlier; a.ls_corr = ls_corr; a.ls_inl = ls_inlier;
    if ((rc = enqueue_verify(ctx, params, kf0, kf1, a))) return rc;
    return fence_leave(ctx, us);
}

int plslam_relpose_robust_gn(plslam_ctx* ctx, const plslam_lc_params* params, const double* P, const double* pl_obs,
                             int32_t npt, const double* sPeP, const double* le_obs, int32_t nls, plslam_lc_result* result,
                             uint8_t* pt_inlier, uint8_t* ls_inlier)
{
    using namespace plslam;
    int rc;
    PLSLAM_REQUIRE(ctx && result && npt >= 0 && nls >= 0, PLSLAM_EINVAL);
    if ((rc = check_params(params))) return rc;
    PLSLAM_REQUIRE(npt == 0 || (P && pl_obs), PLSLAM_EINVAL);
    PLSLAM_REQUIRE(nls == 0 || (sPeP && le_obs), PLSLAM_EINVAL);
    PLSLAM_REQUIRE(npt <= PLSLAM_LC_MAX_FEATURES && nls <= PLSLAM_LC_MAX_FEATURES, PLSLAM_ERANGE);
    std::lock_guard<std::mutex> lk(ctx->mu);
    DeviceGuard guard(ctx->device);
    hipStream_t s = ctx->stream;
    StreamSyncOnError sync_on_error(s);
    const size_t np = (size_t)npt, nl = (size_t)nls;
    Carver ci;
    const size_t oP = ci.take(np * 24), oO = ci.take(np * 16), oS = ci.take(nl * 48), oL = ci.take(nl * 24);
    Carver co;
    const size_t oR = co.take(sizeof(plslam_lc_result)), oPC = co.take(np * 16), oPI = co.take(np), oLC = co.take(nl * 16),
                 oLI = co.take(nl);
    if ((rc = ctx->pin_in.reserve(ci.off + 256))) return rc;
    if ((rc = ctx->lc_in.reserve(ci.off + 256))) return rc;
    if ((rc = ctx->pin_out.reserve(co.off))) return rc;
    if ((rc = ctx->lc_out.reserve(co.off))) return rc;
    char* h = ctx->pin_in.as<char>();
    char* d = ctx->lc_in.as<char>();
    if (np) { memcpy(h + oP, P, np * 24); memcpy(h + oO, pl_obs, np * 16); }
    if (nl) { memcpy(h + oS, sPeP, nl * 48); memcpy(h + oL, le_obs, nl * 24); }
    if (ci.off) PLSLAM_HIP_CHECK(hipMemcpyAsync(d, h, ci.off, hipMemcpyHostToDevice, s));
    char* od = ctx->lc_out.as<char>();
    LcArgs a{};
    fill_args(a, params);
    a.P = (const double*)(d + oP); a.pl = (const double*)(d + oO); a.sPeP = (const double*)(d + oS); a.le = (const double*)(d + oL);
    a.n_pt0 = a.n_pt1 = npt; a.n_ls0 = a.n_ls1 = nls;
    a.identity = 1;
    a.res = (plslam_lc_result*)(od + oR);
    a.pt_corr = (int32_t*)(od + oPC); a.pt_inl = (uint8_t*)(od + oPI);
    a.ls_corr = (int32_t*)(od + oLC); a.ls_inl = (uint8_t*)(od + oLI);
    hipLaunchKernelGGL(k_loop_closure, dim3(1), dim3(LC_THREADS), 0, s, a);
    PLSLAM_HIP_CHECK(hipGetLastError());
    PLSLAM_HIP_CHECK(hipMemcpyAsync(ctx->pin_out.p, od, co.off, hipMemcpyDeviceToHost, s));
    PLSLAM_HIP_CHECK(hipStreamSynchronize(s));
    sync_on_error.dismiss();
    const char* ho = ctx->pin_out.as<char>();
    memcpy(result, ho + oR, sizeof(plslam_lc_result));
    if (pt_inlier && np) memcpy(pt_inlier, ho + oPI, np);
    if (ls_inlier && nl) memcpy(ls_inlier, ho + oLI, nl);
    return PLSLAM_OK;
}

int plslam_lc_batch_create(plslam_ctx* ctx, const plslam_lc_params* params, int32_t max_pairs, plslam_lc_batch** out)
{
    using namespace plslam;
    int rc;
    PLSLAM_REQUIRE(ctx && out, PLSLAM_EINVAL);
    *out = nullptr;
    if ((rc = check_params(params))) return rc;
    PLSLAM_REQUIRE(max_pairs >= 1, PLSLAM_EINVAL);
    PLSLAM_REQUIRE(max_pairs <= PLSLAM_LC_MAX_BATCH, PLSLAM_ERANGE);
    plslam_lc_batch* bt = new (std::nothrow) plslam_lc_batch();
    PLSLAM_REQUIRE(bt != nullptr, PLSLAM_ENOMEM);
    bt->ctx = ctx;
    bt->p = *params;
    bt->max_pairs = max_pairs;
    *out = bt;
    return PLSLAM_OK;
}

void plslam_lc_batch_destroy(plslam_lc_batch* batch)
{
    using namespace plslam;
    if (!batch) return;
    {
        std::lock_guard<std::mutex> lk(batch->ctx->mu);
        DeviceGuard guard(batch->ctx->device);
        (void)hipStreamSynchronize(batch->ctx->stream);
        match_plan_release(batch->plan);
        batch->tab.release(); batch->args.release(); batch->in.release(); batch->out.release();
        batch->pin_in.release(); batch->pin_out.release();
    }
    delete batch;
}

int plslam_lc_batch_verify_dev(plslam_lc_batch* batch, const plslam_lc_keyframe* kf0, const plslam_lc_keyframe* kf1, int32_t B,
                               plslam_lc_result* results, int32_t* pt_corr, uint8_t* pt_inlier, int32_t* ls_corr,
                               uint8_t* ls_inlier, void* stream)
{
    using namespace plslam;
    int rc;
    if ((rc = check_batch(batch, kf0, kf1, B))) return rc;
    if (B == 0) return PLSLAM_OK;
    PLSLAM_REQUIRE(results != nullptr, PLSLAM_EINVAL);
    bool any_pt = false, any_ls = false;
    for (int32_t b = 0; b < B; ++b) { any_pt = any_pt || kf0[b].n_pt > 0; any_ls = any_ls || kf0[b].n_ls > 0; }
    PLSLAM_REQUIRE(!any_pt || (pt_corr && pt_inlier), PLSLAM_EINVAL);
    PLSLAM_REQUIRE(!any_ls || (ls_corr && ls_inlier), PLSLAM_EINVAL);
    plslam_ctx* ctx = batch->ctx;
    std::lock_guard<std::mutex> lk(ctx->mu);
    DeviceGuard guard(ctx->device);
    hipStream_t us = static_cast<hipStream_t>(stream);
    if ((rc = fence_enter(ctx, us))) return rc;
    if ((rc = enqueue_batch(batch, kf0, kf1, B, results, pt_corr, pt_inlier, ls_corr, ls_inlier))) return rc;
    return fence_leave(ctx, us);
}

int plslam_lc_batch_verify(plslam_lc_batch* batch, const plslam_lc_keyframe* kf0, const plslam_lc_keyframe* kf1, int32_t B,
                           plslam_lc_result* results, int32_t* pt_corr, uint8_t* pt_inlier, int32_t* ls_corr, uint8_t* ls_inlier)
{
    using namespace plslam;
    int rc;
    if ((rc = check_batch(batch, kf0, kf1, B))) return rc;
    if (B == 0) return PLSLAM_OK;
    PLSLAM_REQUIRE(results != nullptr, PLSLAM_EINVAL);
    plslam_ctx* ctx = batch->ctx;
    std::lock_guard<std::mutex> lk(ctx->mu);
    DeviceGuard guard(ctx->device);
    hipStream_t s = ctx->stream;
    StreamSyncOnError sync_on_error(s);
    // one page-locked image of every DISTINCT keyframe record (the top-K shape repeats kf1) -> one upload
    const size_t n2 = 2 * (size_t)B;
    auto rec = [&](size_t q) -> const plslam_lc_keyframe& { return q < (size_t)B ? kf0[q] : kf1[q - (size_t)B]; };
    std::vector<size_t> first(n2);
    std::vector<size_t> off(n2 * 8, 0);
    Carver ci;
    for (size_t q = 0; q < n2; ++q) {
        first[q] = q;
        for (size_t r = 0; r < q; ++r)
            if (first[r] == r && rec(r).pdesc == rec(q).pdesc && memcmp(&rec(r), &rec(q), sizeof(plslam_lc_keyframe)) == 0) { first[q] = r; break; }
        if (first[q] != q) continue;
        const size_t np = (size_t)rec(q).n_pt, nl = (size_t)rec(q).n_ls;
        size_t* o = &off[q * 8];
        o[0] = ci.take(np * 32); o[1] = ci.take(np * 24); o[2] = ci.take(np * 16); o[3] = ci.take(np * 4);
        o[4] = ci.take(nl * 32); o[5] = ci.take(nl * 48); o[6] = ci.take(nl * 24); o[7] = ci.take(nl * 4);
    }
    size_t sp = 0, sl = 0;
    for (int32_t b = 0; b < B; ++b) { sp += (size_t)kf0[b].n_pt; sl += (size_t)kf0[b].n_ls; }
    Carver co;
    const size_t oR = co.take((size_t)B * sizeof(plslam_lc_result)), oPC = co.take(sp * 16), oPI = co.take(sp),
                 oLC = co.take(sl * 16), oLI = co.take(sl);
    if ((rc = batch->pin_in.reserve(ci.off + 256))) return rc;
    if ((rc = batch->in.reserve(ci.off + 256))) return rc;
    if ((rc = batch->pin_out.reserve(co.off))) return rc;
    if ((rc = batch->out.reserve(co.off))) return rc;
    char* h = batch->pin_in.as<char>();
    char* d = batch->in.as<char>();
    batch->d_kf.assign(n2, plslam_lc_keyframe{});
    for (size_t q = 0; q < n2; ++q) {
        if (first[q] != q) { batch->d_kf[q] = batch->d_kf[first[q]]; continue; }
        const plslam_lc_keyframe& k = rec(q);
        const size_t np = (size_t)k.n_pt, nl = (size_t)k.n_ls;
        const size_t* o = &off[q * 8];
        if (np) {
            memcpy(h + o[0], k.pdesc, np * 32); memcpy(h + o[1], k.P, np * 24); memcpy(h + o[2], k.pl, np * 16);
            if (k.pt_idx) memcpy(h + o[3], k.pt_idx, np * 4);
        }
        if (nl) {
            memcpy(h + o[4], k.ldesc, nl * 32); memcpy(h + o[5], k.sPeP, nl * 48); memcpy(h + o[6], k.le, nl * 24);
            if (k.ls_idx) memcpy(h + o[7], k.ls_idx, nl * 4);
        }
        plslam_lc_keyframe& D = batch->d_kf[q];
        D.n_pt = k.n_pt; D.n_ls = k.n_ls;
        D.pdesc = (const uint8_t*)(d + o[0]); D.P = (const double*)(d + o[1]); D.pl = (const double*)(d + o[2]);
        D.pt_idx = k.pt_idx ? (const int32_t*)(d + o[3]) : nullptr;
        D.ldesc = (const uint8_t*)(d + o[4]); D.sPeP = (const double*)(d + o[5]); D.le = (const double*)(d + o[6]);
        D.ls_idx = k.ls_idx ? (const int32_t*)(d + o[7]) : nullptr;
    }
    if (ci.off) PLSLAM_HIP_CHECK(hipMemcpyAsync(d, h, ci.off, hipMemcpyHostToDevice, s));
    char* od = batch->out.as<char>();
    if ((rc = enqueue_batch(batch, batch->d_kf.data(), batch->d_kf.data() + B, B, (plslam_lc_result*)(od + oR), (int32_t*)(od + oPC),
                            (uint8_t*)(od + oPI), (int32_t*)(od + oLC), (uint8_t*)(od + oLI))))
        return rc;
    PLSLAM_HIP_CHECK(hipMemcpyAsync(batch->pin_out.p, od, co.off, hipMemcpyDeviceToHost, s));
    PLSLAM_HIP_CHECK(hipStreamSynchronize(s));
    sync_on_error.dismiss();
    const char* ho = batch->pin_out.as<char>();
    memcpy(results, ho + oR, (size_t)B * sizeof(plslam_lc_result));
    size_t rp = 0, rl = 0;
    for (int32_t b = 0; b < B; ++b) {
        const size_t ncp = (size_t)results[b].common_pt, ncl = (size_t)results[b].common_ls;
        if (pt_corr && ncp) memcpy(pt_corr + 4 * rp, ho + oPC + 16 * rp, ncp * 16);
        if (pt_inlier && ncp) memcpy(pt_inlier + rp, ho + oPI + rp, ncp);
        if (ls_corr && ncl) memcpy(ls_corr + 4 * rl, ho + oLC + 16 * rl, ncl * 16);
        if (ls_inlier && ncl) memcpy(ls_inlier + rl, ho + oLI + rl, ncl);
        rp += (size_t)kf0[b].n_pt;
        rl += (size_t)kf0[b].n_ls;
    }
    return PLSLAM_OK;
}

int plslam_relpose_robust_gn_batched_dev(plslam_ctx* ctx, const plslam_lc_params* params, const double* P, const double* pl_obs,
                                         const int32_t* pt_off, const double* sPeP, const double* le_obs, const int32_t* ls_off,
                                         int32_t B, plslam_lc_result* results, uint8_t* pt_inlier, uint8_t* ls_inlier, void* stream)
{
    using namespace plslam;
    int rc;
    PLSLAM_REQUIRE(ctx != nullptr, PLSLAM_EINVAL);
    if ((rc = check_params(params))) return rc;
    PLSLAM_REQUIRE(B >= 0, PLSLAM_EINVAL);
    PLSLAM_REQUIRE(B <= PLSLAM_LC_MAX_BATCH, PLSLAM_ERANGE);
    if (B == 0) return PLSLAM_OK;
    PLSLAM_REQUIRE(results && pt_off && ls_off, PLSLAM_EINVAL);
    // (the counts live on the device: an array that a non-empty problem needs cannot be checked here)
    PLSLAM_REQUIRE((P != nullptr) == (pl_obs != nullptr) && (P == nullptr || pt_inlier != nullptr), PLSLAM_EINVAL);
    PLSLAM_REQUIRE((sPeP != nullptr) == (le_obs != nullptr) && (sPeP == nullptr || ls_inlier != nullptr), PLSLAM_EINVAL);
    PLSLAM_REQUIRE(P || sPeP, PLSLAM_EINVAL);
    std::lock_guard<std::mutex> lk(ctx->mu);
    DeviceGuard guard(ctx->device);
    hipStream_t us = static_cast<hipStream_t>(stream);
    const size_t bytes = (size_t)B * sizeof(LcArgs);
    if ((rc = ctx->lc_args.reserve(bytes))) return rc;
    ctx->lc_args_h.resize(bytes);
    LcArgs* h = reinterpret_cast<LcArgs*>(ctx->lc_args_h.data());
    LcArgs a{};
    fill_args(a, params);
    a.P = P; a.pl = pl_obs; a.sPeP = sPeP; a.le = le_obs;
    a.identity = 1;
    a.pt_inl = pt_inlier; a.ls_inl = ls_inlier;          // no correspondence rows: row k is (k, k)
    for (int32_t b = 0; b < B; ++b) {
        h[b] = a;
        h[b].res = results + b;
    }
    if ((rc = fence_enter(ctx, us))) return rc;
    PLSLAM_HIP_CHECK(hipMemcpyAsync(ctx->lc_args.p, h, bytes, hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(k_loop_closure_batched, dim3((unsigned)B), dim3(LC_THREADS), 0, ctx->stream, ctx->lc_args.as<LcArgs>(),
                       pt_off, ls_off);
    PLSLAM_HIP_CHECK(hipGetLastError());
    return fence_leave(ctx, us);
}

}  // extern "C"
