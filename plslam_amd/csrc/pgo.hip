// pgo.hip -- the loop-closure correction of the reference (MapHandler::loopClosureOptimizationCovGraphG2O,
// src/mapHandler.cpp:4185-4410, up to loopClosureFuseLandmarks()) on the device: the SE(3) pose graph over keyframes 0 ..
// kf_curr_idx optimised with g2o's Levenberg-Marquardt (as restated in tests/pgo_ref.py), the write-back
// of the poses and the rigid re-anchoring of every landmark.
//   K40 k_pgo_meas             a lane per edge: Z = SE3Quat::exp(reverse_se3(logmap_se3(T_i^-1 T_j))) or of the LC pose
//   K41 k_pgo_init             one workgroup: the :4220-4249 estimates, then computeInitialGuess along the host's BFS tree,
//                              level after level
//   K42 k_pgo_edges<JAC>       a lane per edge: e = toVectorMQT(Z^-1 X_i^-1 X_j), chi2_e, and (JAC) the exact Jacobians
//   K43 k_pgo_hblocks          a workgroup per envelope block: the sum of J^T J over its edges, in edge order
//   K44 k_pgo_rhs              a lane per unknown: b = -sum J^T e over the vertex's edges, in edge order
//   K45 k_env_factor<WIN>      one workgroup: L D L^T of (H + lambda I) over the envelope, right-looking, column by column,
//                              the forward solve fused (z = D^-1 L^-1 b); WIN: the active rows in a 128 x 128 LDS window
//   K46 k_env_backward<WIN>    one workgroup: L^T x = z, row by row, last first
//   K47 k_pgo_update           a lane per vertex: X' = X fromVectorMQT(dx) (active vertices), X' = X otherwise
//   K48 k_pgo_reduce           one workgroup: chi (fixed order), dx.(lambda dx + b), the bad-pivot flag: what crosses per trial
//   K49 k_pgo_writeback        a lane per vertex: log, expmap_se3, logmap_se3, T_corr; then the keyframes after kf_curr_idx
//   K50-K53 k_lc_*             the map correction: anchor entries per landmark (counts, scan, fill), then a lane per landmark
//                              applies its anchors' T_corr in anchor order to X, med_obs_dir and every dir_list entry
// Every sum has a fixed order (no floating-point atomics): two runs give the same bits.  Phases are ordered by kernel
// boundaries and, inside the one-workgroup kernels, by workgroup barriers only.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstring>
#include <limits>
#include <numeric>
#include <vector>

#include "common.hpp"
#include "se3_dev.hpp"

namespace plslam {
namespace {

constexpr int LT = 32;          // the dense comparison path's tile edge (ldlt_dense_dev.hpp)
typedef double dvec4_t __attribute__((ext_vector_type(4)));
#include "ldlt_dense_dev.hpp"

constexpr int ENV_W = 128;      // rows / columns of the LDS window (128 x 128 doubles: 128 KiB)
constexpr int ENV_G = 16;       // rows loaded into the window at a time
constexpr int ENV_MAXBW_WIN = ENV_W - ENV_G;   // widest envelope (r - first column of row r) the window takes

struct PgoLevel { int32_t v, u, e, first; };  // BFS tree: vertex v set from parent u through edge e (first: u is the edge's first vertex)
struct PgoTarget { int32_t row, col, c0, c1; };  // envelope block (row block >= col block) and its contribution range
struct PgoStats { double chi, scale; int32_t bad, pad; };

// ---- isometries (R row-major, t) and g2o's maps -----------------------------------------------------------------------------
struct Iso { double R[9], t[3]; };

__device__ __forceinline__ void iso_load(const double* __restrict__ p, Iso& X)
{
#pragma unroll
    for (int a = 0; a < 9; ++a) X.R[a] = p[a];
#pragma unroll
    for (int a = 0; a < 3; ++a) X.t[a] = p[9 + a];
}
__device__ __forceinline__ void iso_store(const Iso& X, double* __restrict__ p)
{
#pragma unroll
    for (int a = 0; a < 9; ++a) p[a] = X.R[a];
#pragma unroll
    for (int a = 0; a < 3; ++a) p[9 + a] = X.t[a];
}
__device__ __forceinline__ void iso_mul(const Iso& A, const Iso& B, Iso& C)
{
    mat3_mul(A.R, B.R, C.R);
    double u[3];
    mv3(A.R, B.t, u);         // (not xform(A.R, A.t, B.t, C.t): the same sums, but the kernels' instruction streams change)
#pragma unroll
    for (int i = 0; i < 3; ++i) C.t[i] = u[i] + A.t[i];
}
// (not inv_pose: that one negates the factors, this one the finished sum, as g2o's Isometry3::inverse does)
__device__ __forceinline__ void iso_inv(const Iso& A, Iso& C)
{
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) C.R[3 * i + j] = A.R[3 * j + i];
    double u[3];
    mv3(C.R, A.t, u);
#pragma unroll
    for (int i = 0; i < 3; ++i) C.t[i] = -u[i];
}
// Eigen's Quaternion(const Matrix3&) -> (w, x, y, z)
__device__ __forceinline__ void quat_from_R(const double R[9], double q[4])
{
    const double tr = R[0] + R[4] + R[8];
    if (tr > 0.0) {
        double t = sqrt(tr + 1.0);
        q[0] = 0.5 * t;
        t = 0.5 / t;
        q[1] = (R[7] - R[5]) * t;
        q[2] = (R[2] - R[6]) * t;
        q[3] = (R[3] - R[1]) * t;
    } else {
        int i = 0;
        if (R[4] > R[0]) i = 1;
        if (R[8] > R[4 * i]) i = 2;
        const int j = (i + 1) % 3, k = (j + 1) % 3;
        double t = sqrt(R[4 * i] - R[4 * j] - R[4 * k] + 1.0);
        q[1 + i] = 0.5 * t;
        t = 0.5 / t;
        q[0] = (R[3 * k + j] - R[3 * j + k]) * t;
        q[1 + j] = (R[3 * j + i] + R[3 * i + j]) * t;
        q[1 + k] = (R[3 * k + i] + R[3 * i + k]) * t;
    }
}
__device__ __forceinline__ void unit_quat(const double R[9], double q[4])
{
    quat_from_R(R, q);
    const double n = sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
#pragma unroll
    for (int a = 0; a < 4; ++a) q[a] /= n;
    if (q[0] < 0.0) {
#pragma unroll
        for (int a = 0; a < 4; ++a) q[a] = -q[a];
    }
}
__device__ __forceinline__ void R_from_quat(const double q[4], double R[9])
{
    const double w = q[0], x = q[1], y = q[2], z = q[3];
    const double tx = 2.0 * x, ty = 2.0 * y, tz = 2.0 * z;
    const double twx = tx * w, twy = ty * w, twz = tz * w, txx = tx * x, txy = ty * x, txz = tz * x, tyy = ty * y, tyz = tz * y,
                 tzz = tz * z;
    R[0] = 1.0 - (tyy + tzz); R[1] = txy - twz;         R[2] = txz + twy;
    R[3] = txy + twz;         R[4] = 1.0 - (txx + tzz); R[5] = tyz - twx;
    R[6] = txz - twy;         R[7] = tyz + twx;         R[8] = 1.0 - (txx + tyy);
}
// SE3Quat::exp([omega; upsilon]) as an isometry (constants: tests/pgo_ref.py G2O)
__device__ __forceinline__ void se3quat_exp(const double u[6], Iso& X)
{
    const double w[3] = {u[0], u[1], u[2]};
    const double theta = sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]);
    double Om[9], Om2[9], R[9], V[9];
    skew3(w, Om);
    mat3_mul(Om, Om, Om2);
    if (theta < 1e-5) {
#pragma unroll
        for (int k = 0; k < 9; ++k) { R[k] = ((k % 4 == 0) ? 1.0 : 0.0) + Om[k] + Om2[k]; V[k] = R[k]; }
    } else {
        const double t2 = theta * theta, s = sin(theta), c = cos(theta);
        const double a = s / theta, b = (1.0 - c) / t2, d = (theta - s) / (t2 * theta);
#pragma unroll
        for (int k = 0; k < 9; ++k) {
            const double id = (k % 4 == 0) ? 1.0 : 0.0;
            R[k] = id + a * Om[k] + b * Om2[k];
            V[k] = id + b * Om[k] + d * Om2[k];
        }
    }
    double q[4];
    unit_quat(R, q);
    R_from_quat(q, X.R);
    mv3(V, u + 3, X.t);
}
// SE3Quat(estimate()).log() -> [omega; V^-1 t]
__device__ __forceinline__ void se3quat_log(const Iso& X, double u[6])
{
    double q[4], R[9];
    unit_quat(X.R, q);
    R_from_quat(q, R);
    const double d = 0.5 * (R[0] + R[4] + R[8] - 1.0);
    const double dR[3] = {R[7] - R[5], R[2] - R[6], R[3] - R[1]};
    double w[3], Om[9], Om2[9], Vi[9];
    if (d > 0.99999) {
#pragma unroll
        for (int a = 0; a < 3; ++a) w[a] = 0.5 * dR[a];
        skew3(w, Om);
        mat3_mul(Om, Om, Om2);
#pragma unroll
        for (int k = 0; k < 9; ++k) Vi[k] = ((k % 4 == 0) ? 1.0 : 0.0) - 0.5 * Om[k] + Om2[k] / 12.0;
    } else {
        const double theta = acos(d);
        const double f = theta / (2.0 * sqrt(1.0 - d * d));
#pragma unroll
        for (int a = 0; a < 3; ++a) w[a] = f * dR[a];
        skew3(w, Om);
        mat3_mul(Om, Om, Om2);
        const double g = (1.0 - theta / (2.0 * tan(theta / 2.0))) / (theta * theta);
#pragma unroll
        for (int k = 0; k < 9; ++k) Vi[k] = ((k % 4 == 0) ? 1.0 : 0.0) - 0.5 * Om[k] + g * Om2[k];
    }
    u[0] = w[0]; u[1] = w[1]; u[2] = w[2];
    mv3(Vi, X.t, u + 3);
}
__device__ __forceinline__ void from_vector_mqt(const double v[6], Iso& X)
{
    const double n = 1.0 - (v[3] * v[3] + v[4] * v[4] + v[5] * v[5]);
    if (n < 0.0) {
#pragma unroll
        for (int k = 0; k < 9; ++k) X.R[k] = (k % 4 == 0) ? 1.0 : 0.0;
    } else {
        const double q[4] = {sqrt(n), v[3], v[4], v[5]};
        R_from_quat(q, X.R);
    }
    X.t[0] = v[0]; X.t[1] = v[1]; X.t[2] = v[2];
}
__device__ __forceinline__ void mat4_mul(const double a[16], const double b[16], double c[16])
{
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
            c[4 * i + j] = a[4 * i] * b[j] + a[4 * i + 1] * b[4 + j] + a[4 * i + 2] * b[8 + j] + a[4 * i + 3] * b[12 + j];
}
__device__ __forceinline__ void rev6(const double x[6], double u[6])
{
    u[0] = x[3]; u[1] = x[4]; u[2] = x[5]; u[3] = x[0]; u[4] = x[1]; u[5] = x[2];
}

// ---- K40: measurements ------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
k_pgo_meas(const int2* __restrict__ ev, const int32_t* __restrict__ elc, int32_t ne, const int32_t* __restrict__ vslot,
           const double* __restrict__ T, const double* __restrict__ lc_pose, double* __restrict__ Z)
{
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= ne) return;
    double x[6], u[6];
    if (elc[e] < 0) {
        double Ti[16], Tj[16], Tii[16], Tij[16];
        const int2 p = ev[e];                       // vertices; their map slots index the stored poses
        const size_t si = (size_t)vslot[p.x], sj = (size_t)vslot[p.y];
#pragma unroll
        for (int a = 0; a < 16; ++a) { Ti[a] = T[16 * si + a]; Tj[a] = T[16 * sj + a]; }
        inverse_se3(Ti, Tii);
        mat4_mul(Tii, Tj, Tij);
        logmap_se3(Tij, x);
    } else {
#pragma unroll
        for (int a = 0; a < 6; ++a) x[a] = lc_pose[6 * (size_t)elc[e] + a];
    }
    rev6(x, u);
    Iso Zi;
    se3quat_exp(u, Zi);
    iso_store(Zi, Z + 12 * (size_t)e);
}

// ---- K41: the initial estimates and computeInitialGuess -------------------------------------------------------------------
// vinit[v] = (map slot, LC entry whose (0)-end this vertex is not but whose (1)-end it is, else -1)
__global__ void __launch_bounds__(256)
k_pgo_init(const int2* __restrict__ vinit, int32_t nv, const double* __restrict__ T, const double* __restrict__ x_kf,
           const int32_t* __restrict__ lc_idx, const double* __restrict__ lc_pose, const PgoLevel* __restrict__ tree,
           const int32_t* __restrict__ lvl_ptr, int32_t nlvl, const double* __restrict__ Z, double* __restrict__ X0,
           double* __restrict__ X)
{
    const int t = threadIdx.x;
    for (int v = t; v < nv; v += 256) {
        const int2 vi = vinit[v];
        double x[6], u[6];
        if (vi.y >= 0) {
            double E[16], Ta[16], P[16];
            expmap_se3(lc_pose + 6 * (size_t)vi.y, E);
            const int a = lc_idx[3 * vi.y];
#pragma unroll
            for (int k = 0; k < 16; ++k) Ta[k] = T[16 * (size_t)a + k];
            mat4_mul(E, Ta, P);
            logmap_se3(P, x);
        } else {
#pragma unroll
            for (int k = 0; k < 6; ++k) x[k] = x_kf[6 * (size_t)vi.x + k];
        }
        rev6(x, u);
        Iso Xv;
        se3quat_exp(u, Xv);
        iso_store(Xv, X0 + 12 * (size_t)v);
        iso_store(Xv, X + 12 * (size_t)v);
    }
    for (int l = 0; l < nlvl; ++l) {
        __syncthreads();
        for (int k = lvl_ptr[l] + t; k < lvl_ptr[l + 1]; k += 256) {
            const PgoLevel L = tree[k];
            Iso Xu, Ze, Zi, Xv;
            iso_load(X + 12 * (size_t)L.u, Xu);
            iso_load(Z + 12 * (size_t)L.e, Ze);
            if (L.first) iso_mul(Xu, Ze, Xv);
            else { iso_inv(Ze, Zi); iso_mul(Xu, Zi, Xv); }
            iso_store(Xv, X + 12 * (size_t)L.v);
        }
    }
}

// ---- K42: edge errors and Jacobians ------------------------------------------------------------------------------------------
// J layout per edge: J_i (6 x 6 row-major), then J_j
template <bool JAC>
__global__ void __launch_bounds__(256)
k_pgo_edges(const int2* __restrict__ evs, int32_t ne, const double* __restrict__ Z, const double* __restrict__ X,
            double* __restrict__ err, double* __restrict__ J, double* __restrict__ chi2)
{
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= ne) return;
    const int2 p = evs[e];
    Iso Ze, Xi, Xj, A, Xii, AX, E;
    iso_load(Z + 12 * (size_t)e, Ze);
    iso_load(X + 12 * (size_t)p.x, Xi);
    iso_load(X + 12 * (size_t)p.y, Xj);
    iso_inv(Ze, A);
    iso_inv(Xi, Xii);
    iso_mul(A, Xii, AX);
    iso_mul(AX, Xj, E);
    double q[4];
    unit_quat(E.R, q);
    const double ev[6] = {E.t[0], E.t[1], E.t[2], q[1], q[2], q[3]};
    double c = 0.0;
#pragma unroll
    for (int a = 0; a < 6; ++a) c += ev[a] * ev[a];
    chi2[e] = c;
    if (!JAC) return;
#pragma unroll
    for (int a = 0; a < 6; ++a) err[6 * (size_t)e + a] = ev[a];
    Iso B, EB;
    iso_mul(Xii, Xj, B);
    iso_mul(A, B, EB);
    double qb[4];
    unit_quat(EB.R, qb);
    const double w = qb[0], v[3] = {qb[1], qb[2], qb[3]};
    double S[9], Sb[9];
    skew3(v, S);
    skew3(B.t, Sb);
    double Ji[36], Jj[36];
#pragma unroll
    for (int k = 0; k < 36; ++k) { Ji[k] = 0.0; Jj[k] = 0.0; }
    double RS[9], M[9], Mr[9];
    mat3_mul(A.R, Sb, RS);
#pragma unroll
    for (int k = 0; k < 9; ++k) {
        const double id = (k % 4 == 0) ? 1.0 : 0.0;
        M[k] = w * id + S[k];      // w I + [v]x
        Mr[k] = w * id - S[k];     // w I - [v]x
    }
    double MA[9];
    mat3_mul(Mr, A.R, MA);
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c2 = 0; c2 < 3; ++c2) {
            Jj[6 * r + c2] = EB.R[3 * r + c2];
            Jj[6 * (r + 3) + 3 + c2] = M[3 * r + c2];
            Ji[6 * r + c2] = -A.R[3 * r + c2];
            Ji[6 * r + 3 + c2] = 2.0 * RS[3 * r + c2];
            Ji[6 * (r + 3) + 3 + c2] = -MA[3 * r + c2];
        }
    double* o = J + 72 * (size_t)e;
#pragma unroll
    for (int k = 0; k < 36; ++k) { o[k] = Ji[k]; o[36 + k] = Jj[k]; }
}

// ---- K43: Hessian blocks in the envelope ------------------------------------------------------------------------------------
// contribution code c: edge = c >> 2, kind = c & 3: 0 J_i^T J_i, 1 J_j^T J_j, 2 J_i^T J_j, 3 J_j^T J_i
__global__ void __launch_bounds__(64)
k_pgo_hblocks(const PgoTarget* __restrict__ tg, const int32_t* __restrict__ contrib, const double* __restrict__ J,
              const int64_t* __restrict__ off, const int32_t* __restrict__ cs, double* __restrict__ H)
{
    const PgoTarget T = tg[blockIdx.x];
    const int t = threadIdx.x;
    if (t >= 36) return;
    const int r = t / 6, c = t % 6;
    const int64_t gr = 6 * (int64_t)T.row + r, gc = 6 * (int64_t)T.col + c;
    if (gc > gr) return;
    double acc = 0.0;
    for (int k = T.c0; k < T.c1; ++k) {
        const int32_t code = contrib[k];
        const int kind = code & 3;
        const double* Je = J + 72 * (size_t)(code >> 2);
        const double* Ja = Je + ((kind == 1 || kind == 3) ? 36 : 0);
        const double* Jb = Je + ((kind == 1 || kind == 2) ? 36 : 0);
        double s = 0.0;
#pragma unroll
        for (int m = 0; m < 6; ++m) s += Ja[6 * m + r] * Jb[6 * m + c];
        acc += s;
    }
    H[off[gr] + (gc - cs[gr])] = acc;
}

// ---- K44: b = -sum J^T e -----------------------------------------------------------------------------------------------------
// rhs_list entry: edge << 1 | side (0: the vertex is the edge's first end)
__global__ void __launch_bounds__(256)
k_pgo_rhs(const int32_t* __restrict__ rptr, const int32_t* __restrict__ rlist, int32_t na, const double* __restrict__ J,
          const double* __restrict__ err, double* __restrict__ b)
{
    const int g = blockIdx.x * 256 + threadIdx.x;
    if (g >= 6 * na) return;
    const int p = g / 6, r = g % 6;
    double acc = 0.0;
    for (int k = rptr[p]; k < rptr[p + 1]; ++k) {
        const int32_t code = rlist[k];
        const int e = code >> 1;
        const double* Jv = J + 72 * (size_t)e + 36 * (code & 1);
        double s = 0.0;
#pragma unroll
        for (int m = 0; m < 6; ++m) s += Jv[6 * m + r] * err[6 * (size_t)e + m];
        acc -= s;
    }
    b[g] = acc;
}

// ---- K45: envelope L D L^T with the forward solve ---------------------------------------------------------------------------
// Row r holds columns cs[r] .. r at off[r]; reach[k] = the last row whose envelope reaches column k.  In: H (lower envelope),
// lambda (added to the diagonal on load), b.  Out: L (strict lower) and D (diagonal) in Lo, z = D^-1 L^-1 b, bad pivots.
// WIN: the rows that column k updates lie in a 128 x 128 LDS window (row r in slot r mod 128); rows enter 16 at a time once
// the 16 rows before them are done.  !WIN: the same arithmetic on Lo in global memory.
template <bool WIN>
__global__ void __launch_bounds__(256)
k_env_factor(const double* __restrict__ H, const int64_t* __restrict__ off, const int32_t* __restrict__ cs,
             const int32_t* __restrict__ reach, int32_t N, double lambda, const double* __restrict__ b, double* __restrict__ Lo,
             double* __restrict__ z, double* __restrict__ bg, int32_t* __restrict__ nbad)
{
    constexpr int M = ENV_W - 1;
    __shared__ double win[WIN ? ENV_W * ENV_W : 1];
    __shared__ double bb[WIN ? ENV_W : 1];
    __shared__ double col[ENV_W];
    const int t = threadIdx.x, tx = t & 15, ty = t >> 4;
    auto load_row = [&](int r) {          // row r of H + lambda I into its window slot (WIN), columns r - 127 .. r
        const int c0 = cs[r];
        const int64_t o = off[r];
        for (int c = tx; c < ENV_W; c += 16) {
            const int j = r - c;
            double v = 0.0;
            if (j >= c0) v = H[o + (j - c0)] + (j == r ? lambda : 0.0);
            win[(r & M) * ENV_W + (j & M)] = v;
        }
        if (tx == 0) bb[r & M] = b[r];
    };
    auto A = [&](int i, int j) -> double& {
        if constexpr (WIN) return win[(i & M) * ENV_W + (j & M)];
        else return Lo[off[i] + (j - cs[i])];
    };
    if constexpr (WIN) {
        for (int r = ty; r < min(N, ENV_W); r += 16) load_row(r);
    } else {
        for (int r = t; r < N; r += 256) {
            for (int j = cs[r]; j <= r; ++j) Lo[off[r] + (j - cs[r])] = H[off[r] + (j - cs[r])] + (j == r ? lambda : 0.0);
            bg[r] = b[r];
        }
    }
    int bad = 0;
    __syncthreads();
    for (int k = 0; k < N; ++k) {
        const double d = A(k, k);
        const double yk = WIN ? bb[k & M] : bg[k];
        const int R = reach[k];
        const int w = R - k;
        if (t == 0) {
            if (!(d != 0.0 && isfinite(d))) ++bad;
            Lo[off[k] + (k - cs[k])] = d;
            z[k] = yk / d;
        }
        for (int ii = t; ii < w; ii += 256) {
            const int i = k + 1 + ii;
            double l = 0.0;
            if (k >= cs[i]) {
                l = A(i, k) / d;
                Lo[off[i] + (k - cs[i])] = l;
            }
            if constexpr (WIN) { col[ii] = l; bb[i & M] -= l * yk; }
            else bg[i] -= l * yk;
        }
        __syncthreads();
        // !WIN: l_i is read back from Lo (rows whose envelope starts after column k have l_i = 0 and are skipped)
        auto lk = [&](int ii) -> double {
            if constexpr (WIN) return col[ii];
            const int i = k + 1 + ii;
            return k >= cs[i] ? Lo[off[i] + (k - cs[i])] : 0.0;
        };
        for (int ii = ty; ii < w; ii += 16) {
            const int i = k + 1 + ii;
            if (!WIN && k < cs[i]) continue;
            const double li = lk(ii);
            for (int jj = tx; jj <= ii; jj += 16) A(i, k + 1 + jj) -= li * (d * lk(jj));
        }
        if constexpr (WIN) {
            if ((k + 1) % ENV_G == 0)
                for (int r = k + 1 - ENV_G + ENV_W + ty; r <= k + ENV_W && r < N; r += 16) load_row(r);
        }
        __syncthreads();
    }
    if (t == 0) *nbad = bad;
}

// ---- K46: L^T x = z, last row first -----------------------------------------------------------------------------------------
template <bool WIN>
__global__ void __launch_bounds__(256)
k_env_backward(const double* __restrict__ Lo, const int64_t* __restrict__ off, const int32_t* __restrict__ cs, int32_t N,
               const double* __restrict__ z, double* __restrict__ zg, double* __restrict__ x)
{
    constexpr int M = ENV_W - 1;
    __shared__ double zb[ENV_W];
    const int t = threadIdx.x;
    if constexpr (WIN) {
        for (int j = t; j < ENV_W; j += 256) if (N - 1 - j >= 0) zb[(N - 1 - j) & M] = z[N - 1 - j];
    } else {
        for (int j = t; j < N; j += 256) zg[j] = z[j];
    }
    __syncthreads();
    for (int i = N - 1; i >= 0; --i) {
        const double xi = WIN ? zb[i & M] : zg[i];
        if (t == 0) x[i] = xi;
        const int c0 = cs[i];
        const int64_t o = off[i];
        for (int j = i - 1 - t; j >= c0; j -= 256) {
            const double l = Lo[o + (j - c0)];
            if constexpr (WIN) zb[j & M] -= l * xi;
            else zg[j] -= l * xi;
        }
        if constexpr (WIN) {
            // slot (i + 1) mod 128 was read by the previous row: it takes z[i + 1 - 128], first needed by row i - 1
            if (t == 0 && i + 1 - ENV_W >= 0 && i + 1 < N) zb[(i + 1) & M] = z[i + 1 - ENV_W];
        }
        __syncthreads();
    }
}

// the dense comparison path: the envelope into a zero-padded npad x npad S (+ lambda, unit padding), b into w
__global__ void __launch_bounds__(256)
k_env_to_dense(const double* __restrict__ H, const int64_t* __restrict__ off, const int32_t* __restrict__ cs, int32_t N,
               int64_t npad, double lambda, const double* __restrict__ b, double* __restrict__ S, double* __restrict__ w)
{
    const int r = blockIdx.x;
    if (r >= npad) return;
    if (r >= N) {
        if (threadIdx.x == 0) S[(int64_t)r * npad + r] = 1.0;
        return;
    }
    for (int j = cs[r] + threadIdx.x; j <= r; j += 256)
        S[(int64_t)r * npad + j] = H[off[r] + (j - cs[r])] + (j == r ? lambda : 0.0);
    if (threadIdx.x == 0) w[r] = b[r];
}
__global__ void __launch_bounds__(256)
k_count_bad(const int32_t* __restrict__ badp, int32_t nt, int32_t* __restrict__ nbad)
{
    if (threadIdx.x == 0) {
        int n = 0;
        for (int i = 0; i < nt; ++i) n += badp[i];
        *nbad = n;
    }
}

// ---- K47: the trial update ---------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
k_pgo_update(const int32_t* __restrict__ vcol, int32_t nv, const double* __restrict__ dx, const int32_t* __restrict__ nbad,
             const double* __restrict__ X, double* __restrict__ Y)
{
    const int v = blockIdx.x * 256 + threadIdx.x;
    if (v >= nv) return;
    Iso Xv, D, Yv;
    iso_load(X + 12 * (size_t)v, Xv);
    const int c = vcol[v];
    if (c < 0 || *nbad) { iso_store(Xv, Y + 12 * (size_t)v); return; }
    double d[6];
#pragma unroll
    for (int a = 0; a < 6; ++a) d[a] = dx[6 * (size_t)c + a];
    from_vector_mqt(d, D);
    iso_mul(Xv, D, Yv);
    iso_store(Yv, Y + 12 * (size_t)v);
}

// ---- K48: the scalars of a trial -------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
k_pgo_reduce(const double* __restrict__ chi2, int32_t ne, const double* __restrict__ dx, const double* __restrict__ b, int32_t N,
             double lambda, const int32_t* __restrict__ nbad, PgoStats* __restrict__ out)
{
    __shared__ double rc[256], rs[256];
    const int t = threadIdx.x;
    double c = 0.0, s = 0.0;
    for (int e = t; e < ne; e += 256) c += chi2[e];
    if (dx && !*nbad)
        for (int k = t; k < N; k += 256) s += dx[k] * (lambda * dx[k] + b[k]);
    rc[t] = c; rs[t] = s;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
        if (t < h) { rc[t] += rc[t + h]; rs[t] += rs[t + h]; }
        __syncthreads();
    }
    if (t == 0) { out->chi = rc[0]; out->scale = rs[0]; out->bad = nbad ? *nbad : 0; out->pad = 0; }
}

// ---- K49: write-back ---------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
k_pgo_writeback(const int32_t* __restrict__ vslot, const int32_t* __restrict__ vcol, int32_t nv, const double* __restrict__ X,
                const double* __restrict__ X0, const double* __restrict__ T, double* __restrict__ T_out, double* __restrict__ x_out,
                double* __restrict__ T_corr)
{
    const int v = blockIdx.x * 256 + threadIdx.x;
    if (v >= nv) return;
    const size_t k = (size_t)vslot[v];
    Iso Xv;
    iso_load((vcol[v] >= 0 ? X : X0) + 12 * (size_t)v, Xv);
    double u[6], x[6], Tk[16], Tp[16], Tpi[16], Tc[16];
    se3quat_log(Xv, u);
    rev6(u, x);
    expmap_se3(x, Tk);
    logmap_se3(Tk, u);
#pragma unroll
    for (int a = 0; a < 16; ++a) Tp[a] = T[16 * k + a];
    inverse_se3(Tp, Tpi);
    mat4_mul(Tk, Tpi, Tc);
#pragma unroll
    for (int a = 0; a < 16; ++a) { T_out[16 * k + a] = Tk[a]; T_corr[16 * k + a] = Tc[a]; }
#pragma unroll
    for (int a = 0; a < 6; ++a) x_out[6 * k + a] = u[a];
}
__global__ void __launch_bounds__(256)
k_pgo_later(const uint8_t* __restrict__ valid, int32_t k0, int32_t n, int32_t last, const double* __restrict__ T,
            double* __restrict__ T_out, double* __restrict__ x_out, double* __restrict__ T_corr, uint8_t* __restrict__ corrected)
{
    const int k = k0 + blockIdx.x * 256 + threadIdx.x;
    if (k >= n || !valid[k]) return;
    double C[16], Tk[16], To[16], u[6];
#pragma unroll
    for (int a = 0; a < 16; ++a) { C[a] = T_corr[16 * (size_t)last + a]; Tk[a] = T[16 * (size_t)k + a]; }
    mat4_mul(C, Tk, To);
    logmap_se3(To, u);
#pragma unroll
    for (int a = 0; a < 16; ++a) { T_out[16 * (size_t)k + a] = To[a]; T_corr[16 * (size_t)k + a] = C[a]; }
#pragma unroll
    for (int a = 0; a < 6; ++a) x_out[6 * (size_t)k + a] = u[a];
    corrected[k] = 1;
}

// ---- K50-K53: the map correction ---------------------------------------------------------------------------------------------
// K50: a lane per anchor entry: its slot (binary search of the CSR), a count per landmark that a corrected slot lists
__global__ void __launch_bounds__(256)
k_lc_count(const int32_t* __restrict__ aptr, int32_t nslot, const int32_t* __restrict__ aidx, int32_t na, int32_t nlm,
           const uint8_t* __restrict__ corrected, int32_t* __restrict__ eslot, int32_t* __restrict__ cnt)
{
    const int a = blockIdx.x * 256 + threadIdx.x;
    if (a >= na) return;
    int lo = 0, hi = nslot;                       // the last slot s with aptr[s] <= a
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (aptr[mid] <= a) lo = mid; else hi = mid;
    }
    const int j = aidx[a];
    const bool use = j >= 0 && j < nlm && corrected[lo];
    eslot[a] = use ? lo : -1;
    if (use) atomic_add_global(cnt + j, 1);
}
// K51: one workgroup: exclusive prefix sum of the counts -> ptr (n + 1); the fill cursors start at 0
__global__ void __launch_bounds__(1024)
k_lc_scan(int32_t* __restrict__ cnt, int32_t n, int32_t* __restrict__ ptr)
{
    __shared__ int32_t part[1024];
    const int t = threadIdx.x;
    const int per = (n + 1023) / 1024, a0 = min(n, t * per), a1 = min(n, a0 + per);
    int s = 0;
    for (int i = a0; i < a1; ++i) s += cnt[i];
    part[t] = s;
    __syncthreads();
    for (int h = 1; h < 1024; h <<= 1) {
        const int v = t >= h ? part[t - h] : 0;
        __syncthreads();
        part[t] += v;
        __syncthreads();
    }
    int run = t ? part[t - 1] : 0;
    for (int i = a0; i < a1; ++i) { ptr[i] = run; run += cnt[i]; cnt[i] = 0; }
    if (t == 1023) ptr[n] = part[1023];
}
// K52: a lane per anchor entry: its place in its landmark's list (the order inside a list is restored by K53)
__global__ void __launch_bounds__(256)
k_lc_fill(const int32_t* __restrict__ aidx, const int32_t* __restrict__ eslot, int32_t na, const int32_t* __restrict__ ptr,
          int32_t* __restrict__ cur, int32_t* __restrict__ list)
{
    const int a = blockIdx.x * 256 + threadIdx.x;
    if (a >= na || eslot[a] < 0) return;
    const int j = aidx[a];
    list[ptr[j] + atomic_add_global(cur + j, 1)] = a;
}
// K53: a lane per landmark: its anchor entries in CSR order (slot order), each applying that slot's T_corr
template <int DL>
__global__ void __launch_bounds__(256)
k_lc_apply(const int32_t* __restrict__ ptr, int32_t* __restrict__ list, const int32_t* __restrict__ eslot,
           const uint8_t* __restrict__ valid, int32_t n, const double* __restrict__ T_corr, double* __restrict__ X,
           double* __restrict__ med, const int32_t* __restrict__ dptr, double* __restrict__ dirs)
{
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= n || !valid[j]) return;
    const int p0 = ptr[j], p1 = ptr[j + 1];
    if (p1 == p0) return;
    for (int a = p0 + 1; a < p1; ++a) {           // insertion sort: the entries of one landmark are few
        const int v = list[a];
        int b = a - 1;
        while (b >= p0 && list[b] > v) { list[b + 1] = list[b]; --b; }
        list[b + 1] = v;
    }
    const int d0 = dptr[j], d1 = dptr[j + 1];
    for (int a = p0; a < p1; ++a) {
        const double* C = T_corr + 16 * (size_t)eslot[list[a]];
        double c[12];
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int q = 0; q < 4; ++q) c[4 * i + q] = C[4 * i + q];
        double p[3];
#pragma unroll
        for (int h = 0; h < DL / 3; ++h) {
#pragma unroll
            for (int q = 0; q < 3; ++q) p[q] = X[(size_t)DL * j + 3 * h + q];
            xform(c, p, p);
#pragma unroll
            for (int q = 0; q < 3; ++q) X[(size_t)DL * j + 3 * h + q] = p[q];
        }
#pragma unroll
        for (int q = 0; q < 3; ++q) p[q] = med[3 * (size_t)j + q];
        xform(c, p, p);
#pragma unroll
        for (int q = 0; q < 3; ++q) med[3 * (size_t)j + q] = p[q];
        for (int d = d0; d < d1; ++d) {
#pragma unroll
            for (int q = 0; q < 3; ++q) p[q] = dirs[3 * (size_t)d + q];
            xform(c, p, p);
#pragma unroll
            for (int q = 0; q < 3; ++q) dirs[3 * (size_t)d + q] = p[q];
        }
    }
}

// ---- the envelope: first column of every row, offsets, reach --------------------------------------------------------------
struct Envelope {
    std::vector<int64_t> off;     // N + 1
    std::vector<int32_t> cs, reach;
    int32_t bw = 0;               // max over rows of r - cs[r]
};
Envelope envelope_from(const std::vector<int32_t>& cs)
{
    Envelope E;
    const int32_t N = (int32_t)cs.size();
    E.cs = cs;
    E.off.assign(N + 1, 0);
    E.reach.assign(N, 0);
    for (int32_t r = 0; r < N; ++r) {
        E.off[r + 1] = E.off[r] + (r - cs[r] + 1);
        E.bw = std::max(E.bw, r - cs[r]);
    }
    // reach[k] = max { r : cs[r] <= k } (>= k)
    int32_t run = -1;
    std::vector<int32_t> best(N, -1);
    for (int32_t r = 0; r < N; ++r) best[cs[r]] = std::max(best[cs[r]], r);
    for (int32_t k = 0; k < N; ++k) { run = std::max(run, std::max(best[k], k)); E.reach[k] = run; }
    return E;
}

struct EnvDev { const int64_t* off; const int32_t* cs; const int32_t* reach; int32_t N, bw; };

// one damped envelope solve: L D L^T of H + lambda I and x with it; nbad: the count of zero / non-finite pivots
int env_solve_enqueue(const EnvDev& E, const double* H, double lambda, const double* b, double* Lo, double* z, double* zg,
                      double* x, int32_t* nbad, hipStream_t s)
{
    if (E.bw <= ENV_MAXBW_WIN) {
        hipLaunchKernelGGL(k_env_factor<true>, dim3(1), dim3(256), 0, s, H, E.off, E.cs, E.reach, E.N, lambda, b, Lo, z, zg, nbad);
        hipLaunchKernelGGL(k_env_backward<true>, dim3(1), dim3(256), 0, s, (const double*)Lo, E.off, E.cs, E.N, (const double*)z,
                           zg, x);
    } else {
        hipLaunchKernelGGL(k_env_factor<false>, dim3(1), dim3(256), 0, s, H, E.off, E.cs, E.reach, E.N, lambda, b, Lo, z, zg, nbad);
        hipLaunchKernelGGL(k_env_backward<false>, dim3(1), dim3(256), 0, s, (const double*)Lo, E.off, E.cs, E.N, (const double*)z,
                           zg, x);
    }
    PLSLAM_HIP_CHECK(hipGetLastError());
    return PLSLAM_OK;
}


}  // namespace
}  // namespace plslam

using namespace plslam;

struct plslam_pgo_plan {
    plslam_ctx* ctx = nullptr;
    plslam_pgo_params prm{};
    int32_t n_map = 0, kf_curr = 0, n_lc = 0, nv = 0, ne = 0, ne_lc = 0, na = 0, N = 0, nlvl = 0, ntarget = 0, bw = 0;
    int64_t env_entries = 0, npad = 0;
    bool dense = false;                       // the tool-only dense comparison path (context option "pgo_solver" = 1)
    std::vector<int32_t> vslot;               // vertex -> map slot (kf_list)
    std::vector<uint8_t> valid;
    std::vector<int32_t> lc_idx;
    DevBuf stat, work, Sbuf;
    size_t oEv = 0, oElc = 0, oVinit = 0, oLcIdx = 0, oTree = 0, oLvl = 0, oTg = 0, oContrib = 0, oRptr = 0, oRlist = 0, oOff = 0,
           oCs = 0, oReach = 0, oVcol = 0, oVslot = 0, oValid = 0;
    size_t oT = 0, oXin = 0, oLcp = 0, oZ = 0, oX0 = 0, oXa = 0, oXb = 0, oErr = 0, oJ = 0, oChi2 = 0, oH = 0, oB = 0, oL = 0,
           oZv = 0, oZg = 0, oDx = 0, oBad = 0, oStats = 0, oTout = 0, oXout = 0, oTcorr = 0, oCorr = 0, oP = 0, oW = 0, oBadp = 0;
};

namespace {

int pgo_fail(plslam_pgo_plan* P, int rc)
{
    P->stat.release(); P->work.release(); P->Sbuf.release();
    delete P;
    return rc;
}

// one trial: factor and solve (H + lambda I) dx = b, X' = X fromVectorMQT(dx), chi' and dx.(lambda dx + b)
int pgo_trial_enqueue(plslam_pgo_plan* P, double lambda, const double* X, double* Y, hipStream_t s)
{
    char* d = P->stat.as<char>();
    char* w = P->work.as<char>();
    auto Dd = [&](size_t o) { return (double*)(w + o); };
    const EnvDev E{(const int64_t*)(d + P->oOff), (const int32_t*)(d + P->oCs), (const int32_t*)(d + P->oReach), P->N, P->bw};
    int32_t* nbad = (int32_t*)(w + P->oBad);
    int rc;
    if (!P->dense) {
        if ((rc = env_solve_enqueue(E, Dd(P->oH), lambda, Dd(P->oB), Dd(P->oL), Dd(P->oZv), Dd(P->oZg), Dd(P->oDx), nbad, s)))
            return rc;
    } else {
        double* S = P->Sbuf.as<double>();
        PLSLAM_HIP_CHECK(hipMemsetAsync(S, 0, (size_t)P->npad * (size_t)P->npad * 8, s));
        PLSLAM_HIP_CHECK(hipMemsetAsync(Dd(P->oW), 0, (size_t)P->npad * 8, s));
        hipLaunchKernelGGL(k_env_to_dense, dim3((unsigned)P->npad), dim3(256), 0, s, (const double*)Dd(P->oH), E.off, E.cs, P->N,
                           P->npad, lambda, (const double*)Dd(P->oB), S, Dd(P->oW));
        if ((rc = ldlt_enqueue(S, P->npad, (int32_t)P->N, Dd(P->oP), Dd(P->oW), Dd(P->oZv), Dd(P->oDx), (int32_t*)(w + P->oBadp), s))) return rc;
        hipLaunchKernelGGL(k_count_bad, dim3(1), dim3(64), 0, s, (const int32_t*)(w + P->oBadp), (int32_t)(P->npad / LT), nbad);
    }
    hipLaunchKernelGGL(k_pgo_update, dim3((P->nv + 255) / 256), dim3(256), 0, s, (const int32_t*)(d + P->oVcol), P->nv,
                       (const double*)Dd(P->oDx), (const int32_t*)nbad, X, Y);
    hipLaunchKernelGGL(k_pgo_edges<false>, dim3((P->ne + 255) / 256), dim3(256), 0, s, (const int2*)(d + P->oEv), P->ne,
                       (const double*)Dd(P->oZ), (const double*)Y, Dd(P->oErr), Dd(P->oJ), Dd(P->oChi2));
    hipLaunchKernelGGL(k_pgo_reduce, dim3(1), dim3(256), 0, s, (const double*)Dd(P->oChi2), P->ne, (const double*)Dd(P->oDx),
                       (const double*)Dd(P->oB), P->N, lambda, (const int32_t*)nbad, (PgoStats*)(w + P->oStats));
    PLSLAM_HIP_CHECK(hipGetLastError());
    return PLSLAM_OK;
}

// the linearisation at X: errors, Jacobians, chi, H blocks, b
int pgo_linearise_enqueue(plslam_pgo_plan* P, const double* X, hipStream_t s)
{
    char* d = P->stat.as<char>();
    char* w = P->work.as<char>();
    auto Dd = [&](size_t o) { return (double*)(w + o); };
    hipLaunchKernelGGL(k_pgo_edges<true>, dim3((P->ne + 255) / 256), dim3(256), 0, s, (const int2*)(d + P->oEv), P->ne,
                       (const double*)Dd(P->oZ), X, Dd(P->oErr), Dd(P->oJ), Dd(P->oChi2));
    hipLaunchKernelGGL(k_pgo_reduce, dim3(1), dim3(256), 0, s, (const double*)Dd(P->oChi2), P->ne, (const double*)nullptr,
                       (const double*)nullptr, 0, 0.0, (const int32_t*)nullptr, (PgoStats*)(w + P->oStats) + 1);
    if (P->ntarget)
        hipLaunchKernelGGL(k_pgo_hblocks, dim3(P->ntarget), dim3(64), 0, s, (const PgoTarget*)(d + P->oTg),
                           (const int32_t*)(d + P->oContrib), (const double*)Dd(P->oJ), (const int64_t*)(d + P->oOff),
                           (const int32_t*)(d + P->oCs), Dd(P->oH));
    hipLaunchKernelGGL(k_pgo_rhs, dim3((6 * P->na + 255) / 256), dim3(256), 0, s, (const int32_t*)(d + P->oRptr),
                       (const int32_t*)(d + P->oRlist), P->na, (const double*)Dd(P->oJ), (const double*)Dd(P->oErr), Dd(P->oB));
    PLSLAM_HIP_CHECK(hipGetLastError());
    return PLSLAM_OK;
}

// reverse Cuthill-McKee over the active vertices (adjacency without duplicates): every component from a vertex of least
// degree (lowest index on ties), neighbours by ascending degree (then index); the whole order reversed
std::vector<int32_t> rcm_order(const std::vector<std::vector<int32_t>>& adj)
{
    const int32_t n = (int32_t)adj.size();
    std::vector<int32_t> order, deg(n);
    for (int32_t i = 0; i < n; ++i) deg[i] = (int32_t)adj[i].size();
    std::vector<char> seen(n, 0);
    std::vector<int32_t> byd(n);
    std::iota(byd.begin(), byd.end(), 0);
    std::stable_sort(byd.begin(), byd.end(), [&](int32_t a, int32_t b) { return deg[a] < deg[b]; });
    for (int32_t s0 : byd) {
        if (seen[s0]) continue;
        seen[s0] = 1;
        size_t h = order.size();
        order.push_back(s0);
        while (h < order.size()) {
            const int32_t u = order[h++];
            std::vector<int32_t> nb;
            for (int32_t v : adj[u]) if (!seen[v]) { seen[v] = 1; nb.push_back(v); }
            std::stable_sort(nb.begin(), nb.end(), [&](int32_t a, int32_t b) { return deg[a] != deg[b] ? deg[a] < deg[b] : a < b; });
            order.insert(order.end(), nb.begin(), nb.end());
        }
    }
    std::reverse(order.begin(), order.end());
    return order;
}

}  // namespace

extern "C" {

int plslam_pgo_plan_create(plslam_ctx* ctx, const plslam_pgo_params* params, int32_t n_map_kf, const uint8_t* kf_valid,
                           const int32_t* full_graph, int32_t n_lc, const int32_t* lc_idx, plslam_pgo_plan** out)
{
    PLSLAM_REQUIRE(ctx && params && out && n_map_kf >= 1 && kf_valid && full_graph && lc_idx, PLSLAM_EINVAL);
    *out = nullptr;
    PLSLAM_REQUIRE(n_lc >= 1 && params->max_iters_pgo >= 0 && params->max_trials >= 1, PLSLAM_EINVAL);
    PLSLAM_REQUIRE(kf_valid[0], PLSLAM_EINVAL);
    for (int32_t k = 0; k < n_lc; ++k) {
        const int32_t a = lc_idx[3 * k], b = lc_idx[3 * k + 1];
        PLSLAM_REQUIRE(a >= 0 && a < n_map_kf && b >= 0 && b < n_map_kf && kf_valid[a] && kf_valid[b] && a != b, PLSLAM_EINVAL);
    }
    int32_t kf_curr = -1;
    for (int32_t k = 0; k < n_lc; ++k) kf_curr = std::max(kf_curr, lc_idx[3 * k + 1]);
    // vertices: every non-NULL keyframe 0 .. kf_curr (:4210-4249)
    std::vector<int32_t> vslot, vof(n_map_kf, -1);
    for (int32_t i = 0; i <= kf_curr; ++i) if (kf_valid[i]) { vof[i] = (int32_t)vslot.size(); vslot.push_back(i); }
    const int32_t nv = (int32_t)vslot.size();
    // edges in creation order (:4252-4290): covisibility i ascending, j > i ascending, then one per LC entry
    std::vector<int2> ev;
    std::vector<int32_t> elc;
    const int64_t nm = n_map_kf;
    for (int32_t i = 0; i <= kf_curr; ++i) {
        if (!kf_valid[i]) continue;
        for (int32_t j = i + 1; j <= kf_curr; ++j) {
            const int32_t c = full_graph[(int64_t)i * nm + j];
            if (kf_valid[j] && (c >= params->min_lm_ess_graph || c >= params->min_lm_cov_graph || j - i == 1)) {
                ev.push_back(make_int2(vof[i], vof[j]));
                elc.push_back(-1);
            }
        }
    }
    for (int32_t k = 0; k < n_lc; ++k) { ev.push_back(make_int2(vof[lc_idx[3 * k]], vof[lc_idx[3 * k + 1]])); elc.push_back(k); }
    const int32_t ne = (int32_t)ev.size();
    // incident edges per vertex in creation order; active vertices: not vertex 0, at least one edge
    std::vector<std::vector<int32_t>> inc(nv);
    for (int32_t e = 0; e < ne; ++e) { inc[ev[e].x].push_back(e); inc[ev[e].y].push_back(e); }
    std::vector<int32_t> act;
    for (int32_t v = 1; v < nv; ++v) if (!inc[v].empty()) act.push_back(v);
    PLSLAM_REQUIRE(!act.empty(), PLSLAM_EINVAL);
    PLSLAM_REQUIRE((int64_t)act.size() <= PLSLAM_GBA_MAX_KEYFRAMES, PLSLAM_ERANGE);
    // computeInitialGuess's BFS tree from vertex 0 (slot 0 is vertex 0), by levels
    std::vector<int32_t> level(nv, -1);
    std::vector<PgoLevel> tree;
    std::vector<int32_t> lvl_ptr{0};
    {
        std::vector<int32_t> q{0};
        level[0] = 0;
        std::vector<std::vector<PgoLevel>> bylvl;
        for (size_t h = 0; h < q.size(); ++h) {
            const int32_t u = q[h];
            for (int32_t e : inc[u]) {
                const int32_t z = ev[e].x == u ? ev[e].y : ev[e].x;
                if (level[z] >= 0) continue;
                level[z] = level[u] + 1;
                if ((int32_t)bylvl.size() < level[z]) bylvl.resize(level[z]);
                bylvl[level[z] - 1].push_back({z, u, e, ev[e].x == u ? 1 : 0});
                q.push_back(z);
            }
        }
        for (auto& L : bylvl) { tree.insert(tree.end(), L.begin(), L.end()); lvl_ptr.push_back((int32_t)tree.size()); }
    }
    for (int32_t v : act) PLSLAM_REQUIRE(level[v] >= 0, PLSLAM_EINVAL);   // no path to vertex 0: a singular system
    // the reordered system
    const int32_t na = (int32_t)act.size();
    std::vector<int32_t> aof(nv, -1);
    for (int32_t k = 0; k < na; ++k) aof[act[k]] = k;
    std::vector<std::vector<int32_t>> adj(na);
    for (int32_t e = 0; e < ne; ++e) {
        const int32_t a = aof[ev[e].x], b = aof[ev[e].y];
        if (a >= 0 && b >= 0) { adj[a].push_back(b); adj[b].push_back(a); }
    }
    for (auto& l : adj) { std::sort(l.begin(), l.end()); l.erase(std::unique(l.begin(), l.end()), l.end()); }
    const std::vector<int32_t> ord = rcm_order(adj);
    std::vector<int32_t> pos(na), vcol(nv, -1);
    for (int32_t p = 0; p < na; ++p) pos[ord[p]] = p;
    for (int32_t k = 0; k < na; ++k) vcol[act[k]] = pos[k];
    std::vector<int32_t> sblk(na);
    for (int32_t p = 0; p < na; ++p) {
        int32_t s = p;
        for (int32_t nb : adj[ord[p]]) s = std::min(s, pos[nb]);
        sblk[p] = s;
    }
    const int32_t N = 6 * na;
    std::vector<int32_t> cs(N);
    for (int32_t r = 0; r < N; ++r) cs[r] = 6 * sblk[r / 6];
    Envelope E = envelope_from(cs);
    // H targets: every diagonal block and every (row block > col block) pair an edge joins; contributions in edge order
    struct Ct { int64_t key; int32_t code; };
    std::vector<Ct> cts;
    std::vector<std::vector<int32_t>> rl(na);
    for (int32_t e = 0; e < ne; ++e) {
        const int32_t ci = vcol[ev[e].x], cj = vcol[ev[e].y];
        if (ci >= 0) { cts.push_back({(int64_t)ci * na + ci, 4 * e + 0}); rl[ci].push_back(2 * e + 0); }
        if (cj >= 0) { cts.push_back({(int64_t)cj * na + cj, 4 * e + 1}); rl[cj].push_back(2 * e + 1); }
        if (ci >= 0 && cj >= 0 && ci != cj) {
            if (ci > cj) cts.push_back({(int64_t)ci * na + cj, 4 * e + 2});
            else cts.push_back({(int64_t)cj * na + ci, 4 * e + 3});
        }
    }
    std::stable_sort(cts.begin(), cts.end(), [](const Ct& a, const Ct& b) { return a.key < b.key; });
    std::vector<PgoTarget> tg;
    std::vector<int32_t> contrib(cts.size());
    for (size_t i = 0; i < cts.size();) {
        size_t j = i;
        while (j < cts.size() && cts[j].key == cts[i].key) { contrib[j] = cts[j].code; ++j; }
        tg.push_back({(int32_t)(cts[i].key / na), (int32_t)(cts[i].key % na), (int32_t)i, (int32_t)j});
        i = j;
    }
    std::vector<int32_t> rptr(na + 1, 0), rlist;
    for (int32_t p = 0; p < na; ++p) { rlist.insert(rlist.end(), rl[p].begin(), rl[p].end()); rptr[p + 1] = (int32_t)rlist.size(); }
    // vertex init: the LC entry whose (1)-end the vertex is, unless an earlier entry names it as (0) (:4220-4231, break)
    std::vector<int2> vinit(nv);
    for (int32_t v = 0; v < nv; ++v) {
        int32_t id = -1;
        for (int32_t k = 0; k < n_lc; ++k) {
            if (lc_idx[3 * k] == vslot[v]) break;
            if (lc_idx[3 * k + 1] == vslot[v]) { id = k; break; }
        }
        vinit[v] = make_int2(vslot[v], id);
    }

    plslam_pgo_plan* P = new (std::nothrow) plslam_pgo_plan();
    PLSLAM_REQUIRE(P != nullptr, PLSLAM_ENOMEM);
    P->ctx = ctx; P->prm = *params; P->n_map = n_map_kf; P->kf_curr = kf_curr; P->n_lc = n_lc; P->nv = nv; P->ne = ne;
    P->ne_lc = n_lc; P->na = na; P->N = N; P->nlvl = (int32_t)lvl_ptr.size() - 1; P->ntarget = (int32_t)tg.size(); P->bw = E.bw;
    P->env_entries = E.off[N]; P->dense = ctx->pgo_solver == 1; P->npad = pad_to_tile(N);
    P->vslot = vslot;
    P->valid.assign(kf_valid, kf_valid + n_map_kf);
    P->lc_idx.assign(lc_idx, lc_idx + 3 * (size_t)n_lc);
    Carver cs_;
    P->oEv = cs_.take((size_t)ne * 8); P->oElc = cs_.take((size_t)ne * 4); P->oVinit = cs_.take((size_t)nv * 8);
    P->oLcIdx = cs_.take((size_t)n_lc * 12); P->oTree = cs_.take(tree.size() * sizeof(PgoLevel) + 16);
    P->oLvl = cs_.take(lvl_ptr.size() * 4); P->oTg = cs_.take(tg.size() * sizeof(PgoTarget) + 16);
    P->oContrib = cs_.take(contrib.size() * 4 + 4); P->oRptr = cs_.take(rptr.size() * 4); P->oRlist = cs_.take(rlist.size() * 4 + 4);
    P->oOff = cs_.take(E.off.size() * 8); P->oCs = cs_.take((size_t)N * 4); P->oReach = cs_.take((size_t)N * 4);
    P->oVcol = cs_.take((size_t)nv * 4); P->oVslot = cs_.take((size_t)nv * 4); P->oValid = cs_.take((size_t)n_map_kf + 8);
    Carver cw;
    const size_t nmz = (size_t)n_map_kf;
    P->oT = cw.take(nmz * 128); P->oXin = cw.take(nmz * 48); P->oLcp = cw.take((size_t)n_lc * 48);
    P->oZ = cw.take((size_t)ne * 96); P->oX0 = cw.take((size_t)nv * 96); P->oXa = cw.take((size_t)nv * 96);
    P->oXb = cw.take((size_t)nv * 96); P->oErr = cw.take((size_t)ne * 48); P->oJ = cw.take((size_t)ne * 576);
    P->oChi2 = cw.take((size_t)ne * 8); P->oH = cw.take((size_t)E.off[N] * 8); P->oB = cw.take((size_t)N * 8);
    P->oL = cw.take((size_t)E.off[N] * 8); P->oZv = cw.take((size_t)P->npad * 8); P->oZg = cw.take((size_t)N * 8);
    P->oDx = cw.take((size_t)P->npad * 8); P->oBad = cw.take(8); P->oStats = cw.take(2 * sizeof(PgoStats));
    P->oTout = cw.take(nmz * 128); P->oXout = cw.take(nmz * 48); P->oTcorr = cw.take(nmz * 128); P->oCorr = cw.take(nmz + 8);
    if (P->dense) {
        P->oP = cw.take((size_t)P->npad * LT * 8); P->oW = cw.take((size_t)P->npad * 8);
        P->oBadp = cw.take((size_t)(P->npad / LT) * 4 + 4);
    }
    int rc;
    if ((rc = P->stat.reserve(cs_.off + 256)) || (rc = P->work.reserve(cw.off + 256)) ||
        (P->dense && (rc = P->Sbuf.reserve((size_t)P->npad * (size_t)P->npad * 8))))
        return pgo_fail(P, rc);
    {
        std::lock_guard<std::mutex> lk(ctx->mu);
        DeviceGuard dg_(ctx->device);
        hipStream_t s = ctx->stream;
        char* d = P->stat.as<char>();
        auto up = [&](size_t o, const void* src, size_t bytes) -> int {
            if (bytes) PLSLAM_HIP_CHECK(hipMemcpyAsync(d + o, src, bytes, hipMemcpyHostToDevice, s));
            return PLSLAM_OK;
        };
        if ((rc = up(P->oEv, ev.data(), ev.size() * 8)) || (rc = up(P->oElc, elc.data(), elc.size() * 4)) ||
            (rc = up(P->oVinit, vinit.data(), vinit.size() * 8)) || (rc = up(P->oLcIdx, lc_idx, (size_t)n_lc * 12)) ||
            (rc = up(P->oTree, tree.data(), tree.size() * sizeof(PgoLevel))) || (rc = up(P->oLvl, lvl_ptr.data(), lvl_ptr.size() * 4)) ||
            (rc = up(P->oTg, tg.data(), tg.size() * sizeof(PgoTarget))) || (rc = up(P->oContrib, contrib.data(), contrib.size() * 4)) ||
            (rc = up(P->oRptr, rptr.data(), rptr.size() * 4)) || (rc = up(P->oRlist, rlist.data(), rlist.size() * 4)) ||
            (rc = up(P->oOff, E.off.data(), E.off.size() * 8)) || (rc = up(P->oCs, E.cs.data(), (size_t)N * 4)) ||
            (rc = up(P->oReach, E.reach.data(), (size_t)N * 4)) || (rc = up(P->oVcol, vcol.data(), vcol.size() * 4)) ||
            (rc = up(P->oVslot, vslot.data(), vslot.size() * 4)) || (rc = up(P->oValid, kf_valid, nmz))) {
            (void)hipStreamSynchronize(s);
            return pgo_fail(P, rc);
        }
        if (hipStreamSynchronize(s) != hipSuccess) return pgo_fail(P, PLSLAM_EHIP);
    }
    *out = P;
    return PLSLAM_OK;
}

int plslam_pgo_optimize(plslam_pgo_plan* P, const double* T_kf_w, const double* x_kf_w, const double* lc_pose, double* T_out,
                        double* x_out, double* T_corr, uint8_t* corrected, plslam_pgo_trial* trace, int32_t trace_cap,
                        plslam_pgo_result* result)
{
    PLSLAM_REQUIRE(P && T_kf_w && x_kf_w && lc_pose && T_out && x_out && T_corr && corrected && trace_cap >= 0 &&
                   (trace_cap == 0 || trace), PLSLAM_EINVAL);
    plslam_ctx* ctx = P->ctx;
    std::lock_guard<std::mutex> lk(ctx->mu);
    DeviceGuard dg_(ctx->device);
    hipStream_t s = ctx->stream;
    StreamSyncOnError guard(s);
    char* d = P->stat.as<char>();
    char* w = P->work.as<char>();
    auto Dd = [&](size_t o) { return (double*)(w + o); };
    const size_t nm = (size_t)P->n_map;
    PLSLAM_HIP_CHECK(hipMemcpyAsync(w + P->oT, T_kf_w, nm * 128, hipMemcpyHostToDevice, s));
    PLSLAM_HIP_CHECK(hipMemcpyAsync(w + P->oXin, x_kf_w, nm * 48, hipMemcpyHostToDevice, s));
    PLSLAM_HIP_CHECK(hipMemcpyAsync(w + P->oLcp, lc_pose, (size_t)P->n_lc * 48, hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(k_pgo_meas, dim3((P->ne + 255) / 256), dim3(256), 0, s, (const int2*)(d + P->oEv),
                       (const int32_t*)(d + P->oElc), P->ne, (const int32_t*)(d + P->oVslot), (const double*)Dd(P->oT),
                       (const double*)Dd(P->oLcp), Dd(P->oZ));
    hipLaunchKernelGGL(k_pgo_init, dim3(1), dim3(256), 0, s, (const int2*)(d + P->oVinit), P->nv, (const double*)Dd(P->oT),
                       (const double*)Dd(P->oXin), (const int32_t*)(d + P->oLcIdx), (const double*)Dd(P->oLcp),
                       (const PgoLevel*)(d + P->oTree), (const int32_t*)(d + P->oLvl), P->nlvl, (const double*)Dd(P->oZ),
                       Dd(P->oX0), Dd(P->oXa));
    PLSLAM_HIP_CHECK(hipMemsetAsync(Dd(P->oH), 0, (size_t)P->env_entries * 8, s));
    PLSLAM_HIP_CHECK(hipGetLastError());
    double* Xs[2] = {Dd(P->oXa), Dd(P->oXb)};
    int cur = 0;
    PgoStats st[2];
    auto fetch = [&]() -> int {
        PLSLAM_HIP_CHECK(hipMemcpyAsync(st, w + P->oStats, sizeof(st), hipMemcpyDeviceToHost, s));
        PLSLAM_HIP_CHECK(hipStreamSynchronize(s));
        return PLSLAM_OK;
    };
    int rc;
    // chi of the initial guess
    hipLaunchKernelGGL(k_pgo_edges<false>, dim3((P->ne + 255) / 256), dim3(256), 0, s, (const int2*)(d + P->oEv), P->ne,
                       (const double*)Dd(P->oZ), (const double*)Xs[cur], Dd(P->oErr), Dd(P->oJ), Dd(P->oChi2));
    hipLaunchKernelGGL(k_pgo_reduce, dim3(1), dim3(256), 0, s, (const double*)Dd(P->oChi2), P->ne, (const double*)nullptr,
                       (const double*)nullptr, 0, 0.0, (const int32_t*)nullptr, (PgoStats*)(w + P->oStats) + 1);
    if ((rc = fetch())) return rc;
    const double chi_initial = st[1].chi;
    double lambda = P->prm.lambda_init, ni = 2.0;
    int32_t iters = 0, trials = 0, stop = PLSLAM_PGO_STOP_MAX_ITERS;
    for (int32_t it = 0; it < P->prm.max_iters_pgo; ++it) {
        if ((rc = pgo_linearise_enqueue(P, Xs[cur], s))) return rc;
        if (it == 0) { lambda = P->prm.lambda_init; ni = 2.0; }
        int32_t q = 0;
        double rho = 0.0;
        iters = it + 1;
        do {
            if ((rc = pgo_trial_enqueue(P, lambda, Xs[cur], Xs[cur ^ 1], s)) || (rc = fetch())) return rc;
            const double chi = st[1].chi;
            const bool ok = st[0].bad == 0;
            const double chi_new = ok ? st[0].chi : DBL_MAX;
            const double scale = st[0].scale + 1e-3;
            rho = (chi - chi_new) / scale;
            const double lam_used = lambda;
            const bool acc = rho > 0 && std::isfinite(chi_new);
            if (acc) {
                const double a = 1.0 - std::pow(2.0 * rho - 1.0, 3);
                lambda *= std::max(1.0 / 3.0, std::min(a, 2.0 / 3.0));
                ni = 2.0;
                cur ^= 1;
            } else {
                lambda *= ni;
                ni *= 2.0;
            }
            if (trials < trace_cap) {
                plslam_pgo_trial& t = trace[trials];
                t.iteration = it; t.trial = q; t.lambda = lam_used; t.chi = chi; t.chi_new = chi_new; t.scale = scale; t.rho = rho;
                t.ok = ok ? 1 : 0; t.accepted = acc ? 1 : 0;
            }
            ++trials;
            ++q;
        } while (rho < 0 && q < P->prm.max_trials);
        if (q == P->prm.max_trials || rho == 0) { stop = PLSLAM_PGO_STOP_TERMINATE; break; }
    }
    // chi of the final state, then the write-back (:4298-4304) and the keyframes after kf_curr (:4358-4362)
    hipLaunchKernelGGL(k_pgo_edges<false>, dim3((P->ne + 255) / 256), dim3(256), 0, s, (const int2*)(d + P->oEv), P->ne,
                       (const double*)Dd(P->oZ), (const double*)Xs[cur], Dd(P->oErr), Dd(P->oJ), Dd(P->oChi2));
    hipLaunchKernelGGL(k_pgo_reduce, dim3(1), dim3(256), 0, s, (const double*)Dd(P->oChi2), P->ne, (const double*)nullptr,
                       (const double*)nullptr, 0, 0.0, (const int32_t*)nullptr, (PgoStats*)(w + P->oStats) + 1);
    PLSLAM_HIP_CHECK(hipMemcpyAsync(w + P->oTout, T_kf_w, nm * 128, hipMemcpyHostToDevice, s));
    PLSLAM_HIP_CHECK(hipMemcpyAsync(w + P->oXout, x_kf_w, nm * 48, hipMemcpyHostToDevice, s));
    {
        std::vector<double> I(nm * 16, 0.0);
        for (size_t k = 0; k < nm; ++k) for (int a = 0; a < 4; ++a) I[16 * k + 5 * a] = 1.0;
        std::vector<uint8_t> cflag(nm, 0);
        for (int32_t v : P->vslot) cflag[v] = 1;
        PLSLAM_HIP_CHECK(hipMemcpyAsync(w + P->oTcorr, I.data(), nm * 128, hipMemcpyHostToDevice, s));
        PLSLAM_HIP_CHECK(hipMemcpyAsync(w + P->oCorr, cflag.data(), nm, hipMemcpyHostToDevice, s));
        hipLaunchKernelGGL(k_pgo_writeback, dim3((P->nv + 255) / 256), dim3(256), 0, s, (const int32_t*)(d + P->oVslot),
                           (const int32_t*)(d + P->oVcol), P->nv, (const double*)Xs[cur], (const double*)Dd(P->oX0),
                           (const double*)Dd(P->oT), Dd(P->oTout), Dd(P->oXout), Dd(P->oTcorr));
        const int32_t k0 = P->kf_curr + 1;
        if (k0 < P->n_map)
            hipLaunchKernelGGL(k_pgo_later, dim3((P->n_map - k0 + 255) / 256), dim3(256), 0, s, (const uint8_t*)(d + P->oValid), k0,
                               P->n_map, P->kf_curr, (const double*)Dd(P->oT), Dd(P->oTout), Dd(P->oXout), Dd(P->oTcorr),
                               (uint8_t*)(w + P->oCorr));
        PLSLAM_HIP_CHECK(hipGetLastError());
        PLSLAM_HIP_CHECK(hipMemcpyAsync(T_out, w + P->oTout, nm * 128, hipMemcpyDeviceToHost, s));
        PLSLAM_HIP_CHECK(hipMemcpyAsync(x_out, w + P->oXout, nm * 48, hipMemcpyDeviceToHost, s));
        PLSLAM_HIP_CHECK(hipMemcpyAsync(T_corr, w + P->oTcorr, nm * 128, hipMemcpyDeviceToHost, s));
        PLSLAM_HIP_CHECK(hipMemcpyAsync(corrected, w + P->oCorr, nm, hipMemcpyDeviceToHost, s));
        if ((rc = fetch())) return rc;
    }
    guard.dismiss();
    if (result) {
        result->iterations = iters; result->trials = trials; result->stop_reason = stop; result->n_vertices = P->nv;
        result->n_active = P->na; result->n_edges = P->ne; result->n_lc_edges = P->ne_lc; result->env_width = P->bw;
        result->env_entries = P->env_entries; result->chi_initial = chi_initial; result->chi_final = st[1].chi;
        result->lambda = lambda;
    }
    return PLSLAM_OK;
}

void plslam_pgo_plan_destroy(plslam_pgo_plan* P)
{
    if (!P) return;
    {
        std::lock_guard<std::mutex> lk(P->ctx->mu);
        DeviceGuard dg_(P->ctx->device);
        (void)hipStreamSynchronize(P->ctx->stream);
        P->stat.release(); P->work.release(); P->Sbuf.release();
    }
    delete P;
}

int plslam_envelope_ldlt_solve(plslam_ctx* ctx, int32_t n, const double* A, const double* b, double* x, int32_t* n_bad_pivots,
                               int32_t* env_width)
{
    PLSLAM_REQUIRE(ctx && n >= 1 && A && b && x && n <= 6 * PLSLAM_GBA_MAX_KEYFRAMES, PLSLAM_EINVAL);
    // the envelope of the lower triangle: the first nonzero column of every row
    std::vector<int32_t> cs(n);
    for (int32_t r = 0; r < n; ++r) {
        int32_t c = r;
        for (int32_t j = 0; j < r; ++j) if (A[(int64_t)r * n + j] != 0.0) { c = j; break; }
        cs[r] = c;
    }
    Envelope E = envelope_from(cs);
    std::vector<double> H((size_t)E.off[n]);
    for (int32_t r = 0; r < n; ++r)
        for (int32_t j = cs[r]; j <= r; ++j) H[E.off[r] + (j - cs[r])] = A[(int64_t)r * n + j];
    std::lock_guard<std::mutex> lk(ctx->mu);
    DeviceGuard dg_(ctx->device);
    hipStream_t s = ctx->stream;
    DevBuf buf;
    Carver c;
    const size_t ne = (size_t)E.off[n];
    const size_t oOff = c.take(((size_t)n + 1) * 8), oCs = c.take((size_t)n * 4), oRe = c.take((size_t)n * 4),
                 oH = c.take(ne * 8), oL = c.take(ne * 8), oB = c.take((size_t)n * 8), oZ = c.take((size_t)n * 8),
                 oZg = c.take((size_t)n * 8), oX = c.take((size_t)n * 8), oBad = c.take(8);
    int rc = buf.reserve(c.off);
    if (rc) return rc;
    ReleaseAfterSync rel{buf, s};
    char* d = buf.as<char>();
    PLSLAM_HIP_CHECK(hipMemcpyAsync(d + oOff, E.off.data(), ((size_t)n + 1) * 8, hipMemcpyHostToDevice, s));
    PLSLAM_HIP_CHECK(hipMemcpyAsync(d + oCs, E.cs.data(), (size_t)n * 4, hipMemcpyHostToDevice, s));
    PLSLAM_HIP_CHECK(hipMemcpyAsync(d + oRe, E.reach.data(), (size_t)n * 4, hipMemcpyHostToDevice, s));
    PLSLAM_HIP_CHECK(hipMemcpyAsync(d + oH, H.data(), ne * 8, hipMemcpyHostToDevice, s));
    PLSLAM_HIP_CHECK(hipMemcpyAsync(d + oB, b, (size_t)n * 8, hipMemcpyHostToDevice, s));
    const EnvDev ED{(const int64_t*)(d + oOff), (const int32_t*)(d + oCs), (const int32_t*)(d + oRe), n, E.bw};
    if ((rc = env_solve_enqueue(ED, (const double*)(d + oH), 0.0, (const double*)(d + oB), (double*)(d + oL), (double*)(d + oZ),
                                (double*)(d + oZg), (double*)(d + oX), (int32_t*)(d + oBad), s)))
        return rc;
    int32_t nb = 0;
    PLSLAM_HIP_CHECK(hipMemcpyAsync(x, d + oX, (size_t)n * 8, hipMemcpyDeviceToHost, s));
    PLSLAM_HIP_CHECK(hipMemcpyAsync(&nb, d + oBad, 4, hipMemcpyDeviceToHost, s));
    PLSLAM_HIP_CHECK(hipStreamSynchronize(s));
    if (n_bad_pivots) *n_bad_pivots = nb;
    if (env_width) *env_width = E.bw;
    return PLSLAM_OK;
}

}  // extern "C"

namespace {

// the map correction of one kind on stream s; scratch: 2 n + 1 + 2 n_anchor int32
int lc_correct_enqueue(int32_t n_map, const double* T_corr, const uint8_t* corrected, const plslam_lc_landmarks* L, int dl,
                       int32_t* scratch, hipStream_t s)
{
    if (!L || L->n == 0 || L->n_anchor == 0) return PLSLAM_OK;
    int32_t* cnt = scratch;
    int32_t* ptr = cnt + L->n;
    int32_t* eslot = ptr + L->n + 1;
    int32_t* list = eslot + L->n_anchor;
    PLSLAM_HIP_CHECK(hipMemsetAsync(cnt, 0, (size_t)L->n * 4, s));
    const unsigned ga = (unsigned)((L->n_anchor + 255) / 256), gl = (unsigned)((L->n + 255) / 256);
    hipLaunchKernelGGL(k_lc_count, dim3(ga), dim3(256), 0, s, L->anchor_ptr, n_map, L->anchor_idx, L->n_anchor, L->n, corrected,
                       eslot, cnt);
    hipLaunchKernelGGL(k_lc_scan, dim3(1), dim3(1024), 0, s, cnt, L->n, ptr);
    hipLaunchKernelGGL(k_lc_fill, dim3(ga), dim3(256), 0, s, L->anchor_idx, (const int32_t*)eslot, L->n_anchor,
                       (const int32_t*)ptr, cnt, list);
    if (dl == 3)
        hipLaunchKernelGGL(k_lc_apply<3>, dim3(gl), dim3(256), 0, s, (const int32_t*)ptr, list, (const int32_t*)eslot, L->valid,
                           L->n, T_corr, L->X, L->med_dir, L->dir_ptr, L->dirs);
    else
        hipLaunchKernelGGL(k_lc_apply<6>, dim3(gl), dim3(256), 0, s, (const int32_t*)ptr, list, (const int32_t*)eslot, L->valid,
                           L->n, T_corr, L->X, L->med_dir, L->dir_ptr, L->dirs);
    PLSLAM_HIP_CHECK(hipGetLastError());
    return PLSLAM_OK;
}

bool lm_ok(const plslam_lc_landmarks* L)
{
    return !L || L->n == 0 ||
           (L->n > 0 && L->n_anchor >= 0 && L->n_dir >= 0 && L->anchor_ptr && (L->n_anchor == 0 || L->anchor_idx) && L->valid &&
            L->X && L->med_dir && L->dir_ptr && (L->n_dir == 0 || L->dirs));
}

size_t scratch_ints(const plslam_lc_landmarks* L) { return L ? 2 * (size_t)L->n + 1 + 2 * (size_t)L->n_anchor : 0; }

}  // namespace

extern "C" {

int plslam_lc_correct_map_dev(plslam_ctx* ctx, int32_t n_map_kf, const double* T_corr, const uint8_t* corrected,
                              const plslam_lc_landmarks* points, const plslam_lc_landmarks* lines, void* stream)
{
    PLSLAM_REQUIRE(ctx && n_map_kf >= 1 && T_corr && corrected && lm_ok(points) && lm_ok(lines), PLSLAM_EINVAL);
    std::lock_guard<std::mutex> lk(ctx->mu);
    DeviceGuard dg_(ctx->device);
    hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
    const size_t need = std::max(scratch_ints(points), scratch_ints(lines)) * 4 + 256;
    // the scratch is the context's: whatever used it before on another stream is finished first
    PLSLAM_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    int rc = ctx->pgo_scratch.reserve(need);
    if (rc) return rc;
    StreamSyncOnError guard(s);
    int32_t* scr = ctx->pgo_scratch.as<int32_t>();
    if ((rc = lc_correct_enqueue(n_map_kf, T_corr, corrected, points, 3, scr, s))) return rc;
    if ((rc = lc_correct_enqueue(n_map_kf, T_corr, corrected, lines, 6, scr, s))) return rc;
    // the scratch is reused by the next call: the correction is finished when this returns
    PLSLAM_HIP_CHECK(hipStreamSynchronize(s));
    guard.dismiss();
    return PLSLAM_OK;
}

int plslam_lc_correct_map(plslam_ctx* ctx, int32_t n_map_kf, const double* T_corr, const uint8_t* corrected,
                          const plslam_lc_landmarks* points, const plslam_lc_landmarks* lines)
{
    PLSLAM_REQUIRE(ctx && n_map_kf >= 1 && T_corr && corrected && lm_ok(points) && lm_ok(lines), PLSLAM_EINVAL);
    // host arrays -> one device image, the _dev form on the context's stream, the landmarks back
    const plslam_lc_landmarks* kinds[2] = {points, lines};
    Carver c;
    const size_t oT = c.take((size_t)n_map_kf * 128), oC = c.take((size_t)n_map_kf + 8);
    size_t o[2][7] = {};
    for (int k = 0; k < 2; ++k) {
        const plslam_lc_landmarks* L = kinds[k];
        if (!L || L->n == 0) continue;
        const int dl = k ? 6 : 3;
        o[k][0] = c.take(((size_t)n_map_kf + 1) * 4); o[k][1] = c.take((size_t)L->n_anchor * 4 + 4);
        o[k][2] = c.take((size_t)L->n + 8); o[k][3] = c.take((size_t)L->n * dl * 8); o[k][4] = c.take((size_t)L->n * 24);
        o[k][5] = c.take(((size_t)L->n + 1) * 4); o[k][6] = c.take((size_t)L->n_dir * 24 + 8);
    }
    DevBuf buf;
    plslam_lc_landmarks dev[2] = {};
    {
        std::lock_guard<std::mutex> lk(ctx->mu);
        DeviceGuard dg_(ctx->device);
        hipStream_t s = ctx->stream;
        int rc = buf.reserve(c.off + 256);
        if (rc) return rc;
        char* d = buf.as<char>();
        StreamSyncOnError guard(s);
        PLSLAM_HIP_CHECK(hipMemcpyAsync(d + oT, T_corr, (size_t)n_map_kf * 128, hipMemcpyHostToDevice, s));
        PLSLAM_HIP_CHECK(hipMemcpyAsync(d + oC, corrected, (size_t)n_map_kf, hipMemcpyHostToDevice, s));
        for (int k = 0; k < 2; ++k) {
            const plslam_lc_landmarks* L = kinds[k];
            if (!L || L->n == 0) continue;
            const int dl = k ? 6 : 3;
            auto up = [&](size_t off, const void* src, size_t bytes) -> int {
                if (bytes) PLSLAM_HIP_CHECK(hipMemcpyAsync(d + off, src, bytes, hipMemcpyHostToDevice, s));
                return PLSLAM_OK;
            };
            if ((rc = up(o[k][0], L->anchor_ptr, ((size_t)n_map_kf + 1) * 4)) || (rc = up(o[k][1], L->anchor_idx, (size_t)L->n_anchor * 4)) ||
                (rc = up(o[k][2], L->valid, (size_t)L->n)) || (rc = up(o[k][3], L->X, (size_t)L->n * dl * 8)) ||
                (rc = up(o[k][4], L->med_dir, (size_t)L->n * 24)) || (rc = up(o[k][5], L->dir_ptr, ((size_t)L->n + 1) * 4)) ||
                (rc = up(o[k][6], L->dirs, (size_t)L->n_dir * 24)))
                return rc;
            dev[k] = *L;
            dev[k].anchor_ptr = (const int32_t*)(d + o[k][0]); dev[k].anchor_idx = (const int32_t*)(d + o[k][1]);
            dev[k].valid = (const uint8_t*)(d + o[k][2]); dev[k].X = (double*)(d + o[k][3]); dev[k].med_dir = (double*)(d + o[k][4]);
            dev[k].dir_ptr = (const int32_t*)(d + o[k][5]); dev[k].dirs = (double*)(d + o[k][6]);
        }
        PLSLAM_HIP_CHECK(hipStreamSynchronize(s));
        guard.dismiss();
    }
    int rc = plslam_lc_correct_map_dev(ctx, n_map_kf, (const double*)(buf.as<char>() + oT), (const uint8_t*)(buf.as<char>() + oC),
                                       points ? &dev[0] : nullptr, lines ? &dev[1] : nullptr, nullptr);
    std::lock_guard<std::mutex> lk(ctx->mu);
    DeviceGuard dg2_(ctx->device);
    hipStream_t s = ctx->stream;
    ReleaseAfterSync rel{buf, s};
    if (rc) return rc;
    for (int k = 0; k < 2; ++k) {
        const plslam_lc_landmarks* L = kinds[k];
        if (!L || L->n == 0) continue;
        const int dl = k ? 6 : 3;
        PLSLAM_HIP_CHECK(hipMemcpyAsync(L->X, dev[k].X, (size_t)L->n * dl * 8, hipMemcpyDeviceToHost, s));
        PLSLAM_HIP_CHECK(hipMemcpyAsync(L->med_dir, dev[k].med_dir, (size_t)L->n * 24, hipMemcpyDeviceToHost, s));
        if (L->n_dir) PLSLAM_HIP_CHECK(hipMemcpyAsync(L->dirs, dev[k].dirs, (size_t)L->n_dir * 24, hipMemcpyDeviceToHost, s));
    }
    PLSLAM_HIP_CHECK(hipStreamSynchronize(s));
    return PLSLAM_OK;
}

}  // extern "C"
