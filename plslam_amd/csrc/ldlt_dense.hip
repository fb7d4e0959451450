// ldlt_dense.hip -- the dense right-looking fp64 L D L^T of the global bundle adjustment (gba.hip) and, as the comparison path of
// the loop-closure pose graph, of pgo.hip; compiled once, used through ldlt_dense.hpp.
//   K32 k_ldlt_diag            one workgroup: L D L^T of the 32 x 32 diagonal tile (pivots that are zero / not finite counted)
//   K33 k_ldlt_panel           a workgroup per row tile below it: L_ik = A_ik L_kk^-T D^-1 (and X_ik = L_ik D kept)
//   K34 k_ldlt_update          a workgroup per lower tile of the trailing matrix: A_ij -= X_ik L_jk^T on v_mfma_f64_16x16x4_f64
//   K35 k_ldlt_fwd             per tile column: L y = b (+ the D scaling), the rows below updated in parallel
//   K36 k_ldlt_bwd             per tile row, last first: L^T x = z, the rows above updated in parallel
// and the two small kernels around a solve: the identity padding of S (k_pad_diag) and the sum of the per-tile counts of bad
// pivots (k_count_bad).  Every sum has a fixed shape; phases are ordered by kernel boundaries only.
#include <hip/hip_runtime.h>

#include "ldlt_dense.hpp"

namespace plslam {
namespace {

typedef double dvec4_t __attribute__((ext_vector_type(4)));

// ---- K32-K34: right-looking blocked L D L^T of the lower triangle, in place (strict lower: L, diagonal: D) --------------------
__global__ void __launch_bounds__(256)
k_ldlt_diag(double* __restrict__ S, int64_t ld, int32_t k, int32_t n, int32_t* __restrict__ badp)
{
    __shared__ double A[LT][LT + 1];
    __shared__ double col[LT];
    const int t = threadIdx.x;
    double* T0 = S + (int64_t)k * LT * ld + (int64_t)k * LT;
    for (int e = t; e < LT * LT; e += 256) {
        const int i = e / LT, c = e % LT;
        A[i][c] = c <= i ? T0[(int64_t)i * ld + c] : 0.0;     // the lower triangle only
    }
    int bad = 0;
    for (int j = 0; j < LT; ++j) {
        __syncthreads();
        const double d = A[j][j];
        // the pivots of the system only: the identity padding behind a bad pivot turns non-finite with it and is not counted
        if (t == 0 && k * LT + j < n && !(d != 0.0 && isfinite(d))) ++bad;
        if (t > j && t < LT) { const double l = A[t][j] / d; col[t] = l; A[t][j] = l; }
        __syncthreads();
        for (int e = t; e < LT * LT; e += 256) {
            const int i = e / LT, c = e % LT;
            if (c > j && i >= c) A[i][c] -= col[i] * (d * col[c]);
        }
    }
    __syncthreads();
    for (int e = t; e < LT * LT; e += 256) {
        const int i = e / LT, c = e % LT;
        if (c <= i) T0[(int64_t)i * ld + c] = A[i][c];
    }
    if (t == 0) badp[k] = bad;
}

// row tile i = k + 1 + blockIdx.x: X = A_ik L_kk^-T (forward over the columns), L_ik = X D^-1; X goes to the panel buffer
__global__ void __launch_bounds__(64)
k_ldlt_panel(double* __restrict__ S, int64_t ld, int32_t k, double* __restrict__ P)
{
    __shared__ double Lk[LT][LT + 1];
    const int r = threadIdx.x;
    const int64_t i0 = (int64_t)(k + 1 + blockIdx.x) * LT;
    const double* Tk = S + (int64_t)k * LT * ld + (int64_t)k * LT;
    for (int e = r; e < LT * LT; e += 64) Lk[e / LT][e % LT] = Tk[(int64_t)(e / LT) * ld + e % LT];
    __syncthreads();
    if (r >= LT) return;
    double* row = S + (i0 + r) * ld + (int64_t)k * LT;
    double x[LT];
#pragma unroll
    for (int c = 0; c < LT; ++c) x[c] = row[c];
#pragma unroll
    for (int j = 0; j < LT; ++j) {
        double s = x[j];
#pragma unroll
        for (int p = 0; p < j; ++p) s -= x[p] * Lk[j][p];
        x[j] = s;
    }
    double* prow = P + (i0 + r) * LT;
#pragma unroll
    for (int j = 0; j < LT; ++j) {
        prow[j] = x[j];
        row[j] = x[j] / Lk[j][j];
    }
}

// lower tile (i, j), k < j <= i: A_ij -= X_ik L_jk^T.  Four waves, one 16 x 16 quadrant each, eight MFMA steps of k = 4.
// v_mfma_f64_16x16x4_f64: A[row lane&15][k lane>>4], B[k lane>>4][col lane&15], D[row (lane>>4) + 4 q][col lane&15].
__global__ void __launch_bounds__(256)
k_ldlt_update(double* __restrict__ S, int64_t ld, int32_t k, const double* __restrict__ P)
{
    const int ti = blockIdx.y, tj = blockIdx.x;
    if (tj > ti) return;
    __shared__ double Xs[LT][LT + 1], Ls[LT][LT + 1];
    const int64_t i0 = (int64_t)(k + 1 + ti) * LT, j0 = (int64_t)(k + 1 + tj) * LT;
    const int t = threadIdx.x;
    for (int e = t; e < LT * LT; e += 256) {
        const int r = e / LT, c = e % LT;
        Xs[r][c] = P[(i0 + r) * LT + c];
        Ls[r][c] = S[(j0 + r) * ld + (int64_t)k * LT + c];
    }
    __syncthreads();
    const int w = t >> 6, lane = t & 63;
    const int r0 = (w >> 1) * 16, c0 = (w & 1) * 16;
    dvec4_t acc = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int s = 0; s < LT / 4; ++s) {
        const double a = Xs[r0 + (lane & 15)][4 * s + (lane >> 4)];
        const double b = Ls[c0 + (lane & 15)][4 * s + (lane >> 4)];
        acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc, 0, 0, 0);
    }
    double* C = S + (i0 + r0) * ld + j0 + c0 + (lane & 15);
#pragma unroll
    for (int q = 0; q < 4; ++q) C[(int64_t)((lane >> 4) + 4 * q) * ld] -= acc[q];
}

// ---- K35 / K36: the triangular solves.  Launch k of the forward solve: every workgroup solves L_kk y_k = w_k (w_k is final:
// only tiles below k change in this launch); workgroup 0 writes z_k = y_k / d_k, workgroup t > 0 updates w_(k+t) -= L y_k. ------
__global__ void __launch_bounds__(64)
k_ldlt_fwd(const double* __restrict__ S, int64_t ld, int32_t k, double* __restrict__ w, double* __restrict__ z)
{
    __shared__ double Ls[LT][LT + 1];
    __shared__ double ys[LT];
    const int r = threadIdx.x;
    const int64_t k0 = (int64_t)k * LT;
    for (int e = r; e < LT * LT; e += 64) Ls[e / LT][e % LT] = S[(k0 + e / LT) * ld + k0 + e % LT];
    __syncthreads();
    double y = r < LT ? w[k0 + r] : 0.0;
    for (int j = 0; j < LT; ++j) {
        const double yj = __shfl(y, j);
        if (r > j && r < LT) y -= Ls[r][j] * yj;
    }
    if (r < LT) ys[r] = y;
    const int64_t i0 = (int64_t)(k + blockIdx.x) * LT;
    if (blockIdx.x == 0) {
        if (r < LT) z[k0 + r] = y / Ls[r][r];
        return;
    }
    __syncthreads();
    for (int e = r; e < LT * LT; e += 64) Ls[e / LT][e % LT] = S[(i0 + e / LT) * ld + k0 + e % LT];
    __syncthreads();
    if (r < LT) {
        double acc = 0.0;
        for (int c = 0; c < LT; ++c) acc += Ls[r][c] * ys[c];
        w[i0 + r] -= acc;
    }
}

// launch k of the backward solve (k descending): L_kk^T x_k = u_k; workgroup k writes x_k, workgroup j < k updates
// u_j -= L_kj^T x_k
__global__ void __launch_bounds__(64)
k_ldlt_bwd(const double* __restrict__ S, int64_t ld, int32_t k, double* __restrict__ u, double* __restrict__ x)
{
    __shared__ double Ls[LT][LT + 1];
    __shared__ double xs[LT];
    const int c = threadIdx.x;
    const int64_t k0 = (int64_t)k * LT;
    for (int e = c; e < LT * LT; e += 64) Ls[e / LT][e % LT] = S[(k0 + e / LT) * ld + k0 + e % LT];
    __syncthreads();
    double v = c < LT ? u[k0 + c] : 0.0;
    for (int r = LT - 1; r >= 0; --r) {
        const double xr = __shfl(v, r);
        if (c < r) v -= Ls[r][c] * xr;
    }
    if (c < LT) xs[c] = v;
    const int j = blockIdx.x;
    if (j == k) {
        if (c < LT) x[k0 + c] = v;
        return;
    }
    const int64_t j0 = (int64_t)j * LT;
    __syncthreads();
    for (int e = c; e < LT * LT; e += 64) Ls[e / LT][e % LT] = S[(k0 + e / LT) * ld + j0 + e % LT];
    __syncthreads();
    if (c < LT) {
        double acc = 0.0;
        for (int r = 0; r < LT; ++r) acc += Ls[r][c] * xs[r];
        u[j0 + c] -= acc;
    }
}

// the padding of the matrix beyond n: identity, so that every tile is full
__global__ void __launch_bounds__(256)
k_pad_diag(double* __restrict__ S, int64_t ld, int32_t n, int32_t npad)
{
    const int i = n + blockIdx.x * 256 + threadIdx.x;
    if (i < npad) S[(int64_t)i * ld + i] = 1.0;
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

}  // namespace

int ldlt_enqueue(double* S, int64_t npad, int32_t n, double* P, double* w, double* z, double* x, int32_t* badp, hipStream_t s)
{
    const int nt = (int)(npad / LT);
    for (int k = 0; k < nt; ++k) {
        hipLaunchKernelGGL(k_ldlt_diag, dim3(1), dim3(256), 0, s, S, npad, k, n, badp);
        const int T = nt - k - 1;
        if (T > 0) {
            hipLaunchKernelGGL(k_ldlt_panel, dim3(T), dim3(64), 0, s, S, npad, k, P);
            hipLaunchKernelGGL(k_ldlt_update, dim3(T, T), dim3(256), 0, s, S, npad, k, (const double*)P);
        }
    }
    for (int k = 0; k < nt; ++k) hipLaunchKernelGGL(k_ldlt_fwd, dim3(nt - k), dim3(64), 0, s, (const double*)S, npad, k, w, z);
    for (int k = nt - 1; k >= 0; --k) hipLaunchKernelGGL(k_ldlt_bwd, dim3(k + 1), dim3(64), 0, s, (const double*)S, npad, k, z, x);
    PLSLAM_HIP_CHECK(hipGetLastError());
    return PLSLAM_OK;
}

void ldlt_pad_diag_enqueue(double* S, int64_t npad, int32_t n, hipStream_t s)
{
    if (npad > n) hipLaunchKernelGGL(k_pad_diag, dim3(1), dim3(256), 0, s, S, npad, n, (int32_t)npad);
}

void ldlt_count_bad_enqueue(const int32_t* badp, int32_t nt, int32_t* nbad, hipStream_t s)
{
    hipLaunchKernelGGL(k_count_bad, dim3(1), dim3(64), 0, s, badp, nt, nbad);
}

}  // namespace plslam

using namespace plslam;

namespace {

struct DenseSolveView { Arr<double> S, P, w, z, x; Arr<int32_t> badp, nbad; };

size_t carve_dense_solve(DenseSolveView& v, int64_t npad, char* base)
{
    ArrCarver c{base};
    const size_t np8 = (size_t)npad * 8;
    v.S = c.take<double>((size_t)npad * np8);
    v.P = c.take<double>(np8 * LT);
    v.w = c.take<double>(np8);
    v.z = c.take<double>(np8);
    v.x = c.take<double>(np8);
    v.badp = c.take<int32_t>((size_t)(npad / LT) * 4);
    v.nbad = c.take<int32_t>(4);
    return c.size();
}

}  // namespace

extern "C" int plslam_dense_ldlt_solve(plslam_ctx* ctx, int32_t n, const double* A, const double* b, double* x, int32_t* n_bad_pivots)
{
    PLSLAM_REQUIRE(ctx && n >= 1 && A && b && x && n <= 6 * PLSLAM_GBA_MAX_KEYFRAMES, PLSLAM_EINVAL);
    const int64_t npad = pad_to_tile(n);
    std::lock_guard<std::mutex> lk(ctx->mu);
    DeviceGuard dg_(ctx->device);
    hipStream_t s = ctx->stream;
    DevBuf buf;
    DenseSolveView v;
    int rc = buf.reserve(carve_dense_solve(v, npad, nullptr));
    if (rc) return rc;
    ReleaseAfterSync rel{buf, s};
    carve_dense_solve(v, npad, buf.as<char>());
    PLSLAM_HIP_CHECK(hipMemsetAsync(v.S, 0, v.S.bytes, s));
    PLSLAM_HIP_CHECK(hipMemsetAsync(v.w, 0, v.w.bytes, s));
    PLSLAM_HIP_CHECK(hipMemcpy2DAsync(v.S, (size_t)npad * 8, A, (size_t)n * 8, (size_t)n * 8, n, hipMemcpyHostToDevice, s));
    PLSLAM_HIP_CHECK(hipMemcpyAsync(v.w, b, (size_t)n * 8, hipMemcpyHostToDevice, s));
    ldlt_pad_diag_enqueue(v.S, npad, n, s);
    if ((rc = ldlt_enqueue(v.S, npad, n, v.P, v.w, v.z, v.x, v.badp, s))) return rc;
    ldlt_count_bad_enqueue(v.badp, (int32_t)(npad / LT), v.nbad, s);
    PLSLAM_HIP_CHECK(hipGetLastError());
    int32_t nb = 0;
    PLSLAM_HIP_CHECK(hipMemcpyAsync(x, v.x, (size_t)n * 8, hipMemcpyDeviceToHost, s));
    PLSLAM_HIP_CHECK(hipMemcpyAsync(&nb, v.nbad, 4, hipMemcpyDeviceToHost, s));
    PLSLAM_HIP_CHECK(hipStreamSynchronize(s));
    if (n_bad_pivots) *n_bad_pivots = nb;
    return PLSLAM_OK;
}
