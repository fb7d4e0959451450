// ldlt_dense_dev.hpp -- the dense right-looking fp64 L D L^T of the global bundle adjustment (K32-K36) and its enqueue
// function, shared by gba.hip and, as the comparison path of the loop-closure pose graph, pgo.hip.  Included INSIDE the
// includer's anonymous namespace in plslam, after it defines LT (the tile edge, 32) and dvec4_t (4 x double ext vector).
#pragma once

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

// ---- host side of the LDL^T: the matrix S (npad x npad, row-major, lower triangle read) is factored in place and
// S x = b solved; w, z: npad doubles of workspace (w holds b on entry and is overwritten); P: npad x 32 doubles; n <= npad: the
// order of the system itself, whose bad pivots badp counts per tile -------------------------------------------------------------
inline int64_t pad_to_tile(int64_t n) { return (n + LT - 1) / LT * LT; }   // the npad of ldlt_enqueue
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
