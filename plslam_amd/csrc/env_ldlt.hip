// env_ldlt.hip -- a general envelope (skyline) L D L^T solver in fp64, one workgroup: the linear solve of the loop-closure pose
// graph (pgo.hip, through env_ldlt.hpp) and, alone, plslam_envelope_ldlt_solve.
//   K45 k_env_factor<WIN>      one workgroup: L D L^T of (H + lambda I) over the envelope, right-looking, column by column,
//                              the forward solve fused (z = D^-1 L^-1 b); WIN: the active rows in a 128 x 128 LDS window
//   K46 k_env_backward<WIN>    one workgroup: L^T x = z, row by row, last first
// Every sum has a fixed order; phases are ordered by kernel boundaries and, inside a kernel, by workgroup barriers only.
#include <hip/hip_runtime.h>

#include <vector>

#include "env_ldlt.hpp"
#include "pgo_graph.hpp"

namespace plslam {
namespace {

constexpr int ENV_W = 128;      // rows / columns of the LDS window (128 x 128 doubles: 128 KiB)
constexpr int ENV_G = 16;       // rows loaded into the window at a time
constexpr int ENV_MAXBW_WIN = ENV_W - ENV_G;   // widest envelope (r - first column of row r) the window takes

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

}  // namespace

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

void env_to_dense_enqueue(const EnvDev& E, const double* H, int64_t npad, double lambda, const double* b, double* S, double* w,
                          hipStream_t s)
{
    hipLaunchKernelGGL(k_env_to_dense, dim3((unsigned)npad), dim3(256), 0, s, H, E.off, E.cs, E.N, npad, lambda, b, S, w);
}

}  // namespace plslam

using namespace plslam;

namespace {

struct EnvSolveView {
    Arr<int64_t> off;
    Arr<int32_t> cs, reach;
    Arr<double> H, L, b, z, zg, x;
    Arr<int32_t> nbad;
};

size_t carve_env_solve(EnvSolveView& v, size_t n, size_t entries, char* base)
{
    ArrCarver c{base};
    v.off = c.take<int64_t>((n + 1) * 8);
    v.cs = c.take<int32_t>(n * 4);
    v.reach = c.take<int32_t>(n * 4);
    v.H = c.take<double>(entries * 8);
    v.L = c.take<double>(entries * 8);
    v.b = c.take<double>(n * 8);
    v.z = c.take<double>(n * 8);
    v.zg = c.take<double>(n * 8);
    v.x = c.take<double>(n * 8);
    v.nbad = c.take<int32_t>(4, 4);
    return c.size();
}

}  // namespace

extern "C" int plslam_envelope_ldlt_solve(plslam_ctx* ctx, int32_t n, const double* A, const double* b, double* x, int32_t* n_bad_pivots,
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
    const Envelope E = envelope_from(cs);
    std::vector<double> H((size_t)E.off[n]);
    for (int32_t r = 0; r < n; ++r)
        for (int32_t j = cs[r]; j <= r; ++j) H[E.off[r] + (j - cs[r])] = A[(int64_t)r * n + j];
    std::lock_guard<std::mutex> lk(ctx->mu);
    DeviceGuard dg_(ctx->device);
    hipStream_t s = ctx->stream;
    DevBuf buf;
    EnvSolveView v;
    int rc = buf.reserve(carve_env_solve(v, (size_t)n, H.size(), nullptr));
    if (rc) return rc;
    ReleaseAfterSync rel{buf, s};
    carve_env_solve(v, (size_t)n, H.size(), buf.as<char>());
    const UploadItem ups[] = {{v.off, E.off.data()}, {v.cs, E.cs.data()}, {v.reach, E.reach.data()}, {v.H, H.data()}, {v.b, b}};
    if ((rc = upload_items(ups, s))) return rc;
    const EnvDev ED{v.off, v.cs, v.reach, n, E.bw};
    if ((rc = env_solve_enqueue(ED, v.H, 0.0, v.b, v.L, v.z, v.zg, v.x, v.nbad, s))) return rc;
    int32_t nb = 0;
    PLSLAM_HIP_CHECK(hipMemcpyAsync(x, v.x, (size_t)n * 8, hipMemcpyDeviceToHost, s));
    PLSLAM_HIP_CHECK(hipMemcpyAsync(&nb, v.nbad, 4, hipMemcpyDeviceToHost, s));
    PLSLAM_HIP_CHECK(hipStreamSynchronize(s));
    if (n_bad_pivots) *n_bad_pivots = nb;
    if (env_width) *env_width = E.bw;
    return PLSLAM_OK;
}
