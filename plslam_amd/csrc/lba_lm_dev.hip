// lba_lm_dev.hip -- plslam_lba_plan_optimize_dev: the whole Levenberg-Marquardt loop of levMarquardtOptimizationLBA
// (src/mapHandler.cpp:1334-1812) on the device in one call, one synchronisation at its end.
//
// The loop's variables (lambda, err, err_prev, iters, the stop word, the apply flag of the current solve, the running counts of
// singular landmarks and bad pivots) live in a control block in device memory (LbaLmCtl, lba_lm_ctl.hpp: the decisions are that
// header's pure functions, run on one lane).  A pass = one H / g build with its solve and step.  EVERY kernel of a pass reads the
// stop word first and returns if it is set, so the host enqueues passes without waiting: a pass behind the stop changes nothing.
// Ordering comes from kernel boundaries on the plan's stream only -- no graph, no grid barrier, no spinning kernel.
//   first pass   rows + cross blocks | landmark blocks, keyframe chunk partials | keyframe blocks + err | K98 | landmark inverses |
//                Schur partials | S, b | K99 | back-substitution | K102                                              (10 launches)
//   later pass   rows + cross blocks | landmark blocks AND their damped inverses, keyframe chunk partials | Schur partials AND the
//                keyframe blocks + err | S, b | K99 | back-substitution | K102                                        (7 launches)
//   K98  k_lm_first      max |H(i,i)| -> lambda0 = lambda_lba_lm * Hmax into the control block (it never comes to the host)
//   K99  k_lm_solve      one workgroup: err and the :1775 test (lane 0) | S into LDS, L D L^T without pivoting, the two triangular
//                        solves, the count of pivots that are <= 0 or not finite | dp where the back-substitution reads it | the
//                        pose update and the estimate slots, a lane per keyframe (pose_step_dev.hpp), when the step is applied
//   K100 k_lm_pre / k_lm_pad   6 nkf > LM_SOLVE_MAX_N6: the :1775 test alone | S and b into the padded copy ldlt_enqueue works on
//   K101 k_lm_post       ... and behind ldlt_enqueue: the pivots of its factor counted, dp, the pose update
//   K102 k_lm_tail       the back-substitution's partial sums added in workgroup order, the lambda schedule, the :1808 test,
//                        err_prev, iters; the pass's trace record completed
//   K103 k_lm_final      x_kf, expmap(x_kf), the result record into the image; the Schur step's counters cleared for the next call
//   K104 k_lm_solve_host plslam_lba_reduced_ldlt_solve: K99's solve alone
// The one-workgroup solve keeps S in LDS with a row stride of n6 + 1 doubles: n6 <= LM_SOLVE_MAX_N6 = 120 (20 keyframes; 116 kB
// of the CU's 160 kB, the dynamic-LDS attribute raised per plan, on the plan's device).  Above it the call uses the blocked
// L D L^T of the global BA (ldlt_dense.hpp) on a padded copy.  fp64, -ffp-contract=off, every sum of a fixed shape: column j of
// the factor is scaled, then the trailing entries take their (L_ij L_cj) d_j in order of j; the forward solve subtracts in
// ascending, the backward solve in descending column order.  No atomics in here.
// The trace records, the result, x_kf and T land in the plan's page-locked image, which the kernels write in place where the device
// can address it; the host may look at the stop word there between two passes and stop enqueuing (context option
// "lba_loop_peek") -- an optimisation: nothing depends on when the word becomes visible.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "lba_plan.hpp"
#include "ldlt_dense.hpp"
#include "pose_step_dev.hpp"

using namespace plslam;

namespace plslam {

constexpr int LM_SOLVE_MAX_N6 = 120;
constexpr int LM_WG = 256;
static_assert(sizeof(plslam_lba_solve) == 48 && sizeof(plslam_lba_result) == 48, "the image's layout");

// what the loop writes for the host, in the page-locked image (mapped) or in its twin on the device: the peeked stop word, the
// result, the trace, x_kf, T
struct LmImage {
    int32_t* peek = nullptr;
    plslam_lba_result* result = nullptr;
    plslam_lba_solve* trace = nullptr;
    double *x = nullptr, *T = nullptr;
    static size_t bytes(size_t nkf, size_t ntr) { return 16 + sizeof(plslam_lba_result) + ntr * sizeof(plslam_lba_solve) + nkf * 22 * 8; }
    LmImage() = default;
    LmImage(char* base, size_t nkf, size_t ntr)
        : peek(reinterpret_cast<int32_t*>(base)), result(reinterpret_cast<plslam_lba_result*>(base + 16)),
          trace(reinterpret_cast<plslam_lba_solve*>(base + 16 + sizeof(plslam_lba_result))),
          x(reinterpret_cast<double*>(base + 16 + sizeof(plslam_lba_result) + ntr * sizeof(plslam_lba_solve))), T(x + 6 * nkf) {}
};
// the device block: the control block with x_kf behind it (ONE copy brings both up), the image's twin, the padded solve's scratch
struct LmDev {
    LbaLmCtl* ctl = nullptr;
    double* x = nullptr;
    char* img = nullptr;
    double *Spad = nullptr, *Ppan = nullptr, *w = nullptr, *z = nullptr, *xs = nullptr;
    int32_t* badp = nullptr;
};
constexpr size_t LM_CTL_BYTES = (sizeof(LbaLmCtl) + 15) / 16 * 16;
static size_t lm_carve(const plslam_lba_plan* P, size_t ntr, char* base, LmDev& d)
{
    ArrCarver c{base};
    const size_t nkf = (size_t)P->nkf, n6 = 6 * nkf;
    d.ctl = c.take<LbaLmCtl>(LM_CTL_BYTES + n6 * 8);
    d.x = reinterpret_cast<double*>(reinterpret_cast<char*>(d.ctl) + LM_CTL_BYTES);
    d.img = c.take<char>(LmImage::bytes(nkf, ntr));
    if (n6 > (size_t)LM_SOLVE_MAX_N6) {
        const size_t npad = (size_t)pad_to_tile((int64_t)n6);
        d.Spad = c.take<double>(npad * npad * 8);
        d.Ppan = c.take<double>(npad * LT * 8);
        d.w = c.take<double>(npad * 8);
        d.z = c.take<double>(npad * 8);
        d.xs = c.take<double>(npad * 8);
        d.badp = c.take<int32_t>(npad / LT * 4);
    }
    return c.size();
}

// ---- the solve on one workgroup -------------------------------------------------------------------------------------------------
// A: n x n in LDS, row stride ld, lower triangle read and factored in place (strict lower: L, diagonal: D); y: n, b on entry, the
// solution on return.  Returns the number of pivots that are <= 0 or not finite (the same on every lane).
__device__ __forceinline__ int lm_ldlt_solve_lds(double* __restrict__ A, int ld, int n, double* __restrict__ y)
{
    const int t = threadIdx.x, ty = t >> 4, tx = t & 15;
    int bad = 0;
    for (int j = 0; j < n; ++j) {
        const double d = A[j * ld + j];
        if (!(d > 0.0) || !isfinite(d)) ++bad;
        for (int i = j + 1 + t; i < n; i += LM_WG) A[i * ld + j] = A[i * ld + j] / d;
        __syncthreads();
        for (int i = j + 1 + ty; i < n; i += 16)
            for (int c = j + 1 + tx; c <= i; c += 16) A[i * ld + c] -= (A[i * ld + j] * A[c * ld + j]) * d;
        __syncthreads();
    }
    for (int k = 0; k < n; ++k) {                          // L y' = b: row i subtracts L_ik y'_k in ascending k
        const double yk = y[k];
        for (int i = k + 1 + t; i < n; i += LM_WG) y[i] -= A[i * ld + k] * yk;
        __syncthreads();
    }
    for (int i = t; i < n; i += LM_WG) y[i] = y[i] / A[i * ld + i];
    __syncthreads();
    for (int k = n - 1; k >= 0; --k) {                     // L^T x = y'': row i subtracts L_ki x_k in descending k
        const double xk = y[k];
        for (int i = t; i < k; i += LM_WG) y[i] -= A[k * ld + i] * xk;
        __syncthreads();
    }
    return bad;
}

// the pose update of an applied step, a lane per keyframe: x_k, and the estimate slot the next pass's point rows read
__device__ __forceinline__ void lm_pose_update(int nkf, const double* __restrict__ dp, double* __restrict__ x, double* __restrict__ Test)
{
    for (int k = threadIdx.x; k < nkf; k += LM_WG) {
        double d[6], xk[6], Tp[16];
#pragma unroll
        for (int a = 0; a < 6; ++a) { d[a] = dp[6 * k + a]; xk[a] = x[6 * k + a]; }
        pose_step_se3(d, xk, Tp);
#pragma unroll
        for (int a = 0; a < 6; ++a) x[6 * k + a] = xk[a];
#pragma unroll
        for (int i = 0; i < 16; ++i) Test[16 * (size_t)k + i] = Tp[i];
    }
}

// K98
__global__ void __launch_bounds__(LM_WG)
k_lm_first(const double* __restrict__ H_pose, int32_t nkf, const double* __restrict__ H_pt, int32_t npt, const double* __restrict__ H_ls,
           int32_t nls, LbaLmCtl* __restrict__ ctl, const LbaLmPrm prm)
{
    __shared__ double red[LM_WG];
    if (ctl->stop != LM_RUNNING) return;
    double m = 0.0;
    const int total = 6 * nkf + 3 * npt + 6 * nls;
    for (int i = threadIdx.x; i < total; i += LM_WG) {
        double v;
        if (i < 6 * nkf) v = H_pose[(size_t)(i / 6) * 36 + (i % 6) * 7];
        else if (i < 6 * nkf + 3 * npt) { const int q = i - 6 * nkf; v = H_pt[(size_t)(q / 3) * 9 + (q % 3) * 4]; }
        else { const int q = i - 6 * nkf - 3 * npt; v = H_ls[(size_t)(q / 6) * 36 + (q % 6) * 7]; }
        v = fabs(v);
        m = v > m ? v : m;                                 // (a maximum: exact whatever the order)
    }
    red[threadIdx.x] = m;
    __syncthreads();
    for (int s = LM_WG / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] = red[threadIdx.x] > red[threadIdx.x + s] ? red[threadIdx.x] : red[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        LbaLmCtl c = *ctl;
        lm_on_hmax(c, prm, red[0]);
        ctl->hmax = c.hmax;
        ctl->lambda = c.lambda;
    }
}

// lane 0 of a control kernel: err, the :1775 test, the pass's trace record opened.  -> the solve runs
__device__ __forceinline__ bool lm_open_pass(LbaLmCtl& c, const LbaLmPrm& prm, double err_raw, plslam_lba_solve* __restrict__ trace,
                                             int32_t* __restrict__ peek)
{
    const bool go = lm_on_err(c, prm, err_raw);
    plslam_lba_solve& r = trace[c.n_builds - 1];
    r.lambda = go ? c.lambda : 0.0;
    r.err_raw = c.err_raw;
    r.err = c.err;
    r.dx_norm = 0.0;
    r.n_singular = 0;
    r.n_bad_pivots = 0;
    r.applied = c.apply;
    r.reserved = 0;
    if (!go) *peek = 1;
    return go;
}
// ... and behind the solve: the pivots, the pose part of ||DX||^2 (dp's squares added in order)
__device__ __forceinline__ void lm_close_solve(LbaLmCtl& c, int n_bad, const double* __restrict__ dp, int n6,
                                               plslam_lba_solve* __restrict__ trace, int32_t* __restrict__ peek)
{
    lm_on_pivots(c, n_bad);
    double s2 = 0.0;
    for (int i = 0; i < n6; ++i) s2 += dp[i] * dp[i];
    c.dp_sumsq = s2;
    plslam_lba_solve& r = trace[c.n_builds - 1];
    r.n_bad_pivots = n_bad;
    r.applied = c.apply;
    if (c.stop != LM_RUNNING) *peek = 1;
}

struct LmSolveArgs {
    LbaLmCtl* ctl;
    LbaLmPrm prm;
    const double *S, *b, *err_src;         // where k_schur_finish leaves them on the device
    double *dp, *x, *Test;                 // where k_schur_backsub reads dp; x_kf; the first estimate slot
    plslam_lba_solve* trace;
    int32_t* peek;
    int32_t nkf;
};

// K99
__global__ void __launch_bounds__(LM_WG)
k_lm_solve(const LmSolveArgs a)
{
    extern __shared__ __attribute__((aligned(16))) double lm_lds[];
    __shared__ int32_t flag[2];
    const int n = 6 * a.nkf, ld = n + 1, t = threadIdx.x;
    double* A = lm_lds;
    double* y = lm_lds + (size_t)n * ld;
    LbaLmCtl c = *a.ctl;
    if (c.stop != LM_RUNNING) return;
    __syncthreads();                                       // (every lane has read the control block before lane 0 rewrites it)
    if (t == 0) {
        const bool go = lm_open_pass(c, a.prm, *a.err_src, a.trace, a.peek);
        if (!go) *a.ctl = c;
        flag[0] = go ? 1 : 0;
    }
    __syncthreads();
    if (!flag[0]) return;
    for (int e = t; e < n * n; e += LM_WG) { const int i = e / n, cc = e - i * n; A[i * ld + cc] = a.S[e]; }
    for (int i = t; i < n; i += LM_WG) y[i] = a.b[i];
    __syncthreads();
    const int bad = lm_ldlt_solve_lds(A, ld, n, y);
    for (int i = t; i < n; i += LM_WG) a.dp[i] = y[i];
    if (t == 0) {
        lm_close_solve(c, bad, y, n, a.trace, a.peek);
        *a.ctl = c;
        flag[1] = c.apply;
    }
    __syncthreads();
    if (flag[1] == 1) lm_pose_update(a.nkf, y, a.x, a.Test);
}

// K100: the padded route's control kernel, and the copy into the padded system (identity behind n6: every tile is full)
__global__ void __launch_bounds__(64)
k_lm_pre(const LmSolveArgs a)
{
    LbaLmCtl c = *a.ctl;
    if (c.stop != LM_RUNNING || threadIdx.x != 0) return;
    (void)lm_open_pass(c, a.prm, *a.err_src, a.trace, a.peek);
    *a.ctl = c;
}
__global__ void __launch_bounds__(LM_WG)
k_lm_pad(const LbaLmCtl* __restrict__ ctl, const double* __restrict__ S, const double* __restrict__ b, int32_t n, int32_t npad,
         double* __restrict__ Spad, double* __restrict__ w)
{
    if (ctl->stop != LM_RUNNING) return;
    const int i = blockIdx.x;
    for (int cc = threadIdx.x; cc < npad; cc += LM_WG)
        Spad[(size_t)i * npad + cc] = (i < n && cc < n) ? S[(size_t)i * n + cc] : (i == cc ? 1.0 : 0.0);
    if (threadIdx.x == 0) w[i] = i < n ? b[i] : 0.0;
}
// K101: behind ldlt_enqueue -- the factor's diagonal holds the pivots
__global__ void __launch_bounds__(LM_WG)
k_lm_post(const LmSolveArgs a, const double* __restrict__ Spad, int32_t npad, const double* __restrict__ xs)
{
    __shared__ int32_t red[LM_WG];
    __shared__ int32_t flag;
    const int n = 6 * a.nkf, t = threadIdx.x;
    LbaLmCtl c = *a.ctl;
    if (c.stop != LM_RUNNING) return;
    int bad = 0;
    for (int i = t; i < n; i += LM_WG) {
        const double d = Spad[(size_t)i * npad + i];
        if (!(d > 0.0) || !isfinite(d)) ++bad;
        a.dp[i] = xs[i];
    }
    red[t] = bad;
    __syncthreads();
    for (int s = LM_WG / 2; s > 0; s >>= 1) {
        if (t < s) red[t] += red[t + s];
        __syncthreads();
    }
    if (t == 0) {
        lm_close_solve(c, red[0], xs, n, a.trace, a.peek);
        *a.ctl = c;
        flag = c.apply;
    }
    __syncthreads();
    if (flag == 1) lm_pose_update(a.nkf, xs, a.x, a.Test);
}

// K102
__global__ void __launch_bounds__(64)
k_lm_tail(LbaLmCtl* __restrict__ ctl, const LbaLmPrm prm, const double* __restrict__ part, int32_t nwg, const int32_t* __restrict__ sing_cur,
          plslam_lba_solve* __restrict__ trace, int32_t* __restrict__ peek)
{
    LbaLmCtl c = *ctl;
    if (c.stop != LM_RUNNING || threadIdx.x != 0) return;
    double s2 = 0.0;                                       // one sum of squares per workgroup of the back-substitution, in their order
    for (int i0 = 0; i0 < nwg; i0 += 8) {
        double v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = part[i0 + u < nwg ? i0 + u : nwg - 1];
#pragma unroll
        for (int u = 0; u < 8; ++u) if (i0 + u < nwg) s2 += v[u];
    }
    const int32_t ns = *sing_cur;
    c.n_singular += ns;
    plslam_lba_solve& r = trace[c.n_builds - 1];
    r.dx_norm = sqrt(c.dp_sumsq + s2);
    r.n_singular = ns;
    lm_on_step(c, prm, s2);
    *ctl = c;
    if (c.stop != LM_RUNNING) *peek = 1;
}

// K103: not behind the stop word -- it reports how the loop ended
__global__ void __launch_bounds__(64)
k_lm_final(const LbaLmCtl* __restrict__ ctl, const double* __restrict__ x, int32_t nkf, plslam_lba_result* __restrict__ result,
           double* __restrict__ x_out, double* __restrict__ T_out, int32_t* __restrict__ sing2)
{
    const int k = blockIdx.x * 64 + threadIdx.x;
    if (k < nkf) {
        double xk[6], Tp[16];
#pragma unroll
        for (int a = 0; a < 6; ++a) { xk[a] = x[6 * (size_t)k + a]; x_out[6 * (size_t)k + a] = xk[a]; }
        expmap_se3(xk, Tp);
#pragma unroll
        for (int i = 0; i < 16; ++i) T_out[16 * (size_t)k + i] = Tp[i];
    }
    if (k == 0) {
        const LbaLmCtl c = *ctl;
        result->iters = c.iters;
        result->n_builds = c.n_builds;
        result->stop_reason = c.stop == LM_RUNNING ? PLSLAM_LBA_STOP_MAX_ITERS : c.stop;
        result->n_enqueued_passes = 0;                     // (the host's count)
        result->err = c.err;
        result->err_prev = c.err_prev;
        result->lambda = c.lambda;
        result->hmax = c.hmax;
        sing2[0] = 0;                                      // both counters of singular landmarks: passes behind the stop left them as they were
        sing2[1] = 0;
    }
}

// K104
__global__ void __launch_bounds__(LM_WG)
k_lm_solve_host(const double* __restrict__ S, const double* __restrict__ b, int32_t n, double* __restrict__ x, int32_t* __restrict__ nbad)
{
    extern __shared__ __attribute__((aligned(16))) double lm_lds[];
    const int ld = n + 1, t = threadIdx.x;
    double* A = lm_lds;
    double* y = lm_lds + (size_t)n * ld;
    for (int e = t; e < n * n; e += LM_WG) { const int i = e / n, cc = e - i * n; A[i * ld + cc] = S[e]; }
    for (int i = t; i < n; i += LM_WG) y[i] = b[i];
    __syncthreads();
    const int bad = lm_ldlt_solve_lds(A, ld, n, y);
    for (int i = t; i < n; i += LM_WG) x[i] = y[i];
    if (t == 0) *nbad = bad;
}
// the padded route of the same call: the pivots on the factor's diagonal
__global__ void __launch_bounds__(LM_WG)
k_lm_count_pivots(const double* __restrict__ Spad, int32_t n, int32_t npad, int32_t* __restrict__ nbad)
{
    __shared__ int32_t red[LM_WG];
    const int t = threadIdx.x;
    int bad = 0;
    for (int i = t; i < n; i += LM_WG) {
        const double d = Spad[(size_t)i * npad + i];
        if (!(d > 0.0) || !isfinite(d)) ++bad;
    }
    red[t] = bad;
    __syncthreads();
    for (int s = LM_WG / 2; s > 0; s >>= 1) {
        if (t < s) red[t] += red[t + s];
        __syncthreads();
    }
    if (t == 0) *nbad = red[0];
}

static size_t lm_solve_lds_bytes(int n) { return ((size_t)n * (size_t)(n + 1) + (size_t)n) * 8; }

// the two blocks of the loop for `ntr` trace records: laid out once per plan (again when a call asks for more records), the
// dynamic-LDS attribute of the solve kernel raised for THIS plan's device
static int lm_prepare(plslam_lba_plan* P, int32_t ntr, LmDev& d, LmImage& himg, LmImage& dimg)
{
    if (P->lm_trace_cap < ntr) {
        LmDev tmp;
        int rc;
        if ((rc = P->lm.reserve(lm_carve(P, (size_t)ntr, nullptr, tmp) + 256)) ||
            (rc = P->lm_pin.reserve(LM_CTL_BYTES + 6 * (size_t)P->nkf * 8 + LmImage::bytes((size_t)P->nkf, (size_t)ntr) + 256)))
            return rc;
        // (the attribute belongs to the kernel on this device, not to the plan: every plan raises it to the SAME value, the largest
        // system the kernel takes, so no plan can lower it under another's feet)
        if (6 * P->nkf <= LM_SOLVE_MAX_N6)
            PLSLAM_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_lm_solve), hipFuncAttributeMaxDynamicSharedMemorySize,
                                                 (int)lm_solve_lds_bytes(LM_SOLVE_MAX_N6)));
        P->lm_trace_cap = ntr;
    }
    const size_t cap = (size_t)P->lm_trace_cap;
    lm_carve(P, cap, P->lm.as<char>(), d);
    const size_t in_bytes = LM_CTL_BYTES + 6 * (size_t)P->nkf * 8;
    himg = LmImage(P->lm_pin.as<char>() + in_bytes, (size_t)P->nkf, cap);
    dimg = P->lm_pin.dev ? LmImage(static_cast<char*>(P->lm_pin.dev) + in_bytes, (size_t)P->nkf, cap) : LmImage(d.img, (size_t)P->nkf, cap);
    return PLSLAM_OK;
}

}  // namespace plslam

extern "C" int plslam_lba_plan_optimize_dev(plslam_lba_plan* P, const plslam_lba_lm_params* prm, const double* T_slots, const double* x_kf,
                                            int32_t first_estimate_slot, double* x_kf_out, double* T_out, plslam_lba_solve* trace,
                                            plslam_lba_result* result)
{
    PLSLAM_REQUIRE(P && prm && T_slots && x_kf && x_kf_out && result, PLSLAM_EINVAL);
    PLSLAM_REQUIRE(prm->lambda_lba_k != 0.0, PLSLAM_EINVAL);
    plslam_ctx* ctx = P->ctx;
    std::lock_guard<std::mutex> lk(ctx->mu);
    DeviceGuard dg_(ctx->device);
    PLSLAM_REQUIRE(P->nkf >= 1 && first_estimate_slot >= 0 && first_estimate_slot + P->nkf <= P->n_slots, PLSLAM_EINVAL);
    PLSLAM_REQUIRE(P->state_valid || P->lm_resident, PLSLAM_EINVAL);      // the landmarks must be resident
    hipStream_t s = ctx->stream;
    const int32_t nkf = P->nkf, n6 = 6 * nkf;
    const int32_t ntr = std::max(prm->max_iters_lba, 1);
    int rc = lba_schur_prepare(P);
    if (rc) return rc;
    LmDev D;
    LmImage H, I;                          // the image as the host reads it, and as the kernels address it
    if ((rc = lm_prepare(P, ntr, D, H, I))) return rc;
    const bool mapped = P->lm_pin.dev != nullptr;
    const size_t img_bytes = LmImage::bytes((size_t)nkf, (size_t)P->lm_trace_cap);
    StreamSyncOnError drain(s);
    // ---- up, once: the pose slots, the control block with x_kf behind it (and the cleared image where the device has its own)
    memcpy(P->hx.T, T_slots, P->hx.T.bytes);
    PLSLAM_HIP_CHECK(hipMemcpyAsync(P->x.T, P->hx.T, P->x.T.bytes, hipMemcpyHostToDevice, s));
    char* pin = P->lm_pin.as<char>();
    LbaLmCtl c0;
    lm_init(c0);
    memset(pin, 0, LM_CTL_BYTES);
    memcpy(pin, &c0, sizeof c0);
    memcpy(pin + LM_CTL_BYTES, x_kf, (size_t)n6 * 8);
    memset(H.peek, 0, img_bytes);
    PLSLAM_HIP_CHECK(hipMemcpyAsync(D.ctl, pin, LM_CTL_BYTES + (size_t)n6 * 8, hipMemcpyHostToDevice, s));
    if (!mapped) PLSLAM_HIP_CHECK(hipMemcpyAsync(D.img, H.peek, img_bytes, hipMemcpyHostToDevice, s));
    P->state_valid = true;
    LbaLmPrm prmd{prm->lambda_lba_lm, prm->lambda_lba_k, prm->min_error_change, prm->min_error, (double)(P->npt + P->nls),
                  prm->max_iters_lba, 0};
    const LbaOutView& O = P->o;
    const LbaSchurView& C = P->sc;
    LmSolveArgs A{};
    A.ctl = D.ctl; A.prm = prmd; A.S = C.tail.S; A.b = C.tail.b; A.err_src = O.err;
    A.dp = C.dp; A.x = D.x; A.Test = P->x.T + 16 * (size_t)first_estimate_slot;
    A.trace = I.trace; A.peek = I.peek; A.nkf = nkf;
    const int32_t nwg_back = lba_backsub_wgs(P);
    const bool peek = ctx->lba_loop_peek != 0 && mapped;
    const volatile int32_t* stop_word = H.peek;
    int32_t n_enq = 0;
    for (int32_t pass = 0; pass < ntr; ++pass) {
        if (pass > 0 && peek && *stop_word) break;         // (the loop has ended on the device: what is enqueued behind it does nothing)
        int par = 0;
        if (pass == 0) {
            if ((rc = lba_plan_enqueue(P, nullptr, nullptr, nullptr, 0, false, -1.0, D.ctl))) return rc;
            hipLaunchKernelGGL(k_lm_first, dim3(1), dim3(LM_WG), 0, s, (const double*)O.H_pose, nkf, (const double*)O.H_pt, P->npt,
                               (const double*)O.H_ls, P->nls, D.ctl, prmd);
            if ((rc = lba_schur_enqueue(P, 0.0, &par, false, D.ctl))) return rc;
        } else {
            if ((rc = lba_plan_enqueue(P, nullptr, nullptr, nullptr, PLSLAM_LBA_COMPAT_ITER_PASS, false, 0.0, D.ctl))) return rc;
            if ((rc = lba_schur_enqueue(P, 0.0, &par, true, D.ctl))) return rc;
        }
        if (n6 <= LM_SOLVE_MAX_N6) {
            hipLaunchKernelGGL(k_lm_solve, dim3(1), dim3(LM_WG), lm_solve_lds_bytes(n6), s, A);
        } else {
            const int32_t npad = (int32_t)pad_to_tile(n6);
            hipLaunchKernelGGL(k_lm_pre, dim3(1), dim3(64), 0, s, A);
            hipLaunchKernelGGL(k_lm_pad, dim3(npad), dim3(LM_WG), 0, s, (const LbaLmCtl*)D.ctl, A.S, A.b, n6, npad, D.Spad, D.w);
            if ((rc = ldlt_enqueue(D.Spad, npad, n6, D.Ppan, D.w, D.z, D.xs, D.badp, s))) return rc;
            hipLaunchKernelGGL(k_lm_post, dim3(1), dim3(LM_WG), 0, s, A, (const double*)D.Spad, npad, (const double*)D.xs);
        }
        if ((rc = lba_backsub_enqueue_lm(P, D.ctl))) return rc;
        hipLaunchKernelGGL(k_lm_tail, dim3(1), dim3(64), 0, s, D.ctl, prmd, (const double*)C.dx_part, nwg_back,
                           (const int32_t*)(C.tail.sing + par), I.trace, I.peek);
        PLSLAM_HIP_CHECK(hipGetLastError());
        ++n_enq;
    }
    hipLaunchKernelGGL(k_lm_final, dim3((nkf + 63) / 64), dim3(64), 0, s, (const LbaLmCtl*)D.ctl, (const double*)D.x, nkf, I.result, I.x,
                       I.T, C.tail.sing);
    PLSLAM_HIP_CHECK(hipGetLastError());
    if (!mapped) PLSLAM_HIP_CHECK(hipMemcpyAsync(H.peek, D.img, img_bytes, hipMemcpyDeviceToHost, s));
    PLSLAM_HIP_CHECK(hipStreamSynchronize(s));             // the call's ONE synchronisation
    drain.dismiss();
    P->schur_parity = 0;
    P->schur_done = false;
    *result = *H.result;
    result->n_enqueued_passes = n_enq;
    memcpy(x_kf_out, H.x, (size_t)n6 * 8);
    if (T_out) memcpy(T_out, H.T, (size_t)nkf * 128);
    if (trace) memcpy(trace, H.trace, (size_t)ntr * sizeof(plslam_lba_solve));
    return PLSLAM_OK;
}

extern "C" int plslam_lba_reduced_ldlt_solve(plslam_ctx* ctx, int32_t n, const double* A, const double* b, double* x, int32_t* n_bad_pivots)
{
    PLSLAM_REQUIRE(ctx && n >= 1 && A && b && x && n <= 6 * PLSLAM_GBA_MAX_KEYFRAMES, PLSLAM_EINVAL);
    std::lock_guard<std::mutex> lk(ctx->mu);
    DeviceGuard dg_(ctx->device);
    hipStream_t s = ctx->stream;
    const bool lds = n <= LM_SOLVE_MAX_N6;
    const size_t npad = lds ? (size_t)n : (size_t)pad_to_tile(n);
    DevBuf buf;
    ArrCarver c{nullptr};
    auto carve = [&](char* base) {
        c = ArrCarver{base};
        struct V { Arr<double> S, P, w, z, x; Arr<int32_t> badp, nbad; } v;
        v.S = c.take<double>(npad * npad * 8); v.P = c.take<double>(npad * LT * 8); v.w = c.take<double>(npad * 8);
        v.z = c.take<double>(npad * 8); v.x = c.take<double>(npad * 8); v.badp = c.take<int32_t>((npad / LT + 1) * 4);
        v.nbad = c.take<int32_t>(4);
        return v;
    };
    carve(nullptr);
    int rc = buf.reserve(c.size());
    if (rc) return rc;
    ReleaseAfterSync rel{buf, s};
    const auto v = carve(buf.as<char>());
    if (!lds) {
        PLSLAM_HIP_CHECK(hipMemsetAsync(v.S, 0, v.S.bytes, s));
        PLSLAM_HIP_CHECK(hipMemsetAsync(v.w, 0, v.w.bytes, s));
    }
    PLSLAM_HIP_CHECK(hipMemcpy2DAsync(v.S, npad * 8, A, (size_t)n * 8, (size_t)n * 8, n, hipMemcpyHostToDevice, s));
    PLSLAM_HIP_CHECK(hipMemcpyAsync(v.w, b, (size_t)n * 8, hipMemcpyHostToDevice, s));
    if (lds) {
        PLSLAM_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_lm_solve_host), hipFuncAttributeMaxDynamicSharedMemorySize,
                                             (int)lm_solve_lds_bytes(LM_SOLVE_MAX_N6)));
        hipLaunchKernelGGL(k_lm_solve_host, dim3(1), dim3(LM_WG), lm_solve_lds_bytes(n), s, (const double*)v.S, (const double*)v.w, n, v.x.p,
                           v.nbad.p);
    } else {
        ldlt_pad_diag_enqueue(v.S, (int64_t)npad, n, s);
        if ((rc = ldlt_enqueue(v.S, (int64_t)npad, n, v.P, v.w, v.z, v.x, v.badp, s))) return rc;
        hipLaunchKernelGGL(k_lm_count_pivots, dim3(1), dim3(LM_WG), 0, s, (const double*)v.S, n, (int32_t)npad, v.nbad.p);
    }
    PLSLAM_HIP_CHECK(hipGetLastError());
    int32_t nb = 0;
    PLSLAM_HIP_CHECK(hipMemcpyAsync(x, v.x, (size_t)n * 8, hipMemcpyDeviceToHost, s));
    PLSLAM_HIP_CHECK(hipMemcpyAsync(&nb, v.nbad, 4, hipMemcpyDeviceToHost, s));
    PLSLAM_HIP_CHECK(hipStreamSynchronize(s));
    if (n_bad_pivots) *n_bad_pivots = nb;
    return PLSLAM_OK;
}
