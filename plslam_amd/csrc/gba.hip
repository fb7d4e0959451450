// gba.hip -- the global bundle adjustment of the reference (MapHandler::globalBundleAdjustment + levMarquardtOptimizationGBA,
// src/mapHandler.cpp:1995-2099, :2101-2703) on the device, on top of the LBA plan's public device-block API.
//
// The rows, H and g of every pass are the LBA plan's (plslam_lba_plan_iterate_dev / _iterate_resident: PLSLAM_LBA_COMPAT_GBA on
// the first pass, PLSLAM_LBA_COMPAT_ITER_PASS on every later one -- DESIGN.md section 5).  What this file adds is the solve that
// scales to the whole map:
//   K26 k_gba_hmax             max |H(i,i)| over all N diagonal entries (the first pass's Hmax, :2359-2364)
//   K27 k_gba_landmarks<DL>    a lane per landmark: Vj' = Vj + lambda diag(Vj), its inverse (Gauss-Jordan, no pivoting: a pivot
//                              that is not positive makes the landmark singular -- no contribution, zero step), tj = Vj'^-1 gj
//   K28 k_gba_cross<DL>        a lane per observation of an optimised keyframe: Y_o = Vj'^-1 W_o
//   K29 k_gba_pairs            a workgroup per ragged chunk (<= 64 observation pairs of one covisible block, one kind): the
//                              chunk's sum of W_o1^T Y_o2, pair after pair
//   K30 k_gba_blocks           a workgroup per covisible block (k1 >= k2): S(k1,k2) = [H_pose + lambda diag]delta - chunk sums
//   K31 k_gba_rhs              a workgroup per keyframe: b_k = g_k - sum_o W_o^T t_lm(o)
//   K32-K36                    the dense blocked L D L^T of S and its triangular solves: ldlt_dense.hip, through ldlt_dense.hpp
//   K37 k_gba_backsub<DL>      a lane per landmark: dxj = Vj'^-1 (gj - sum_o W_o dp[kf(o)]), X += dx when the step is taken
//   K38 k_gba_pose             a lane per optimised keyframe: x <- logmap(expmap(x) inverse(expmap(dp))), its estimate slot
//   K39 k_gba_stats            ||DX||^2 over all N unknowns, singular landmarks, bad pivots: 24 bytes for the host
// Every sum has a fixed shape (no floating-point atomics): two runs give the same bits.  Phases are ordered by kernel
// boundaries only -- no grid barrier, no device-scope fence.
//
// The lists the kernels walk are host work (gba_lists.hpp) or built on the device (gba_plan_dev.hip); the plan object is in
// gba_plan.hpp.  The plan's buffers are named ONCE: each is carved in one function (gba_carve_stat, gba_carve_pairs,
// gba_carve_work), which fills a view of typed pointers with the bytes behind each; every launch site, upload and download reads
// the views.  The LM loop is ONE body (gba_optimize) behind plslam_gba_optimize (host state) and plslam_gba_optimize_dev (device
// state: the landmarks stay resident in the LBA plan, plslam_local_map_apply_gba writes them into the map image).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <limits>
#include <vector>

#include "common.hpp"
#include "gba_plan.hpp"
#include "lba_plan.hpp"
#include "ldlt_dense.hpp"
#include "pose_step_dev.hpp"

namespace plslam {
namespace {

// ---- K26 ----------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
k_gba_hmax(const double* __restrict__ Hp, int32_t nkf, const double* __restrict__ Hpt, int32_t npt, const double* __restrict__ Hls,
           int32_t nls, double* __restrict__ out)
{
    __shared__ double red[256];
    const int t = threadIdx.x;
    const int64_t n1 = 6 * (int64_t)nkf, n2 = n1 + 3 * (int64_t)npt, n3 = n2 + 6 * (int64_t)nls;
    double m = 0.0;
    for (int64_t i = t; i < n3; i += 256) {
        double v;
        if (i < n1) v = Hp[(i / 6) * 36 + (i % 6) * 7];
        else if (i < n2) v = Hpt[((i - n1) / 3) * 9 + ((i - n1) % 3) * 4];
        else v = Hls[((i - n2) / 6) * 36 + ((i - n2) % 6) * 7];
        v = fabs(v);
        if (v > m) m = v;            // a NaN diagonal never wins the comparison (as in the reference's test)
    }
    red[t] = m;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (t < s && red[t + s] > red[t]) red[t] = red[t + s];
        __syncthreads();
    }
    if (t == 0) out[0] = red[0];
}

// ---- K27 ----------------------------------------------------------------------------------------------------------------
template <int DL>
__global__ void __launch_bounds__(256)
k_gba_landmarks(const double* __restrict__ H, const double* __restrict__ g, int32_t nlm, double lambda, double* __restrict__ Vinv,
                double* __restrict__ tv, int32_t* __restrict__ sing)
{
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= nlm) return;
    double A[DL][DL], I[DL][DL];
#pragma unroll
    for (int a = 0; a < DL; ++a)
#pragma unroll
        for (int b = 0; b < DL; ++b) {
            const double h = H[(size_t)j * DL * DL + a * DL + b];
            A[a][b] = a == b ? h + lambda * h : h;
            I[a][b] = a == b ? 1.0 : 0.0;
        }
    bool ok = true;
#pragma unroll
    for (int c = 0; c < DL; ++c) {
        const double piv = A[c][c];
        ok = ok && piv > 0.0;
        const double ip = 1.0 / (piv > 0.0 ? piv : 1.0);
#pragma unroll
        for (int b = 0; b < DL; ++b) { A[c][b] *= ip; I[c][b] *= ip; }
#pragma unroll
        for (int a = 0; a < DL; ++a) {
            if (a == c) continue;
            const double f = A[a][c];
#pragma unroll
            for (int b = 0; b < DL; ++b) { A[a][b] -= f * A[c][b]; I[a][b] -= f * I[c][b]; }
        }
    }
    double gj[DL];
#pragma unroll
    for (int a = 0; a < DL; ++a) gj[a] = g[(size_t)j * DL + a];
#pragma unroll
    for (int a = 0; a < DL; ++a) {
        double acc = 0.0;
#pragma unroll
        for (int b = 0; b < DL; ++b) {
            const double v = ok ? I[a][b] : 0.0;
            Vinv[(size_t)j * DL * DL + a * DL + b] = v;
            acc += v * gj[b];
        }
        tv[(size_t)j * DL + a] = acc;
    }
    sing[j] = ok ? 0 : 1;
}

// ---- K28: Y_o = Vinv_j W_o (DL x 6), for the observations of optimised keyframes ------------------------------------------------
template <int DL>
__global__ void __launch_bounds__(256)
k_gba_cross(const int32_t* __restrict__ lm, const int32_t* __restrict__ kf, int32_t nobs, const double* __restrict__ Vinv,
            const double* __restrict__ W, double* __restrict__ Y)
{
    const int o = blockIdx.x * 256 + threadIdx.x;
    if (o >= nobs || kf[o] < 0) return;
    const int j = lm[o];
    double V[DL * DL], w[DL * 6];
#pragma unroll
    for (int i = 0; i < DL * DL; ++i) V[i] = Vinv[(size_t)j * DL * DL + i];
#pragma unroll
    for (int i = 0; i < DL * 6; ++i) w[i] = W[(size_t)o * DL * 6 + i];
#pragma unroll
    for (int x = 0; x < DL; ++x)
#pragma unroll
        for (int b = 0; b < 6; ++b) {
            double acc = 0.0;
#pragma unroll
            for (int y = 0; y < DL; ++y) acc += V[x * DL + y] * w[y * 6 + b];
            Y[(size_t)o * DL * 6 + x * 6 + b] = acc;
        }
}

// ---- K29: a chunk's sum of W_o1^T Y_o2 -----------------------------------------------------------------------------------
template <int DL>
__device__ __forceinline__ void gba_pair_product(const double* __restrict__ W, const double* __restrict__ Y, int o1, int o2,
                                                 double* __restrict__ out /* LDS, [36] with stride GBA_CHUNK */)
{
    double w1[DL * 6], y2[DL * 6];
#pragma unroll
    for (int i = 0; i < DL * 6; ++i) { w1[i] = W[(size_t)o1 * DL * 6 + i]; y2[i] = Y[(size_t)o2 * DL * 6 + i]; }
#pragma unroll
    for (int a = 0; a < 6; ++a)
#pragma unroll
        for (int b = 0; b < 6; ++b) {
            double acc = 0.0;
#pragma unroll
            for (int x = 0; x < DL; ++x) acc += w1[x * 6 + a] * y2[x * 6 + b];
            out[(a * 6 + b) * GBA_CHUNK] = acc;
        }
}

__global__ void __launch_bounds__(GBA_CHUNK)
k_gba_pairs(const GbaChunk* __restrict__ chunks, const int2* __restrict__ pairs, const double* __restrict__ W_pt,
            const double* __restrict__ Y_pt, const double* __restrict__ W_ls, const double* __restrict__ Y_ls,
            double* __restrict__ part)
{
    __shared__ double prod[36 * GBA_CHUNK];
    const GbaChunk c = chunks[blockIdx.x];
    const int i = threadIdx.x;
    if (i < c.np) {
        const int2 q = pairs[c.p0 + i];
        if (c.line) gba_pair_product<6>(W_ls, Y_ls, q.x, q.y, prod + i);
        else gba_pair_product<3>(W_pt, Y_pt, q.x, q.y, prod + i);
    }
    __syncthreads();
    if (i < 36) {
        double s = 0.0;
        for (int p = 0; p < c.np; ++p) s += prod[i * GBA_CHUNK + p];    // pair after pair, in list order
        part[(size_t)blockIdx.x * 36 + i] = s;
    }
}

// ---- K30: S(k1,k2) = [H_pose + lambda diag] delta(k1,k2) - sum of its chunks, lower blocks only ---------------------------------
__global__ void __launch_bounds__(64)
k_gba_blocks(const GbaBlock* __restrict__ blocks, const double* __restrict__ part, const double* __restrict__ Hp, double lambda,
             double* __restrict__ S, int64_t ld)
{
    const GbaBlock B = blocks[blockIdx.x];
    const int e = threadIdx.x;
    if (e >= 36) return;
    const int a = e / 6, b = e % 6;
    double v = 0.0;
    if (B.k1 == B.k2) {
        const double h = Hp[(size_t)B.k1 * 36 + e];
        v = a == b ? h + lambda * h : h;
    }
    for (int c = B.c0; c < B.c1; ++c) v -= part[(size_t)c * 36 + e];
    S[(6 * (int64_t)B.k1 + a) * ld + 6 * (int64_t)B.k2 + b] = v;
}

// ---- K31: b_k = g_k - sum over the keyframe's observations of W_o^T t_lm(o) ---------------------------------------------------
template <int DL>
__device__ __forceinline__ void gba_rhs_term(const double* __restrict__ W, const double* __restrict__ tv, int o, int j, double (&acc)[6])
{
    double t[DL];
#pragma unroll
    for (int x = 0; x < DL; ++x) t[x] = tv[(size_t)j * DL + x];
#pragma unroll
    for (int a = 0; a < 6; ++a) {
        double s = 0.0;
#pragma unroll
        for (int x = 0; x < DL; ++x) s += W[(size_t)o * DL * 6 + x * 6 + a] * t[x];
        acc[a] += s;
    }
}

__global__ void __launch_bounds__(64)
k_gba_rhs(const int32_t* __restrict__ kp_ptr, const int32_t* __restrict__ kp_obs, const int32_t* __restrict__ kl_ptr,
          const int32_t* __restrict__ kl_obs, const int32_t* __restrict__ pt_lm, const int32_t* __restrict__ ls_lm,
          const double* __restrict__ W_pt, const double* __restrict__ t_pt, const double* __restrict__ W_ls,
          const double* __restrict__ t_ls, const double* __restrict__ g, double* __restrict__ b)
{
    __shared__ double red[6][64];
    const int k = blockIdx.x, i = threadIdx.x;
    double acc[6] = {0, 0, 0, 0, 0, 0};
    for (int q = kp_ptr[k] + i; q < kp_ptr[k + 1]; q += 64) { const int o = kp_obs[q]; gba_rhs_term<3>(W_pt, t_pt, o, pt_lm[o], acc); }
    for (int q = kl_ptr[k] + i; q < kl_ptr[k + 1]; q += 64) { const int o = kl_obs[q]; gba_rhs_term<6>(W_ls, t_ls, o, ls_lm[o], acc); }
#pragma unroll
    for (int a = 0; a < 6; ++a) red[a][i] = acc[a];
    __syncthreads();
    for (int s = 32; s > 0; s >>= 1) {
        if (i < s)
#pragma unroll
            for (int a = 0; a < 6; ++a) red[a][i] += red[a][i + s];
        __syncthreads();
    }
    if (i < 6) b[6 * (size_t)k + i] = g[6 * (size_t)k + i] - red[i][0];
}

// ---- K37: landmark steps ----------------------------------------------------------------------------------------------------
template <int DL>
__global__ void __launch_bounds__(256)
k_gba_backsub(const int32_t* __restrict__ lm_ptr, const int32_t* __restrict__ lm_obs, const int32_t* __restrict__ kf,
              int32_t nlm, const double* __restrict__ W, const double* __restrict__ Vinv, const double* __restrict__ g,
              const double* __restrict__ dp, int32_t apply, double* __restrict__ X, double* __restrict__ part)
{
    __shared__ double red[256];
    const int t = threadIdx.x, j = blockIdx.x * 256 + t;
    double ss = 0.0;
    if (j < nlm) {
        double rhs[DL];
#pragma unroll
        for (int x = 0; x < DL; ++x) rhs[x] = g[(size_t)j * DL + x];
        for (int q = lm_ptr[j]; q < lm_ptr[j + 1]; ++q) {
            const int o = lm_obs[q];
            const int k = kf[o];
            double d[6];
#pragma unroll
            for (int a = 0; a < 6; ++a) d[a] = dp[6 * (size_t)k + a];
#pragma unroll
            for (int x = 0; x < DL; ++x) {
                double s = 0.0;
#pragma unroll
                for (int a = 0; a < 6; ++a) s += W[(size_t)o * DL * 6 + x * 6 + a] * d[a];
                rhs[x] -= s;
            }
        }
#pragma unroll
        for (int x = 0; x < DL; ++x) {
            double s = 0.0;
#pragma unroll
            for (int y = 0; y < DL; ++y) s += Vinv[(size_t)j * DL * DL + x * DL + y] * rhs[y];
            ss += s * s;
            if (apply) X[(size_t)j * DL + x] += s;
        }
    }
    red[t] = ss;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (t < s) red[t] += red[t + s];
        __syncthreads();
    }
    if (t == 0) part[blockIdx.x] = red[0];
}

// ---- K38: the pose update of :2371-2377 / :2650-2655, and the estimate slot the next pass's point rows read -----------------------
__global__ void __launch_bounds__(256)
k_gba_pose(int32_t nkf, const double* __restrict__ dp, int32_t apply, double* __restrict__ xkf, double* __restrict__ Test,
           double* __restrict__ part)
{
    __shared__ double red[256];
    const int t = threadIdx.x, k = blockIdx.x * 256 + t;
    double ss = 0.0;
    if (k < nkf) {
        double d[6], x[6];
#pragma unroll
        for (int a = 0; a < 6; ++a) { d[a] = dp[6 * (size_t)k + a]; ss += d[a] * d[a]; x[a] = xkf[6 * (size_t)k + a]; }
        if (apply) {
            double Tp[16];
            pose_step_se3(d, x, Tp);
#pragma unroll
            for (int a = 0; a < 6; ++a) xkf[6 * (size_t)k + a] = x[a];
#pragma unroll
            for (int i = 0; i < 16; ++i) Test[16 * (size_t)k + i] = Tp[i];
        }
    }
    red[t] = ss;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (t < s) red[t] += red[t + s];
        __syncthreads();
    }
    if (t == 0) part[blockIdx.x] = red[0];
}

// ---- K39 -------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
k_gba_stats(const double* __restrict__ part, int32_t npart, const int32_t* __restrict__ sing, int32_t nsing,
            const int32_t* __restrict__ badp, int32_t nbad, GbaStats* __restrict__ out)
{
    __shared__ int32_t red[256];
    const int t = threadIdx.x;
    int c = 0;
    for (int i = t; i < nsing; i += 256) c += sing[i];
    red[t] = c;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (t < s) red[t] += red[t + s];
        __syncthreads();
    }
    if (t == 0) {
        double ss = 0.0;
        for (int i = 0; i < npart; ++i) ss += part[i];     // the partials in a fixed order
        int nb = 0;
        for (int i = 0; i < nbad; ++i) nb += badp[i];
        out->dx_sumsq = ss;
        out->n_singular = red[0];
        out->n_bad_pivots = nb;
    }
}

}  // namespace
}  // namespace plslam

using namespace plslam;

namespace plslam {

size_t gba_carve_stat(plslam_gba_plan* G, const GbaListRoom& r, char* base)
{
    GbaStatView& v = G->st;
    ArrCarver c{base};
    const size_t np = (size_t)G->np, nl = (size_t)G->nl;
    v.plm = c.take<int32_t>(np * 4, 4);
    v.pkf = c.take<int32_t>(np * 4, 4);
    v.llm = c.take<int32_t>(nl * 4, 4);
    v.lkf = c.take<int32_t>(nl * 4, 4);
    v.kpp = c.take<int32_t>(((size_t)G->nkf + 1) * 4);
    v.kpo = c.take<int32_t>(r.kpo * 4, 4);
    v.klp = c.take<int32_t>(((size_t)G->nkf + 1) * 4);
    v.klo = c.take<int32_t>(r.klo * 4, 4);
    v.lpp = c.take<int32_t>(((size_t)G->npt + 1) * 4);
    v.lpo = c.take<int32_t>(r.lpo * 4, 4);
    v.llp = c.take<int32_t>(((size_t)G->nls + 1) * 4);
    v.llo = c.take<int32_t>(r.llo * 4, 4);
    return c.size();
}

size_t gba_carve_pairs(plslam_gba_plan* G, const GbaListRoom& r, char* base)
{
    GbaStatView& v = G->st;
    ArrCarver c{base};
    v.blk = c.take<GbaBlock>(r.nblk * sizeof(GbaBlock));
    v.chk = c.take<GbaChunk>(r.nchunk * sizeof(GbaChunk), 16);
    v.pair = c.take<int2>(r.npair * sizeof(int2), 8);
    return c.size();
}

size_t gba_carve_work(plslam_gba_plan* G, char* base)
{
    GbaWorkView& v = G->wk;
    ArrCarver c{base};
    const size_t npt = (size_t)G->npt, nls = (size_t)G->nls, np = (size_t)G->np, nl = (size_t)G->nl, npad = (size_t)G->npad;
    v.Vp = c.take<double>(npt * 72, 8);
    v.tp = c.take<double>(npt * 24, 8);
    v.Vl = c.take<double>(nls * 288, 8);
    v.tl = c.take<double>(nls * 48, 8);
    // the one deliberate adjacency: K39 counts the singular landmarks of both kinds in one pass over npt + nls flags, so the
    // lines' flags directly follow the points'
    v.sing = c.take<int32_t>((npt + nls) * 4, 8);
    v.sing_pt = {v.sing.p, npt * 4};
    v.sing_ls = {v.sing.p + npt, nls * 4};
    v.Yp = c.take<double>(np * 144, 8);
    v.Yl = c.take<double>(nl * 288, 8);
    v.part = c.take<double>((size_t)G->nchunk * 288, 8);
    v.P = c.take<double>(npad * LT * 8);
    v.w = c.take<double>(npad * 8);
    v.z = c.take<double>(npad * 8);
    v.dp = c.take<double>(npad * 8);
    v.bad = c.take<int32_t>((size_t)G->nt * 4, 4);
    v.ss_part = c.take<double>((size_t)(G->nwk() + G->nwp() + G->nwl()) * 8, 8);
    v.stats = c.take<GbaStats>(sizeof(GbaStats));
    v.hmax = c.take<double>(8);
    v.x = c.take<double>((size_t)G->nkf * 48);
    return c.size();
}

int gba_fail(plslam_gba_plan* G, int rc)
{
    {
        DeviceGuard dg_(G->ctx->device);
        (void)hipStreamSynchronize(G->ctx->stream);        // (a device-built plan: its builders may still read the scratch)
    }
    if (G->lba) plslam_lba_plan_destroy(G->lba);
    G->release();
    delete G;
    return rc;
}

// one damped solve on the blocks the LBA plan left on the device: Schur complement, LDL^T, landmark and pose steps, stats
static int gba_solve_enqueue(plslam_gba_plan* G, double lambda, bool apply, hipStream_t s)
{
    plslam_lba_blocks B;
    plslam_lba_state st;
    int rc;
    if ((rc = plslam_lba_plan_device_blocks(G->lba, &B)) || (rc = plslam_lba_plan_device_state(G->lba, &st))) return rc;
    const GbaStatView& l = G->st;
    const GbaWorkView& w = G->wk;
    double* S = G->Sbuf.as<double>();
    const int32_t nkf = G->nkf, npt = G->npt, nls = G->nls;
    const double* g_pt = B.g + 6 * (size_t)nkf;
    const double* g_ls = g_pt + 3 * (size_t)npt;
    if (npt)
        hipLaunchKernelGGL(k_gba_landmarks<3>, dim3((npt + 255) / 256), dim3(256), 0, s, B.H_pt, g_pt, npt, lambda, w.Vp.p, w.tp.p,
                           w.sing_pt.p);
    if (nls)
        hipLaunchKernelGGL(k_gba_landmarks<6>, dim3((nls + 255) / 256), dim3(256), 0, s, B.H_ls, g_ls, nls, lambda, w.Vl.p, w.tl.p,
                           w.sing_ls.p);
    if (G->np)
        hipLaunchKernelGGL(k_gba_cross<3>, dim3((G->np + 255) / 256), dim3(256), 0, s, (const int32_t*)l.plm, (const int32_t*)l.pkf,
                           G->np, (const double*)w.Vp, B.W_pt, w.Yp.p);
    if (G->nl)
        hipLaunchKernelGGL(k_gba_cross<6>, dim3((G->nl + 255) / 256), dim3(256), 0, s, (const int32_t*)l.llm, (const int32_t*)l.lkf,
                           G->nl, (const double*)w.Vl, B.W_ls, w.Yl.p);
    PLSLAM_HIP_CHECK(hipMemsetAsync(S, 0, (size_t)G->npad * (size_t)G->npad * 8, s));
    PLSLAM_HIP_CHECK(hipMemsetAsync(w.w, 0, w.w.bytes, s));
    if (G->nchunk)
        hipLaunchKernelGGL(k_gba_pairs, dim3(G->nchunk), dim3(GBA_CHUNK), 0, s, (const GbaChunk*)l.chk, (const int2*)l.pair, B.W_pt,
                           (const double*)w.Yp, B.W_ls, (const double*)w.Yl, w.part.p);
    hipLaunchKernelGGL(k_gba_blocks, dim3(G->nblk), dim3(64), 0, s, (const GbaBlock*)l.blk, (const double*)w.part, B.H_pose, lambda,
                       S, G->npad);
    ldlt_pad_diag_enqueue(S, G->npad, (int32_t)G->n, s);
    hipLaunchKernelGGL(k_gba_rhs, dim3(nkf), dim3(64), 0, s, (const int32_t*)l.kpp, (const int32_t*)l.kpo, (const int32_t*)l.klp,
                       (const int32_t*)l.klo, (const int32_t*)l.plm, (const int32_t*)l.llm, B.W_pt, (const double*)w.tp, B.W_ls,
                       (const double*)w.tl, B.g, w.w.p);
    if ((rc = ldlt_enqueue(S, G->npad, (int32_t)G->n, w.P, w.w, w.z, w.dp, w.bad, s))) return rc;
    const int nwp = G->nwp(), nwl = G->nwl(), nwk = G->nwk();
    double* part = w.ss_part;
    hipLaunchKernelGGL(k_gba_pose, dim3(nwk), dim3(256), 0, s, nkf, (const double*)w.dp, (int32_t)apply, w.x.p,
                       st.T_kf_w + 16 * (size_t)G->n_map, part);
    if (npt)
        hipLaunchKernelGGL(k_gba_backsub<3>, dim3(nwp), dim3(256), 0, s, (const int32_t*)l.lpp, (const int32_t*)l.lpo,
                           (const int32_t*)l.pkf, npt, B.W_pt, (const double*)w.Vp, g_pt, (const double*)w.dp, (int32_t)apply, st.Xw,
                           part + nwk);
    if (nls)
        hipLaunchKernelGGL(k_gba_backsub<6>, dim3(nwl), dim3(256), 0, s, (const int32_t*)l.llp, (const int32_t*)l.llo,
                           (const int32_t*)l.lkf, nls, B.W_ls, (const double*)w.Vl, g_ls, (const double*)w.dp, (int32_t)apply, st.Lw,
                           part + nwk + nwp);
    hipLaunchKernelGGL(k_gba_stats, dim3(1), dim3(256), 0, s, (const double*)part, nwk + nwp + nwl, (const int32_t*)w.sing, npt + nls,
                       (const int32_t*)w.bad, G->nt, w.stats.p);
    PLSLAM_HIP_CHECK(hipGetLastError());
    return PLSLAM_OK;
}

int gba_plan_args_ok(plslam_ctx* ctx, const plslam_cam* K, double homog_th, int32_t n_map_kf, int32_t nkf, const void* kf_list, int32_t npt,
                     int32_t nls, const void* pt_obs, const void* pt_obs_uv, int32_t n_pt_obs, const void* ls_obs, const void* ls_l_obs,
                     int32_t n_ls_obs, plslam_gba_plan** out)
{
    PLSLAM_REQUIRE(ctx && K && out && n_map_kf >= 0 && nkf >= 1 && npt >= 0 && nls >= 0 && n_pt_obs >= 0 && n_ls_obs >= 0,
                   PLSLAM_EINVAL);
    *out = nullptr;
    PLSLAM_REQUIRE(nkf <= PLSLAM_GBA_MAX_KEYFRAMES && kf_list, PLSLAM_EINVAL);
    // the iteration pass's line rows are the LBA plan's COMPAT_ITER_PASS rows only where homogTh is the literal they spell
    PLSLAM_REQUIRE(homog_th == 1e-7, PLSLAM_EINVAL);
    PLSLAM_REQUIRE(n_pt_obs == 0 || (pt_obs && pt_obs_uv), PLSLAM_EINVAL);
    PLSLAM_REQUIRE(n_ls_obs == 0 || (ls_obs && ls_l_obs), PLSLAM_EINVAL);
    // 32-bit addressing: observation blocks (DL x 6 doubles each), landmark blocks and pair lists are indexed with int32
    PLSLAM_REQUIRE((int64_t)n_pt_obs * 18 < INT32_MAX && (int64_t)n_ls_obs * 36 < INT32_MAX &&
                   (int64_t)npt * 9 < INT32_MAX && (int64_t)nls * 36 < INT32_MAX, PLSLAM_EINVAL);
    return PLSLAM_OK;
}

void gba_plan_dims(plslam_gba_plan* G, plslam_ctx* ctx, int32_t n_map_kf, int32_t nkf, int32_t npt, int32_t nls, int32_t n_pt_obs,
                   int32_t n_ls_obs)
{
    G->ctx = ctx; G->n_map = n_map_kf; G->nkf = nkf; G->npt = npt; G->nls = nls; G->np = n_pt_obs; G->nl = n_ls_obs;
    G->n = 6 * (int64_t)nkf;
    G->npad = pad_to_tile(G->n);
    G->nt = (int32_t)(G->npad / LT);
}

}  // namespace plslam

extern "C" {

// check the arguments the lists do not cover, plan (gba_lists.hpp), carve and upload, return
int plslam_gba_plan_create(plslam_ctx* ctx, const plslam_cam* K, double homog_th, int32_t n_map_kf, int32_t nkf, const int32_t* kf_list, int32_t npt, int32_t nls, const int32_t* pt_obs,
                           const double* pt_obs_uv, int32_t n_pt_obs, const int32_t* ls_obs, const double* ls_l_obs,
                           int32_t n_ls_obs, plslam_gba_plan** out)
{
    int rc = gba_plan_args_ok(ctx, K, homog_th, n_map_kf, nkf, kf_list, npt, nls, pt_obs, pt_obs_uv, n_pt_obs, ls_obs, ls_l_obs, n_ls_obs, out);
    if (rc) return rc;
    GbaLists L;
    rc = gba_lists_build(n_map_kf, nkf, kf_list, npt, nls, pt_obs, n_pt_obs, ls_obs, n_ls_obs, &L);
    if (rc) {
        set_last_error("plslam_gba_plan_create: %s", L.why);
        return rc;
    }
    plslam_gba_plan* G = new (std::nothrow) plslam_gba_plan();
    PLSLAM_REQUIRE(G != nullptr, PLSLAM_ENOMEM);
    gba_plan_dims(G, ctx, n_map_kf, nkf, npt, nls, n_pt_obs, n_ls_obs);
    G->kf_list.assign(kf_list, kf_list + nkf);
    G->nblk = (int32_t)L.blks.size(); G->nchunk = (int32_t)L.chks.size(); G->npair = (int64_t)L.pairs.size();
    rc = plslam_lba_plan_create(ctx, K, homog_th, n_map_kf + nkf, nkf, npt, nls, L.plm.data(), L.pslot.data(), L.pkf.data(),
                                pt_obs_uv, n_pt_obs, L.llm.data(), L.lslot.data(), L.lkf.data(), ls_l_obs, n_ls_obs, &G->lba);
    if (rc) return gba_fail(G, rc);
    const GbaListRoom room{L.lpo.size(), L.llo.size(), L.kpo.size(), L.klo.size(), L.blks.size(), L.chks.size(), L.pairs.size()};
    if ((rc = G->stat.reserve(gba_carve_stat(G, room, nullptr) + 256)) || (rc = G->pairbuf.reserve(gba_carve_pairs(G, room, nullptr) + 256)) ||
        (rc = G->work.reserve(gba_carve_work(G, nullptr) + 256)) || (rc = G->Sbuf.reserve((size_t)G->npad * (size_t)G->npad * 8)))
        return gba_fail(G, rc);
    gba_carve_stat(G, room, G->stat.as<char>());
    gba_carve_pairs(G, room, G->pairbuf.as<char>());
    gba_carve_work(G, G->work.as<char>());
    {
        std::lock_guard<std::mutex> lk(ctx->mu);
        DeviceGuard dg_(ctx->device);
        hipStream_t s = ctx->stream;
        const GbaStatView& st = G->st;
        const UploadItem ups[] = {{st.blk, L.blks.data()}, {st.chk, L.chks.data()}, {st.pair, L.pairs.data()},
                                  {st.plm, L.plm.data()}, {st.pkf, L.pkf.data()}, {st.llm, L.llm.data()}, {st.lkf, L.lkf.data()},
                                  {st.kpp, L.kpp.data()}, {st.kpo, L.kpo.data()}, {st.klp, L.klp.data()}, {st.klo, L.klo.data()},
                                  {st.lpp, L.lpp.data()}, {st.lpo, L.lpo.data()}, {st.llp, L.llp.data()}, {st.llo, L.llo.data()}};
        rc = upload_items(ups, s);
        if (hipStreamSynchronize(s) != hipSuccess && !rc) rc = PLSLAM_EHIP;
        if (rc) return gba_fail(G, rc);
    }
    *out = G;
    return PLSLAM_OK;
}

}  // extern "C"

// The LM loop both entry points run.  dev: Xw / Lw are DEVICE pointers, copied device to device into the LBA plan's resident
// state, and the landmarks stay there (no Xw_out / Lw_out); otherwise they are host pointers and go up with the poses.
static int gba_optimize(plslam_gba_plan* G, double lambda_lba_lm, double lambda_lba_k, int32_t max_iters_lba, const double* T_kf_w,
                        const double* x_kf, bool dev, const double* Xw, const double* Lw, double* x_kf_out, double* T_out, double* Xw_out,
                        double* Lw_out, plslam_gba_solve* trace, plslam_gba_result* result)
{
    PLSLAM_REQUIRE(G && x_kf && x_kf_out && (G->n_map == 0 || T_kf_w) && (G->npt == 0 || (Xw && (dev || Xw_out))) &&
                   (G->nls == 0 || (Lw && (dev || Lw_out))), PLSLAM_EINVAL);
    PLSLAM_REQUIRE(lambda_lba_k != 0.0, PLSLAM_EINVAL);
    plslam_ctx* ctx = G->ctx;
    DeviceGuard dg_(ctx->device);
    const int32_t nkf = G->nkf, n_map = G->n_map;
    const double eps = std::numeric_limits<double>::epsilon();
    // Npt_obs / Nls_obs are never incremented (:2121, :2230): every err is divided by zero (:2356, :2635)
    const double n_obs_counted = 0.0;
    // pose slots: the stored T_kf_w of every keyframe, then the estimate slots -- which hold the stored poses too on the first
    // pass (:2136: every row of the first pass reads map_keyframes[kf]->T_kf_w)
    std::vector<double> T((size_t)(n_map + nkf) * 16);
    if (n_map) std::memcpy(T.data(), T_kf_w, (size_t)n_map * 128);
    for (int32_t k = 0; k < nkf; ++k) std::memcpy(&T[16 * (size_t)(n_map + k)], &T_kf_w[16 * (size_t)G->kf_list[k]], 128);
    double err_raw = 0.0;
    int rc;
    G->optimized = false;
    if (!dev) rc = plslam_lba_plan_iterate_dev(G->lba, T.data(), Xw, Lw, PLSLAM_LBA_COMPAT_GBA, nullptr, &err_raw);
    else {
        // the same first pass on the same state: the landmarks device to device, the poses up, then the resident iteration
        plslam_lba_plan* P = G->lba;
        {
            std::lock_guard<std::mutex> lk(ctx->mu);
            DeviceGuard dg1_(ctx->device);
            hipStream_t s1 = ctx->stream;
            StreamSyncOnError guard(s1);
            if (G->npt) PLSLAM_HIP_CHECK(hipMemcpyAsync(P->x.Xw, Xw, P->x.Xw.bytes, hipMemcpyDeviceToDevice, s1));
            if (G->nls) PLSLAM_HIP_CHECK(hipMemcpyAsync(P->x.Lw, Lw, P->x.Lw.bytes, hipMemcpyDeviceToDevice, s1));
            if (P->n_slots) {
                memcpy(P->hx.T, T.data(), P->hx.T.bytes);
                PLSLAM_HIP_CHECK(hipMemcpyAsync(P->x.T, P->hx.T, P->x.T.bytes, hipMemcpyHostToDevice, s1));
            }
            guard.dismiss();                                // (the resident iteration below synchronises the same stream)
            P->state_valid = true;
        }
        rc = plslam_lba_plan_iterate_resident(P, PLSLAM_LBA_COMPAT_GBA, &err_raw);
    }
    if (rc) return rc;
    plslam_lba_blocks B;
    if ((rc = plslam_lba_plan_device_blocks(G->lba, &B))) return rc;
    hipStream_t s = (hipStream_t)B.stream;
    const GbaWorkView& wk = G->wk;
    double hmax = 0.0;
    {
        std::lock_guard<std::mutex> lk(ctx->mu);
        DeviceGuard dg2_(ctx->device);
        StreamSyncOnError guard(s);
        PLSLAM_HIP_CHECK(hipMemcpyAsync(wk.x, x_kf, wk.x.bytes, dev ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, s));
        hipLaunchKernelGGL(k_gba_hmax, dim3(1), dim3(256), 0, s, B.H_pose, nkf, B.H_pt, G->npt, B.H_ls, G->nls, wk.hmax.p);
        PLSLAM_HIP_CHECK(hipGetLastError());
        PLSLAM_HIP_CHECK(hipMemcpyAsync(&hmax, wk.hmax, 8, hipMemcpyDeviceToHost, s));
        PLSLAM_HIP_CHECK(hipStreamSynchronize(s));
        guard.dismiss();
    }
    // int Hmax = 0.0 (:2359): the comparisons run against the truncated running maximum, so Hmax ends as trunc(max |H(i,i)|)
    const double Hmax = std::trunc(hmax);
    double lambda = lambda_lba_lm * Hmax, lambda_k = lambda_lba_k;
    int32_t nsol = 0;
    auto solve = [&](double err_raw_, double err_, bool apply, GbaStats& st) -> int {
        std::lock_guard<std::mutex> lk(ctx->mu);
        DeviceGuard dg3_(ctx->device);
        StreamSyncOnError guard(s);
        int r = gba_solve_enqueue(G, lambda, apply, s);
        if (r) return r;
        PLSLAM_HIP_CHECK(hipMemcpyAsync(&st, wk.stats, sizeof(GbaStats), hipMemcpyDeviceToHost, s));
        PLSLAM_HIP_CHECK(hipStreamSynchronize(s));
        guard.dismiss();
        if (trace) {
            plslam_gba_solve& t = trace[nsol];
            t.lambda = lambda; t.err_raw = err_raw_; t.err = err_; t.dx_norm = std::sqrt(st.dx_sumsq);
            t.n_singular = st.n_singular; t.n_bad_pivots = st.n_bad_pivots; t.accepted = apply ? 1 : 0; t.reserved = 0;
        }
        ++nsol;
        return PLSLAM_OK;
    };
    GbaStats st{};
    double err = err_raw / n_obs_counted;
    if ((rc = solve(err_raw, err, true, st))) return rc;            // the first solve is always applied (:2366-2380)
    double err_prev = err;
    int32_t iters, stop = PLSLAM_GBA_STOP_MAX_ITERS;
    for (iters = 1; iters < max_iters_lba; ++iters) {
        if ((rc = plslam_lba_plan_iterate_resident(G->lba, PLSLAM_LBA_COMPAT_ITER_PASS, &err_raw))) return rc;
        err = err_raw / n_obs_counted;
        if (std::fabs(err - err_prev) < eps || err < eps) { stop = PLSLAM_GBA_STOP_ERR; break; }
        const bool accept = !(err > err_prev);
        if ((rc = solve(err_raw, err, accept, st))) return rc;
        if (accept) lambda *= lambda_k;
        else lambda /= lambda_k;
        if (std::sqrt(st.dx_sumsq) < eps) { stop = PLSLAM_GBA_STOP_DX; break; }
        err_prev = err;
    }
    // the write-back (:2674-2702): T_kf_w = expmap(X) of every optimised keyframe, point3D / line3D = X
    plslam_lba_state ls;
    if ((rc = plslam_lba_plan_device_state(G->lba, &ls))) return rc;
    {
        std::lock_guard<std::mutex> lk(ctx->mu);
        DeviceGuard dg4_(ctx->device);
        StreamSyncOnError guard(s);
        PLSLAM_HIP_CHECK(hipMemcpyAsync(x_kf_out, wk.x, wk.x.bytes, hipMemcpyDeviceToHost, s));
        if (T_out)
            PLSLAM_HIP_CHECK(hipMemcpyAsync(T_out, ls.T_kf_w + 16 * (size_t)n_map, (size_t)nkf * 128, hipMemcpyDeviceToHost, s));
        if (G->npt && Xw_out) PLSLAM_HIP_CHECK(hipMemcpyAsync(Xw_out, ls.Xw, (size_t)G->npt * 24, hipMemcpyDeviceToHost, s));
        if (G->nls && Lw_out) PLSLAM_HIP_CHECK(hipMemcpyAsync(Lw_out, ls.Lw, (size_t)G->nls * 48, hipMemcpyDeviceToHost, s));
        PLSLAM_HIP_CHECK(hipStreamSynchronize(s));
        guard.dismiss();
    }
    if (result) {
        result->iters = iters; result->n_solves = nsol; result->stop_reason = stop; result->reserved = 0;
        result->err = err; result->err_prev = err_prev; result->lambda = lambda; result->hmax = hmax;
    }
    G->optimized = true;
    return PLSLAM_OK;
}

extern "C" {

int plslam_gba_optimize(plslam_gba_plan* G, double lambda_lba_lm, double lambda_lba_k, int32_t max_iters_lba, const double* T_kf_w,
                        const double* x_kf, const double* Xw, const double* Lw, double* x_kf_out, double* T_out, double* Xw_out,
                        double* Lw_out, plslam_gba_solve* trace, plslam_gba_result* result)
{
    PLSLAM_REQUIRE(G && (G->npt == 0 || Xw_out) && (G->nls == 0 || Lw_out), PLSLAM_EINVAL);
    return gba_optimize(G, lambda_lba_lm, lambda_lba_k, max_iters_lba, T_kf_w, x_kf, false, Xw, Lw, x_kf_out, T_out, Xw_out, Lw_out, trace,
                        result);
}

int plslam_gba_optimize_dev(plslam_gba_plan* G, double lambda_lba_lm, double lambda_lba_k, int32_t max_iters_lba, const double* T_kf_w,
                            const double* d_x_kf, const double* d_Xw, const double* d_Lw, double* x_kf_out, double* T_out,
                            plslam_gba_solve* trace, plslam_gba_result* result)
{
    return gba_optimize(G, lambda_lba_lm, lambda_lba_k, max_iters_lba, T_kf_w, d_x_kf, true, d_Xw, d_Lw, x_kf_out, T_out, nullptr, nullptr,
                        trace, result);
}

void plslam_gba_plan_destroy(plslam_gba_plan* G)
{
    if (!G) return;
    {
        std::lock_guard<std::mutex> lk(G->ctx->mu);
        DeviceGuard dg_(G->ctx->device);
        (void)hipStreamSynchronize(G->ctx->stream);
        G->release();
    }
    if (G->lba) plslam_lba_plan_destroy(G->lba);
    delete G;
}

}  // extern "C"
