// lba_assemble_rows.hip -- device-side assembly of the local-BA normal equations in BLOCK form.
//
// The reference adds every observation's blocks into a dense MatrixXd H(N,N) and VectorXd g
// (src/mapHandler.cpp:1410-1429 for points, :1519-1538 for lines) and then takes H.sparseView()
// (:1555).  H has a fixed block structure -- one 6x6 block per optimised keyframe, one 3x3 / 6x6
// block per landmark, one 3x6 / 6x6 cross block per observation -- so this file produces exactly
// those blocks (the Schur-complement-ready layout) and g.  Landmark and cross blocks keep the
// reference's accumulation ORDER (sequential over the landmark's observations in list order), so
// they are bit-exact against the dense accumulation; the keyframe blocks, which sum thousands of
// observations, use a fixed-shape two-level sum (deterministic, equal up to rounding).  No atomics
// (they would make the sums depend on scheduling).
//   K7  k_landmark_blocks<DL>   one lane per landmark: H_ll (DLxDL), g_l (DL) over its observations
//   K8  k_cross_blocks<DL>      one lane per observation: W = J_lm * J_pose^T * w (DLx6)
//   K9  k_pose_partials/_blocks one lane per (keyframe, chunk, entry) then per (keyframe, entry):
//                                H_pp (6x6) and g_p (6) over the keyframe's observations (points
//                                first, then lines, list order; 64-observation chunks)
//   K10 k_weighted_error_*      err = sum r^2 w (fixed-shape two-level tree: deterministic, not sequential)
// The same blocks from rows that never leave the device: lba_plan.hip.  The lists every sum here runs over: lba_lists.hpp.
#include <algorithm>
#include <vector>

#include "common.hpp"
#include "lba_lists.hpp"

using namespace plslam;

namespace plslam {

template <int DL>
__global__ void __launch_bounds__(256)
k_landmark_blocks(const int32_t* __restrict__ lm_ptr, const int32_t* __restrict__ lm_obs, int32_t nlm,
                  const double* __restrict__ Jl, const double* __restrict__ r, const double* __restrict__ w,
                  double* __restrict__ Hll, double* __restrict__ gl)
{
    const int l = blockIdx.x * 256 + threadIdx.x;
    if (l >= nlm) return;
    double H[DL * DL], g[DL];
#pragma unroll
    for (int i = 0; i < DL * DL; ++i) H[i] = 0.0;
#pragma unroll
    for (int i = 0; i < DL; ++i) g[i] = 0.0;
    for (int k = lm_ptr[l]; k < lm_ptr[l + 1]; ++k) {
        const int o = lm_obs[k];
        double J[DL];
#pragma unroll
        for (int a = 0; a < DL; ++a) J[a] = Jl[(size_t)o * DL + a];
        const double rr = r[o], ww = w[o];
#pragma unroll
        for (int a = 0; a < DL; ++a) g[a] += J[a] * rr * ww;
#pragma unroll
        for (int a = 0; a < DL; ++a)
#pragma unroll
            for (int b = 0; b < DL; ++b) H[a * DL + b] += J[a] * J[b] * ww;
    }
#pragma unroll
    for (int i = 0; i < DL * DL; ++i) Hll[(size_t)l * DL * DL + i] = H[i];
#pragma unroll
    for (int i = 0; i < DL; ++i) gl[(size_t)l * DL + i] = g[i];
}

// TRANSPOSED (DL == 6 only): element (a, b) receives Jl[b] * Jp[a] * w -- the block as levMarquardtOptimizationGBA writes
// it for lines (src/mapHandler.cpp:2341-2352 against :1531-1532 of the local BA; a reference defect that callers after
// the reference's GBA numbers reproduce with PLSLAM_LBA_COMPAT_GBA)
template <int DL, bool TRANSPOSED = false>
__global__ void __launch_bounds__(256)
k_cross_blocks(const int32_t* __restrict__ kf_loc, int32_t nobs, const double* __restrict__ Jp,
               const double* __restrict__ Jl, const double* __restrict__ w, double* __restrict__ W)
{
    static_assert(!TRANSPOSED || DL == 6, "only the square line block can be transposed in place");
    const int o = blockIdx.x * 256 + threadIdx.x;
    if (o >= nobs) return;
    const bool opt = kf_loc[o] >= 0;   // kf_loc == -1: the keyframe is not optimised, no cross block
    double P[6];
#pragma unroll
    for (int b = 0; b < 6; ++b) P[b] = Jp[(size_t)o * 6 + b];
    const double ww = w[o];
#pragma unroll
    for (int a = 0; a < DL; ++a) {
        const double ja = Jl[(size_t)o * DL + a];
#pragma unroll
        for (int b = 0; b < 6; ++b) W[TRANSPOSED ? ((size_t)o * 6 + b) * 6 + a : ((size_t)o * DL + a) * 6 + b] = opt ? ja * P[b] * ww : 0.0;
    }
}

// (K9's two-level sum over chunks of POSE_CHUNK observations: lba_lists.hpp)
__global__ void __launch_bounds__(64)
k_pose_partials(const int32_t* __restrict__ kf_ptr, const int32_t* __restrict__ kf_obs, int32_t n_pt_obs,
                const double* __restrict__ Jp_pt, const double* __restrict__ r_pt, const double* __restrict__ w_pt,
                const double* __restrict__ Jp_ls, const double* __restrict__ r_ls, const double* __restrict__ w_ls,
                int32_t max_chunks, double* __restrict__ part /* [nkf][max_chunks][42] */)
{
    const int k = blockIdx.x, c = blockIdx.y, e = threadIdx.x;
    if (e >= 42) return;
    const int beg = kf_ptr[k] + c * POSE_CHUNK;
    const int end = beg + POSE_CHUNK < kf_ptr[k + 1] ? beg + POSE_CHUNK : kf_ptr[k + 1];
    const int a = e < 36 ? e / 6 : e - 36, b = e < 36 ? e % 6 : 0;
    double acc = 0.0;
    // Same terms, same order -- the loads of PB observations are issued together (the loop was a chain of two dependent round
    // trips per observation: 128 of them = 48 us for work that takes microseconds)
    constexpr int PB = 16;
    for (int i0 = beg; i0 < end; i0 += PB) {
        int oo[PB];
        bool pt[PB];
#pragma unroll
        for (int j = 0; j < PB; ++j) {
            const int o = kf_obs[i0 + j < end ? i0 + j : end - 1];      // global observation id: points [0, n_pt_obs), then lines
            pt[j] = o < n_pt_obs;
            oo[j] = pt[j] ? o : o - n_pt_obs;
        }
        double ja[PB], jb[PB], ww[PB];
#pragma unroll
        for (int j = 0; j < PB; ++j) {
            const double* J = (pt[j] ? Jp_pt : Jp_ls) + (size_t)oo[j] * 6;
            ja[j] = J[a];
            jb[j] = e < 36 ? J[b] : (pt[j] ? r_pt : r_ls)[oo[j]];
            ww[j] = (pt[j] ? w_pt : w_ls)[oo[j]];
        }
#pragma unroll
        for (int j = 0; j < PB; ++j)
            if (i0 + j < end) acc += ja[j] * jb[j] * ww[j];
    }
    part[((size_t)k * max_chunks + c) * 42 + e] = acc;   // empty chunks write 0
}

__global__ void __launch_bounds__(64)
k_pose_blocks(const int32_t* __restrict__ kf_ptr, int32_t max_chunks, const double* __restrict__ part,
              double* __restrict__ Hpp, double* __restrict__ gp)
{
    const int k = blockIdx.x, e = threadIdx.x;
    if (e >= 42) return;
    const int nchunks = (kf_ptr[k + 1] - kf_ptr[k] + POSE_CHUNK - 1) / POSE_CHUNK;
    double acc = 0.0;
    constexpr int PB = 8;                       // (same order of additions; the loads in batches)
    for (int c0 = 0; c0 < nchunks; c0 += PB) {
        double v[PB];
#pragma unroll
        for (int j = 0; j < PB; ++j) v[j] = part[((size_t)k * max_chunks + (c0 + j < nchunks ? c0 + j : nchunks - 1)) * 42 + e];
#pragma unroll
        for (int j = 0; j < PB; ++j)
            if (c0 + j < nchunks) acc += v[j];
    }
    if (e < 36) Hpp[(size_t)k * 36 + e] = acc;
    else gp[(size_t)k * 6 + (e - 36)] = acc;
}

// err = sum r^2 w in a fixed shape: ERR_BLOCKS workgroups of 256 lanes -- lane g of all ERR_BLOCKS x 256 sums observations g,
// g + ERR_BLOCKS x 256, ... (points, then lines) in that order, a tree over the workgroup's lanes -> err[1 + block] -- then one
// wave's tree over the ERR_BLOCKS partials -> err[0].  (One workgroup alone read the 0.96 MB of a C3 pass at a single CU's
// 60 GB/s: 58 us with one load per loop trip, 16 us with the loads batched.)
constexpr int ERR_BLOCKS = 64;
__global__ void __launch_bounds__(256)
k_weighted_error_partials(const double* __restrict__ r_pt, const double* __restrict__ w_pt, int32_t n_pt,
                          const double* __restrict__ r_ls, const double* __restrict__ w_ls, int32_t n_ls,
                          double* __restrict__ err)
{
    __shared__ double red[256];
    constexpr int G = ERR_BLOCKS * 256, PB = 4;
    const int g = blockIdx.x * 256 + threadIdx.x;
    double acc = 0.0;
    auto sum = [&](const double* __restrict__ r, const double* __restrict__ w, int32_t n) {
        for (int o0 = g; o0 < n; o0 += G * PB) {
            double rr[PB], ww[PB];
#pragma unroll
            for (int j = 0; j < PB; ++j) {
                const int o = o0 + j * G;
                rr[j] = o < n ? r[o] : 0.0;
                ww[j] = o < n ? w[o] : 0.0;
            }
#pragma unroll
            for (int j = 0; j < PB; ++j)
                if (o0 + j * G < n) acc += rr[j] * rr[j] * ww[j];
        }
    };
    sum(r_pt, w_pt, n_pt);
    sum(r_ls, w_ls, n_ls);
    red[threadIdx.x] = acc;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) err[1 + blockIdx.x] = red[0];
}
__global__ void __launch_bounds__(ERR_BLOCKS)
k_weighted_error_final(double* __restrict__ err)
{
    __shared__ double red[ERR_BLOCKS];
    red[threadIdx.x] = err[1 + threadIdx.x];
    __syncthreads();
    for (int s = ERR_BLOCKS / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) err[0] = red[0];
}

// all pointers on the device; CSR lists as built by build_csr().  Asynchronous on `s`.
struct AssembleDev {
    const int32_t *pt_kf_loc, *ls_kf_loc, *pt_ptr, *pt_ids, *ls_ptr, *ls_ids, *kf_ptr, *kf_ids;
    const double *pt_Jp, *pt_Jl, *pt_r, *pt_w, *ls_Jp, *ls_Jl, *ls_r, *ls_w;
    double *g, *H_pose, *H_pt, *H_ls, *W_pt, *W_ls, *err;
    double* pose_part;      // [nkf][max_chunks][42] scratch
    int32_t max_chunks;     // max over keyframes of ceil(#observations / POSE_CHUNK)
    int32_t transpose_ls_cross = 0;   // PLSLAM_LBA_COMPAT_GBA: the pose x line cross blocks as the reference's GBA writes them
};

static int assemble_on_device(const AssembleDev& a, int32_t nkf, int32_t npt, int32_t nls, int32_t n_pt_obs,
                              int32_t n_ls_obs, hipStream_t s)
{
    // g layout = the reference's X layout: [6*nkf poses | 3*npt points | 6*nls lines]
    if (npt)
        hipLaunchKernelGGL(k_landmark_blocks<3>, dim3((npt + 255) / 256), dim3(256), 0, s, a.pt_ptr, a.pt_ids, npt,
                           a.pt_Jl, a.pt_r, a.pt_w, a.H_pt, a.g + 6 * (size_t)nkf);
    if (nls)
        hipLaunchKernelGGL(k_landmark_blocks<6>, dim3((nls + 255) / 256), dim3(256), 0, s, a.ls_ptr, a.ls_ids, nls,
                           a.ls_Jl, a.ls_r, a.ls_w, a.H_ls, a.g + 6 * (size_t)nkf + 3 * (size_t)npt);
    if (n_pt_obs)
        hipLaunchKernelGGL(k_cross_blocks<3>, dim3((n_pt_obs + 255) / 256), dim3(256), 0, s, a.pt_kf_loc, n_pt_obs,
                           a.pt_Jp, a.pt_Jl, a.pt_w, a.W_pt);
    if (n_ls_obs && !a.transpose_ls_cross)
        hipLaunchKernelGGL(k_cross_blocks<6>, dim3((n_ls_obs + 255) / 256), dim3(256), 0, s, a.ls_kf_loc, n_ls_obs,
                           a.ls_Jp, a.ls_Jl, a.ls_w, a.W_ls);
    if (n_ls_obs && a.transpose_ls_cross)
        hipLaunchKernelGGL((k_cross_blocks<6, true>), dim3((n_ls_obs + 255) / 256), dim3(256), 0, s, a.ls_kf_loc, n_ls_obs,
                           a.ls_Jp, a.ls_Jl, a.ls_w, a.W_ls);
    if (nkf) {
        if (a.max_chunks > 0)
            hipLaunchKernelGGL(k_pose_partials, dim3(nkf, a.max_chunks), dim3(64), 0, s, a.kf_ptr, a.kf_ids, n_pt_obs,
                               a.pt_Jp, a.pt_r, a.pt_w, a.ls_Jp, a.ls_r, a.ls_w, a.max_chunks, a.pose_part);
        hipLaunchKernelGGL(k_pose_blocks, dim3(nkf), dim3(64), 0, s, a.kf_ptr, a.max_chunks, a.pose_part, a.H_pose, a.g);
    }
    hipLaunchKernelGGL(k_weighted_error_partials, dim3(ERR_BLOCKS), dim3(256), 0, s, a.pt_r, a.pt_w, n_pt_obs, a.ls_r, a.ls_w,
                       n_ls_obs, a.err);
    hipLaunchKernelGGL(k_weighted_error_final, dim3(1), dim3(ERR_BLOCKS), 0, s, a.err);
    PLSLAM_HIP_CHECK(hipGetLastError());
    return PLSLAM_OK;
}

}  // namespace plslam

extern "C" int plslam_lba_assemble(plslam_ctx* ctx, int32_t nkf, int32_t npt, int32_t nls,
                                   const int32_t* pt_lm_loc, const int32_t* pt_kf_loc, int32_t n_pt_obs,
                                   const double* pt_J_pose, const double* pt_J_lm, const double* pt_r,
                                   const double* pt_w, const int32_t* ls_lm_loc, const int32_t* ls_kf_loc,
                                   int32_t n_ls_obs, const double* ls_J_pose, const double* ls_J_lm,
                                   const double* ls_r, const double* ls_w, double* g, double* H_pose,
                                   double* H_pt, double* H_ls, double* W_pt, double* W_ls, double* err)
{
    PLSLAM_REQUIRE(ctx && nkf >= 0 && npt >= 0 && nls >= 0 && n_pt_obs >= 0 && n_ls_obs >= 0, PLSLAM_EINVAL);
    PLSLAM_REQUIRE(n_pt_obs == 0 || (pt_lm_loc && pt_kf_loc && pt_J_pose && pt_J_lm && pt_r && pt_w && W_pt), PLSLAM_EINVAL);
    PLSLAM_REQUIRE(n_ls_obs == 0 || (ls_lm_loc && ls_kf_loc && ls_J_pose && ls_J_lm && ls_r && ls_w && W_ls), PLSLAM_EINVAL);
    PLSLAM_REQUIRE(g && err && (nkf == 0 || H_pose) && (npt == 0 || H_pt) && (nls == 0 || H_ls), PLSLAM_EINVAL);
    for (int32_t o = 0; o < n_pt_obs; ++o)
        PLSLAM_REQUIRE(pt_lm_loc[o] >= 0 && pt_lm_loc[o] < npt && pt_kf_loc[o] >= -1 && pt_kf_loc[o] < nkf, PLSLAM_EINVAL);
    for (int32_t o = 0; o < n_ls_obs; ++o)
        PLSLAM_REQUIRE(ls_lm_loc[o] >= 0 && ls_lm_loc[o] < nls && ls_kf_loc[o] >= -1 && ls_kf_loc[o] < nkf, PLSLAM_EINVAL);

    CsrLists L;
    build_csr(pt_lm_loc, pt_kf_loc, n_pt_obs, ls_lm_loc, ls_kf_loc, n_ls_obs, nkf, npt, nls, L);
    std::vector<int32_t>&ptp = L.ptp, &pti = L.pti, &lsp = L.lsp, &lsi = L.lsi, &kfp = L.kfp, &kfi = L.kfi;

    std::lock_guard<std::mutex> lk(ctx->mu);
    DeviceGuard dg_(ctx->device);    // every entry point runs on the context's device, whatever the calling thread's current one
    hipStream_t s = ctx->stream;
    Carver c;
    const size_t np = (size_t)n_pt_obs, nl = (size_t)n_ls_obs;
    const size_t oPJp = c.take(np * 48), oPJl = c.take(np * 24), oPr = c.take(np * 8), oPw = c.take(np * 8),
                 oPk = c.take(np * 4), oLJp = c.take(nl * 48), oLJl = c.take(nl * 48), oLr = c.take(nl * 8),
                 oLw = c.take(nl * 8), oLk = c.take(nl * 4), oPtp = c.take(ptp.size() * 4), oPti = c.take(pti.size() * 4),
                 oLsp = c.take(lsp.size() * 4), oLsi = c.take(lsi.size() * 4), oKfp = c.take(kfp.size() * 4),
                 oKfi = c.take(kfi.size() * 4 + 4);
    const size_t N = 6 * (size_t)nkf + 3 * (size_t)npt + 6 * (size_t)nls;
    Carver co;
    const size_t oG = co.take(N * 8 + 8), oHp = co.take((size_t)nkf * 288 + 8), oHpt = co.take((size_t)npt * 72 + 8),
                 oHls = co.take((size_t)nls * 288 + 8), oWp = co.take(np * 144 + 8), oWl = co.take(nl * 288 + 8),
                 oErr = co.take(8 * (1 + ERR_BLOCKS));
    const int32_t max_chunks = pose_max_chunks(kfp);
    const size_t oPart = co.take((size_t)nkf * (size_t)max_chunks * 42 * 8 + 8);
    int rc;
    if ((rc = ctx->in_a.reserve(c.off + 256))) return rc;
    if ((rc = ctx->out_a.reserve(co.off + 256))) return rc;
    char* di = ctx->in_a.as<char>();
    char* dout = ctx->out_a.as<char>();
    auto up = [&](size_t off, const void* src, size_t bytes) -> int {
        if (bytes) PLSLAM_HIP_CHECK(hipMemcpyAsync(di + off, src, bytes, hipMemcpyHostToDevice, s));
        return PLSLAM_OK;
    };
    if ((rc = up(oPJp, pt_J_pose, np * 48)) || (rc = up(oPJl, pt_J_lm, np * 24)) || (rc = up(oPr, pt_r, np * 8)) ||
        (rc = up(oPw, pt_w, np * 8)) || (rc = up(oPk, pt_kf_loc, np * 4)) || (rc = up(oLJp, ls_J_pose, nl * 48)) ||
        (rc = up(oLJl, ls_J_lm, nl * 48)) || (rc = up(oLr, ls_r, nl * 8)) || (rc = up(oLw, ls_w, nl * 8)) ||
        (rc = up(oLk, ls_kf_loc, nl * 4)) || (rc = up(oPtp, ptp.data(), ptp.size() * 4)) ||
        (rc = up(oPti, pti.data(), pti.size() * 4)) || (rc = up(oLsp, lsp.data(), lsp.size() * 4)) ||
        (rc = up(oLsi, lsi.data(), lsi.size() * 4)) || (rc = up(oKfp, kfp.data(), kfp.size() * 4)) ||
        (rc = up(oKfi, kfi.data(), kfi.size() * 4)))
        return rc;
    AssembleDev a{(int32_t*)(di + oPk), (int32_t*)(di + oLk), (int32_t*)(di + oPtp), (int32_t*)(di + oPti),
                  (int32_t*)(di + oLsp), (int32_t*)(di + oLsi), (int32_t*)(di + oKfp), (int32_t*)(di + oKfi),
                  (double*)(di + oPJp), (double*)(di + oPJl), (double*)(di + oPr), (double*)(di + oPw),
                  (double*)(di + oLJp), (double*)(di + oLJl), (double*)(di + oLr), (double*)(di + oLw),
                  (double*)(dout + oG), (double*)(dout + oHp), (double*)(dout + oHpt), (double*)(dout + oHls),
                  (double*)(dout + oWp), (double*)(dout + oWl), (double*)(dout + oErr), (double*)(dout + oPart),
                  max_chunks};
    if ((rc = assemble_on_device(a, nkf, npt, nls, n_pt_obs, n_ls_obs, s))) return rc;
    auto down = [&](void* dst, size_t off, size_t bytes) -> int {
        if (bytes) PLSLAM_HIP_CHECK(hipMemcpyAsync(dst, dout + off, bytes, hipMemcpyDeviceToHost, s));
        return PLSLAM_OK;
    };
    if ((rc = down(g, oG, N * 8)) || (rc = down(H_pose, oHp, (size_t)nkf * 288)) || (rc = down(H_pt, oHpt, (size_t)npt * 72)) ||
        (rc = down(H_ls, oHls, (size_t)nls * 288)) || (rc = down(W_pt, oWp, np * 144)) || (rc = down(W_ls, oWl, nl * 288)) ||
        (rc = down(err, oErr, 8)))
        return rc;
    PLSLAM_HIP_CHECK(hipStreamSynchronize(s));
    return PLSLAM_OK;
}
