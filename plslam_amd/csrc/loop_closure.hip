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
//
// The host side: lc_plan.hpp decides everything that needs no device (checks, match problems, records, the layouts of the
// staged blocks); what is left here reserves, copies, launches and waits.
#include <cfloat>
#include <new>
#include <vector>

#include "match_plan.hpp"   // (common.hpp first: lc_plan.hpp's checks then report through its PLSLAM_REQUIRE)

#include "dense6_dev.hpp"
#include "lc_plan.hpp"
#include "pose_gn_dev.hpp"
#include "se3_dev.hpp"

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

constexpr int LC_THREADS = 256;
constexpr int LC_RED = 2 * GN_TERMS;     // points' then lines' partial sums per lane

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

// ---- the host side ----------------------------------------------------------------------------------------------------------
// the two launchers, on ctx->stream.  K54's records come from pageable memory: the copy call stages them before it returns
int launch_k25(plslam_ctx* ctx, const LcArgs& a)
{
    hipLaunchKernelGGL(k_loop_closure, dim3(1), dim3(LC_THREADS), 0, ctx->stream, a);
    PLSLAM_HIP_CHECK(hipGetLastError());
    return PLSLAM_OK;
}

int launch_k54(plslam_ctx* ctx, LcArgs* d_tab, const LcArgs* h_tab, int32_t B, const int32_t* pt_off, const int32_t* ls_off)
{
    PLSLAM_HIP_CHECK(hipMemcpyAsync(d_tab, h_tab, (size_t)B * sizeof(LcArgs), hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(k_loop_closure_batched, dim3((unsigned)B), dim3(LC_THREADS), 0, ctx->stream, d_tab, pt_off, ls_off);
    PLSLAM_HIP_CHECK(hipGetLastError());
    return PLSLAM_OK;
}

// one pair (device arrays): its match problems through the context's plan (ctx->lc_plan, tables in ctx->lc_tab), then K25 with
// the record by value
int enqueue_verify(plslam_ctx* ctx, const plslam_lc_params* p, const plslam_lc_keyframe* k0, const plslam_lc_keyframe* k1,
                   const LcOut& out)
{
    int rc;
    const LcTables T = lc_tables(k0, 1);
    if ((rc = ctx->lc_tab.reserve(T.bytes))) return rc;
    plslam_match_problem pr[2];
    LcArgs a;
    const int32_t np = lc_plan_pairs(p, k0, k1, 1, T, ctx->lc_tab.p, out, pr, &a);
    if (np && (rc = match_problems_lc(ctx, pr, np))) return rc;
    return launch_k25(ctx, a);
}

// B pairs (device arrays): their match problems as ONE plan, rebuilt only when the list changed, then K54 over the B records
int enqueue_batch(plslam_lc_batch* bt, const plslam_lc_keyframe* kf0, const plslam_lc_keyframe* kf1, int32_t B, const LcOut& out)
{
    int rc;
    plslam_ctx* ctx = bt->ctx;
    const LcTables T = lc_tables(kf0, B);
    if ((rc = bt->tab.reserve(T.bytes))) return rc;
    if ((rc = bt->args.reserve((size_t)B * sizeof(LcArgs)))) return rc;
    bt->probs.resize(2 * (size_t)B);
    bt->h_args.resize((size_t)B);
    bt->probs.resize((size_t)lc_plan_pairs(&bt->p, kf0, kf1, B, T, bt->tab.p, out, bt->probs.data(), bt->h_args.data()));
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
    return launch_k54(ctx, bt->args.as<LcArgs>(), bt->h_args.data(), B, nullptr, nullptr);
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

// The host-pointer forms stage through four buffers (the single forms through the context's, the batch through its own):
// prepare(h, d, od) fills the in_bytes of the page-locked input image at h -- d: where its copy will be on the device, od: the
// device's output block --, ONE upload, enqueue(), ONE download of the out_bytes into st.pin_out, one synchronisation.
struct LcStage { HostBuf &pin_in, &pin_out; DevBuf &in, &out; };
template <class Prepare, class Enqueue>
int staged(plslam_ctx* ctx, LcStage st, size_t in_bytes, size_t out_bytes, Prepare prepare, Enqueue enqueue)
{
    int rc;
    hipStream_t s = ctx->stream;
    StreamSyncOnError sync_on_error(s);
    if ((rc = st.pin_in.reserve(in_bytes + 256)) || (rc = st.in.reserve(in_bytes + 256))) return rc;
    if ((rc = st.pin_out.reserve(out_bytes)) || (rc = st.out.reserve(out_bytes))) return rc;
    prepare(st.pin_in.as<char>(), st.in.as<char>(), st.out.as<char>());
    if (in_bytes) PLSLAM_HIP_CHECK(hipMemcpyAsync(st.in.p, st.pin_in.p, in_bytes, hipMemcpyHostToDevice, s));
    if ((rc = enqueue())) return rc;
    PLSLAM_HIP_CHECK(hipMemcpyAsync(st.pin_out.p, st.out.p, out_bytes, hipMemcpyDeviceToHost, s));
    PLSLAM_HIP_CHECK(hipStreamSynchronize(s));
    sync_on_error.dismiss();
    return PLSLAM_OK;
}

// B pairs of host records: one image of every distinct record up, enqueue(kf0 and kf1 of the device records, the output bases),
// the output block down and scattered into the caller's arrays.  D: where the 2 B device records are kept
template <class Enqueue>
int verify_host(plslam_ctx* ctx, LcStage st, const plslam_lc_keyframe* kf0, const plslam_lc_keyframe* kf1, int32_t B,
                std::vector<plslam_lc_keyframe>& D, Enqueue enqueue, plslam_lc_result* results, int32_t* pt_corr,
                uint8_t* pt_inlier, int32_t* ls_corr, uint8_t* ls_inlier)
{
    LcKfImage img;
    lc_kf_layout(kf0, kf1, B, img);
    const LcOutBlock ob = lc_out_block(kf0, B);
    D.assign(2 * (size_t)B, plslam_lc_keyframe{});
    LcOut out{};
    const int rc = staged(
        ctx, st, img.bytes, ob.bytes,
        [&](char* h, char* d, char* od) {
            lc_kf_fill(kf0, kf1, img, h);
            lc_kf_device(kf0, kf1, img, d, D.data());
            out = lc_out_bases(ob, od);
        },
        [&] { return enqueue(D.data(), D.data() + B, out); });
    if (rc == PLSLAM_OK) lc_out_scatter(ob, st.pin_out.as<char>(), kf0, B, results, pt_corr, pt_inlier, ls_corr, ls_inlier);
    return rc;
}

// plslam_relpose_robust_gn's input image: the caller's four arrays
struct GnImage { Arr<double> P, pl, sPeP, le; size_t bytes; };
GnImage gn_image(char* base, size_t np, size_t nl)
{
    ArrCarver c{base};
    GnImage I;
    I.P = c.take<double>(np * 24); I.pl = c.take<double>(np * 16); I.sPeP = c.take<double>(nl * 48); I.le = c.take<double>(nl * 24);
    I.bytes = c.size();
    return I;
}

}  // namespace

// plslam_relpose_robust_gn_batched_dev behind its checks and its lock (common.hpp; the tracker, track.hip, runs K54 through
// it): the B records, K54 behind `us`.  The caller holds ctx->mu and has selected the context's device.
int lc_relpose_batched_unlocked(plslam_ctx* ctx, const plslam_lc_params* params, const double* P, const double* pl_obs,
                                const int32_t* pt_off, const double* sPeP, const double* le_obs, const int32_t* ls_off, int32_t B,
                                plslam_lc_result* results, uint8_t* pt_inlier, uint8_t* ls_inlier, hipStream_t us)
{
    int rc;
    const size_t bytes = (size_t)B * sizeof(LcArgs);
    if ((rc = ctx->lc_args.reserve(bytes))) return rc;
    ctx->lc_args_h.resize(bytes);
    LcArgs* h = reinterpret_cast<LcArgs*>(ctx->lc_args_h.data());
    LcArgs a;                   // K54 takes the counts from pt_off / ls_off; no correspondence rows: row k is (k, k)
    lc_identity_args(a, params, P, pl_obs, 0, sPeP, le_obs, 0, LcOut{nullptr, nullptr, pt_inlier, nullptr, ls_inlier});
    for (int32_t b = 0; b < B; ++b) {
        h[b] = a;
        h[b].res = results + b;
    }
    if ((rc = fence_enter(ctx, us))) return rc;
    if ((rc = launch_k54(ctx, ctx->lc_args.as<LcArgs>(), h, B, pt_off, ls_off))) return rc;
    return fence_leave(ctx, us);
}

}  // namespace plslam

extern "C" {

int plslam_loop_closure_verify(plslam_ctx* ctx, const plslam_lc_params* params, const plslam_lc_keyframe* kf0,
                               const plslam_lc_keyframe* kf1, plslam_lc_result* result, int32_t* pt_corr, uint8_t* pt_inlier,
                               int32_t* ls_corr, uint8_t* ls_inlier)
{
    using namespace plslam;
    int rc;
    PLSLAM_REQUIRE(ctx && result, PLSLAM_EINVAL);
    if ((rc = lc_check_params(params)) || (rc = lc_check_kf(kf0)) || (rc = lc_check_kf(kf1))) return rc;
    std::lock_guard<std::mutex> lk(ctx->mu);
    DeviceGuard guard(ctx->device);
    std::vector<plslam_lc_keyframe> D;
    return verify_host(
        ctx, LcStage{ctx->pin_in, ctx->pin_out, ctx->lc_in, ctx->lc_out}, kf0, kf1, 1, D,
        [&](const plslam_lc_keyframe* d0, const plslam_lc_keyframe* d1, const LcOut& out) { return enqueue_verify(ctx, params, d0, d1, out); },
        result, pt_corr, pt_inlier, ls_corr, ls_inlier);
}

int plslam_loop_closure_verify_dev(plslam_ctx* ctx, const plslam_lc_params* params, const plslam_lc_keyframe* kf0,
                                   const plslam_lc_keyframe* kf1, plslam_lc_result* result, int32_t* pt_corr,
                                   uint8_t* pt_inlier, int32_t* ls_corr, uint8_t* ls_inlier, void* stream)
{
    using namespace plslam;
    int rc;
    PLSLAM_REQUIRE(ctx && result, PLSLAM_EINVAL);
    if ((rc = lc_check_params(params)) || (rc = lc_check_kf(kf0)) || (rc = lc_check_kf(kf1))) return rc;
    PLSLAM_REQUIRE(kf0->n_pt == 0 || (pt_corr && pt_inlier), PLSLAM_EINVAL);
    PLSLAM_REQUIRE(kf0->n_ls == 0 || (ls_corr && ls_inlier), PLSLAM_EINVAL);
    std::lock_guard<std::mutex> lk(ctx->mu);
    DeviceGuard guard(ctx->device);
    hipStream_t us = static_cast<hipStream_t>(stream);
    if ((rc = fence_enter(ctx, us))) return rc;
    if ((rc = enqueue_verify(ctx, params, kf0, kf1, LcOut{result, pt_corr, pt_inlier, ls_corr, ls_inlier}))) return rc;
    return fence_leave(ctx, us);
}

int plslam_relpose_robust_gn(plslam_ctx* ctx, const plslam_lc_params* params, const double* P, const double* pl_obs,
                             int32_t npt, const double* sPeP, const double* le_obs, int32_t nls, plslam_lc_result* result,
                             uint8_t* pt_inlier, uint8_t* ls_inlier)
{
    using namespace plslam;
    int rc;
    PLSLAM_REQUIRE(ctx && result && npt >= 0 && nls >= 0, PLSLAM_EINVAL);
    if ((rc = lc_check_params(params))) return rc;
    PLSLAM_REQUIRE(npt == 0 || (P && pl_obs), PLSLAM_EINVAL);
    PLSLAM_REQUIRE(nls == 0 || (sPeP && le_obs), PLSLAM_EINVAL);
    PLSLAM_REQUIRE(npt <= PLSLAM_LC_MAX_FEATURES && nls <= PLSLAM_LC_MAX_FEATURES, PLSLAM_ERANGE);
    std::lock_guard<std::mutex> lk(ctx->mu);
    DeviceGuard guard(ctx->device);
    const size_t np = (size_t)npt, nl = (size_t)nls;
    plslam_lc_keyframe rows{};               // the output block of ONE problem with npt / nls rows (all of them common: (k, k))
    rows.n_pt = npt; rows.n_ls = nls;
    const LcOutBlock ob = lc_out_block(&rows, 1);
    LcArgs a;
    rc = staged(
        ctx, LcStage{ctx->pin_in, ctx->pin_out, ctx->lc_in, ctx->lc_out}, gn_image(nullptr, np, nl).bytes, ob.bytes,
        [&](char* h, char* d, char* od) {
            const GnImage H = gn_image(h, np, nl), I = gn_image(d, np, nl);
            if (np) { memcpy(H.P, P, H.P.bytes); memcpy(H.pl, pl_obs, H.pl.bytes); }
            if (nl) { memcpy(H.sPeP, sPeP, H.sPeP.bytes); memcpy(H.le, le_obs, H.le.bytes); }
            lc_identity_args(a, params, I.P, I.pl, npt, I.sPeP, I.le, nls, lc_out_bases(ob, od));
        },
        [&] { return launch_k25(ctx, a); });
    if (rc == PLSLAM_OK) lc_out_scatter(ob, ctx->pin_out.as<char>(), &rows, 1, result, nullptr, pt_inlier, nullptr, ls_inlier);
    return rc;
}

int plslam_lc_batch_create(plslam_ctx* ctx, const plslam_lc_params* params, int32_t max_pairs, plslam_lc_batch** out)
{
    using namespace plslam;
    int rc;
    PLSLAM_REQUIRE(ctx && out, PLSLAM_EINVAL);
    *out = nullptr;
    if ((rc = lc_check_params(params))) return rc;
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
    if ((rc = lc_check_batch(batch ? &batch->max_pairs : nullptr, kf0, kf1, B))) return rc;
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
    if ((rc = enqueue_batch(batch, kf0, kf1, B, LcOut{results, pt_corr, pt_inlier, ls_corr, ls_inlier}))) return rc;
    return fence_leave(ctx, us);
}

int plslam_lc_batch_verify(plslam_lc_batch* batch, const plslam_lc_keyframe* kf0, const plslam_lc_keyframe* kf1, int32_t B,
                           plslam_lc_result* results, int32_t* pt_corr, uint8_t* pt_inlier, int32_t* ls_corr, uint8_t* ls_inlier)
{
    using namespace plslam;
    int rc;
    if ((rc = lc_check_batch(batch ? &batch->max_pairs : nullptr, kf0, kf1, B))) return rc;
    if (B == 0) return PLSLAM_OK;
    PLSLAM_REQUIRE(results != nullptr, PLSLAM_EINVAL);
    plslam_ctx* ctx = batch->ctx;
    std::lock_guard<std::mutex> lk(ctx->mu);
    DeviceGuard guard(ctx->device);
    return verify_host(
        ctx, LcStage{batch->pin_in, batch->pin_out, batch->in, batch->out}, kf0, kf1, B, batch->d_kf,
        [&](const plslam_lc_keyframe* d0, const plslam_lc_keyframe* d1, const LcOut& out) { return enqueue_batch(batch, d0, d1, B, out); },
        results, pt_corr, pt_inlier, ls_corr, ls_inlier);
}

int plslam_relpose_robust_gn_batched_dev(plslam_ctx* ctx, const plslam_lc_params* params, const double* P, const double* pl_obs,
                                         const int32_t* pt_off, const double* sPeP, const double* le_obs, const int32_t* ls_off,
                                         int32_t B, plslam_lc_result* results, uint8_t* pt_inlier, uint8_t* ls_inlier, void* stream)
{
    using namespace plslam;
    int rc;
    PLSLAM_REQUIRE(ctx != nullptr, PLSLAM_EINVAL);
    if ((rc = lc_check_params(params))) return rc;
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
    return lc_relpose_batched_unlocked(ctx, params, P, pl_obs, pt_off, sPeP, le_obs, ls_off, B, results, pt_inlier, ls_inlier,
                                       static_cast<hipStream_t>(stream));
}

}  // extern "C"
