// lba_plan.hip -- the LBA plan: the observation lists on the device once, then every iteration of the LM loop from the state
// (poses, landmarks) to the blocks of the normal equations without leaving the device.  The plan object: lba_plan.hpp.
//
// The iteration of an LBA plan in THREE launches (round 4; round 3: ten launches of 4-13 us each, i.e. launch granularity):
//   F1 k_lba_rows_cross   one lane per observation (points, then lines): the row (K3 / K4), its cross block (K8) from the
//                         values still in registers, and the workgroup's share of err = sum r^2 w
//   F2 k_lba_blocks       workgroups [0, nb3): point landmark blocks (K7<3>); [.., +nb6): line landmark blocks (K7<6>); the
//                         rest: the keyframes' chunk partials (K9, four 64-lane chunks per workgroup)
//   F3 k_lba_finish       workgroup k < nkf: keyframe k's blocks from its chunk partials (K9); workgroup nkf: err
// Every block keeps the summation ORDER of the separate kernels (landmark and cross blocks: the reference's, bit for bit;
// keyframe blocks: chunks of 64 observations in list order, then the chunks in order); err is the sum of the row workgroups'
// trees in workgroup order -- a fixed shape, deterministic, equal to the reference's sequential sum up to rounding.
#include <cstring>
#include <new>
#include <utility>

#include "lba_plan.hpp"

using namespace plslam;

namespace plslam {

struct LbaIterArgs {
    CamD K;
    double th;
    int32_t compat_iter, transpose_ls_cross;
    const double *T, *Xw, *Lw, *uv, *lobs;
    const int32_t *pt_lm, *pt_slot, *pt_kf_loc, *ls_lm, *ls_slot, *ls_kf_loc;
    int32_t np, nl, nbp, nbl;                 // observations and row workgroups (points, lines)
    int32_t n_slots;                          // pose slots behind T (the first of them ride in LDS: pose12_cached)
    double *pJp, *pJl, *pr, *pw, *lJp, *lJl, *lr, *lw, *Wp, *Wl, *err_part;   // err_part[nbp + nbl]
};

__device__ __forceinline__ void lba_rows_cross_wg(const LbaIterArgs& A)
{
    // (a slab holds a wave's 64 rows of up to 18 doubles: the cross blocks leave through it too -- written lane by lane they were 18 /
    // 36 instructions of 64 scattered 8-byte stores each)
    __shared__ __attribute__((aligned(16))) double slabs[4][64 * 18];
    __shared__ double red[256];
    __shared__ PoseCache<POSE_LINES> poses;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const bool lines = (int)blockIdx.x >= A.nbp;
    const int nobs = lines ? A.nl : A.np;
    const int o = (lines ? (int)blockIdx.x - A.nbp : (int)blockIdx.x) * 256 + (int)threadIdx.x;
    const int o0 = o - lane;
    // every load a row needs goes out before the workgroup's one barrier (lba_rows_dev.hpp: pose_cache_fill): slot number, landmark
    // index, observation, the pose matrices' copy into LDS, the landmark
    double T12[12], LM6[6], ob3[3];
    {
        const int oq = o < nobs ? o : nobs - 1;
        const int32_t slot = (lines ? A.ls_slot : A.pt_slot)[oq];
        const size_t l0 = (size_t)(lines ? A.ls_lm : A.pt_lm)[oq];
        if (!lines) {
            const double2 ob = reinterpret_cast<const double2*>(A.uv)[oq];
            ob3[0] = ob.x; ob3[1] = ob.y; ob3[2] = 0.0;
        } else {
            load3(A.lobs + 3 * (size_t)oq, ob3);
        }
        pose_cache_fill(poses, A.T, A.n_slots);
        if (!lines || A.compat_iter) {                       // (the iteration pass's quirk: both end points = the 3 doubles at 3 l0)
            double P3[3];
            load3((lines ? A.Lw : A.Xw) + 3 * l0, P3);
#pragma unroll
            for (int a = 0; a < 3; ++a) LM6[a] = LM6[3 + a] = P3[a];
        } else {
            load6(A.Lw + 6 * l0, LM6);
        }
        pose12_take(poses, A.T, A.n_slots, slot, T12);       // (every wave of the workgroup: a barrier inside)
    }
    double e2w = 0.0;
    if (o0 < nobs) {                                         // (wave-uniform)
        const int valid = nobs - o0 < 64 ? nobs - o0 : 64;
        const int oc = o < nobs ? o : nobs - 1;              // tail lanes recompute the last row
        double nrm, wgt;
        if (!lines) {
            double out6[6], out3[3];
            double2 ob;
            ob.x = ob3[0]; ob.y = ob3[1];
            point_row(A.K, A.th, T12, LM6, ob, out6, out3, nrm, wgt);
            wave_store_rows<6>(A.pJp + 6 * (size_t)o0, out6, slabs[wave], lane, valid);
            wave_store_rows<3>(A.pJl + 3 * (size_t)o0, out3, slabs[wave], lane, valid);
            if (o < nobs) {
                A.pr[o] = nrm;
                A.pw[o] = wgt;
            }
            const bool opt = A.pt_kf_loc[oc] >= 0;             // kf_loc == -1: the keyframe is not optimised, no cross block
            double w18[18];
#pragma unroll
            for (int a = 0; a < 3; ++a)
#pragma unroll
                for (int b = 0; b < 6; ++b) w18[a * 6 + b] = opt ? out3[a] * out6[b] * wgt : 0.0;
            wave_store_rows<18>(A.Wp + 18 * (size_t)o0, w18, slabs[wave], lane, valid);
        } else {
            double outl[6], outp[6];
            // (the iteration pass's line rows take a literal for homogTh, :1698 - :1741; its point rows do not, :1616 - :1637)
            line_row(A.K, A.compat_iter ? 0.0000001 : A.th, T12, LM6, LM6 + 3, ob3[0], ob3[1], ob3[2], outl, outp, nrm, wgt);
            wave_store_rows<6>(A.lJl + 6 * (size_t)o0, outl, slabs[wave], lane, valid);
            wave_store_rows<6>(A.lJp + 6 * (size_t)o0, outp, slabs[wave], lane, valid);
            if (o < nobs) {
                A.lr[o] = nrm;
                A.lw[o] = wgt;
            }
            const bool opt = A.ls_kf_loc[oc] >= 0;
#pragma unroll
            for (int half = 0; half < 2; ++half) {             // rows 0-2, then rows 3-5 of the 6 x 6 block
                double w18[18];
#pragma unroll
                for (int a = 0; a < 3; ++a)
#pragma unroll
                    for (int b = 0; b < 6; ++b) {
                        const int r = 3 * half + a;            // (transposed: entry (r, b) of what is stored is outl[b] * outp[r])
                        w18[a * 6 + b] = !opt ? 0.0 : A.transpose_ls_cross ? outl[b] * outp[r] * wgt : outl[r] * outp[b] * wgt;
                    }
                wave_store_row_parts<18, 36>(A.Wl + 36 * (size_t)o0 + 18 * half, w18, slabs[wave], lane, valid);
            }
        }
        if (o < nobs) e2w = nrm * nrm * wgt;
    }
    red[threadIdx.x] = e2w;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) A.err_part[blockIdx.x] = red[0];
}
__global__ void __launch_bounds__(256)
k_lba_rows_cross(const LbaIterArgs A)
{
    lba_rows_cross_wg(A);
}
// plslam_lba_plan_optimize_dev (lba_lm_dev.hip): the same pass behind the loop's stop word -- a pass enqueued behind the stop changes nothing
__global__ void __launch_bounds__(256)
k_lba_rows_cross_lm(const LbaIterArgs A, const LbaLmCtl* __restrict__ ctl)
{
    if (ctl->stop != LM_RUNNING) return;
    lba_rows_cross_wg(A);
}

// One lane per landmark, 64 landmarks per workgroup (a wave: the 2 000 lines of C3 were 8 workgroups of 256 on 8 CUs).  The blocks
// leave through an LDS slab in runs (wave_store_rows): a lane storing its own 36 doubles word by word is 36 instructions of 64
// scattered 8-byte stores.  Lanes past the last landmark replay it and store nothing.
template <int DL>
__device__ __forceinline__ void landmark_block(int l0 /* the wave's first landmark */, int32_t nlm, const int32_t* __restrict__ lm_ptr,
                                               const int32_t* __restrict__ lm_obs, const double* __restrict__ Jl,
                                               const double* __restrict__ r, const double* __restrict__ w, double* __restrict__ Hll,
                                               double* __restrict__ gl, double* __restrict__ slab /* [64 * DL * DL] */, double lambda,
                                               double* __restrict__ Vinv, double* __restrict__ t, int32_t* __restrict__ nsing)
{
    const int lane = threadIdx.x;
    const int valid = nlm - l0 < 64 ? nlm - l0 : 64;
    const bool live = lane < valid;
    const int l = live ? l0 + lane : nlm - 1;
    double H[DL * DL], g[DL];
#pragma unroll
    for (int i = 0; i < DL * DL; ++i) H[i] = 0.0;
#pragma unroll
    for (int i = 0; i < DL; ++i) g[i] = 0.0;
    // (the observations go PB at a time: their ids in one round trip, their rows in a second -- one by one a landmark's list was a
    // chain of two dependent round trips per observation; the sums keep their order)
    constexpr int PB = DL == 3 ? 8 : 4;
    const int kbeg = lm_ptr[l], kend = lm_ptr[l + 1];
    for (int k0 = kbeg; k0 < kend; k0 += PB) {
        int oo[PB];
#pragma unroll
        for (int u = 0; u < PB; ++u) oo[u] = lm_obs[k0 + u < kend ? k0 + u : kend - 1];
        double J[PB][DL], rr[PB], ww[PB];
#pragma unroll
        for (int u = 0; u < PB; ++u) {
#pragma unroll
            for (int a = 0; a < DL; ++a) J[u][a] = Jl[(size_t)oo[u] * DL + a];
            rr[u] = r[oo[u]];
            ww[u] = w[oo[u]];
        }
#pragma unroll
        for (int u = 0; u < PB; ++u) {
            if (k0 + u < kend) {
#pragma unroll
                for (int a = 0; a < DL; ++a) g[a] += J[u][a] * rr[u] * ww[u];
#pragma unroll
                for (int a = 0; a < DL; ++a)
#pragma unroll
                    for (int b = 0; b < DL; ++b) H[a * DL + b] += J[u][a] * J[u][b] * ww[u];
            }
        }
    }
    wave_store_rows<DL * DL>(Hll + (size_t)l0 * DL * DL, H, slab, lane, valid);
    wave_store_rows<DL>(gl + (size_t)l0 * DL, g, slab, lane, valid);
    // plslam_lba_plan_iterate_schur: lambda is known when the blocks are built, so the landmark's damped inverse and t = Vinv g
    // (K20's work) follow from the registers -- the same arithmetic on the same words, one launch and one round trip less
    if (Vinv) {                                                  // (kernel argument: uniform)
        double Vo[DL * DL], to[DL];
        schur_landmark<DL>(H, g, 0, lambda, Vo, to, live ? nsing : nullptr);
        wave_store_rows<DL * DL>(Vinv + (size_t)l0 * DL * DL, Vo, slab, lane, valid);
        wave_store_rows<DL>(t + (size_t)l0 * DL, to, slab, lane, valid);
    }
}

__device__ __forceinline__ void lba_blocks_wg(const LbaBlockArgs& A)
{
    __shared__ __attribute__((aligned(16))) double slab[64 * 36];
    const int b = blockIdx.x;
    // (knock-out builds at C3: the launch is 16.3 us; points alone 5.1, lines alone 8.9, the chunk partials alone 13.9 -- the launch's
    // critical path, and not a matter of round trips: 16 / 32 observations in flight gave 16.3 / 16.1 us)
    if (b < A.nb3) {                                   // (64 landmarks: the workgroup's first wave; the others leave)
        if (threadIdx.x >= 64) return;
        landmark_block<3>(b * 64, A.npt, A.pt_ptr, A.pt_ids, A.pJl, A.pr, A.pw, A.H_pt, A.g_pt, slab, A.lambda, A.Vp, A.tp, A.nsing);
    } else if (b < A.nb3 + A.nb6) {
        if (threadIdx.x >= 64) return;
        landmark_block<6>((b - A.nb3) * 64, A.nls, A.ls_ptr, A.ls_ids, A.lJl, A.lr, A.lw, A.H_ls, A.g_ls, slab, A.lambda, A.Vl, A.tl,
                          A.nsing);
    } else {
        // chunk partials of the keyframes (K9): item = keyframe * max_chunks + chunk, one wave per item, lane e < 42 an entry
        // (the item is the wave's: said so, the observation ids are scalar loads)
        const int item = __builtin_amdgcn_readfirstlane((b - A.nb3 - A.nb6) * 4 + ((int)threadIdx.x >> 6)), e = (int)threadIdx.x & 63;
        if (item >= A.nkf * A.max_chunks || e >= 42) return;
        const int k = item / A.max_chunks, c = item - k * A.max_chunks;
        const int beg = A.kf_ptr[k] + c * POSE_CHUNK;
        const int end = beg + POSE_CHUNK < A.kf_ptr[k + 1] ? beg + POSE_CHUNK : A.kf_ptr[k + 1];
        const int a = e < 36 ? e / 6 : e - 36, bb = e < 36 ? e % 6 : 0;
        double acc = 0.0;
        constexpr int PB = 32;   // (observations whose loads are in flight together: 32 = two round trips per 64-observation chunk; 16 was four, and this part of the launch its critical path: 13.9 us alone)
        for (int i0 = beg; i0 < end; i0 += PB) {
            int oo[PB];
            bool pt[PB];
#pragma unroll
            for (int j = 0; j < PB; ++j) {
                const int o = A.kf_ids[i0 + j < end ? i0 + j : end - 1];
                pt[j] = o < A.np;
                oo[j] = pt[j] ? o : o - A.np;
            }
            double ja[PB], jb[PB], ww[PB];
#pragma unroll
            for (int j = 0; j < PB; ++j) {
                const double* J = (pt[j] ? A.pJp : A.lJp) + (size_t)oo[j] * 6;
                ja[j] = J[a];
                jb[j] = e < 36 ? J[bb] : (pt[j] ? A.pr : A.lr)[oo[j]];
                ww[j] = (pt[j] ? A.pw : A.lw)[oo[j]];
            }
#pragma unroll
            for (int j = 0; j < PB; ++j)
                if (i0 + j < end) acc += ja[j] * jb[j] * ww[j];
        }
        A.pose_part[((size_t)k * A.max_chunks + c) * 42 + e] = acc;   // empty chunks write 0
    }
}

__global__ void __launch_bounds__(256)
k_lba_blocks(const LbaBlockArgs A)
{
    lba_blocks_wg(A);
}
// ... with the damping read from the loop's control block (the landmark inverses of the fused form)
__global__ void __launch_bounds__(256)
k_lba_blocks_lm(LbaBlockArgs A, const LbaLmCtl* __restrict__ ctl)
{
    if (ctl->stop != LM_RUNNING) return;
    A.lambda = ctl->lambda;
    lba_blocks_wg(A);
}

__global__ void __launch_bounds__(256)
k_lba_finish(const LbaBlockArgs A)
{
    __shared__ double red[256];
    lba_finish_wg<256>(A, (int)blockIdx.x, red);
}
__global__ void __launch_bounds__(256)
k_lba_finish_lm(const LbaBlockArgs A, const LbaLmCtl* __restrict__ ctl)
{
    __shared__ double red[256];
    if (ctl->stop != LM_RUNNING) return;
    lba_finish_wg<256>(A, (int)blockIdx.x, red);
}

LbaBlockArgs lba_block_args(plslam_lba_plan* P)
{
    const LbaStatView& S = P->st; const LbaRowsView& R = P->rw; const LbaOutView& O = P->o;
    const size_t N6 = 6 * (size_t)P->nkf;
    LbaBlockArgs B{};
    B.pt_ptr = S.pt_ptr; B.pt_ids = S.pt_ids; B.ls_ptr = S.ls_ptr; B.ls_ids = S.ls_ids; B.kf_ptr = S.kf_ptr; B.kf_ids = S.kf_ids;
    B.pJp = R.pJp; B.pJl = R.pJl; B.pr = R.pr; B.pw = R.pw; B.lJp = R.lJp; B.lJl = R.lJl; B.lr = R.lr; B.lw = R.lw;
    B.H_pt = O.H_pt; B.g_pt = O.g + N6; B.H_ls = O.H_ls; B.g_ls = O.g + N6 + 3 * (size_t)P->npt;
    B.pose_part = O.pose_part; B.H_pose = O.H_pose; B.g_pose = O.g;
    B.err = O.err; B.err_part = O.err_part;
    B.npt = P->npt; B.nls = P->nls; B.nkf = P->nkf; B.np = P->np;
    B.nb3 = (P->npt + 63) / 64; B.nb6 = (P->nls + 63) / 64; B.max_chunks = P->max_chunks;
    B.nerr = (P->np + 255) / 256 + (P->nl + 255) / 256;
    return B;
}

int lba_plan_enqueue(plslam_lba_plan* P, const double* T_kf_w, const double* Xw, const double* Lw, int compat_flags, bool upload,
                     double fused_lambda, const LbaLmCtl* ctl)
{
    plslam_ctx* ctx = P->ctx;
    hipStream_t s = ctx->stream;
    const LbaStatView& S = P->st; const LbaRowsView& R = P->rw; const LbaOutView& O = P->o;
    const LbaStateView &X = P->x, &HX = P->hx;
    if (upload) {
        // (the page-locked image is rewritten per call: the previous call's copy has completed -- every caller synchronises
        // the stream before it returns)
        // (a caller that keeps its state IN the image -- plslam_lba_plan_host_state -- passes the image's own pointers: no copy)
        if (P->n_slots && T_kf_w != HX.T) memcpy(HX.T, T_kf_w, HX.T.bytes);
        if (P->npt && Xw != HX.Xw) memcpy(HX.Xw, Xw, HX.Xw.bytes);
        if (P->nls && Lw != HX.Lw) memcpy(HX.Lw, Lw, HX.Lw.bytes);
        if (P->dyn_bytes) PLSLAM_HIP_CHECK(hipMemcpyAsync(P->dyn.p, P->pin_in.p, P->dyn_bytes, hipMemcpyHostToDevice, s));
        P->state_valid = true;
    }
    const int32_t nbp = (P->np + 255) / 256, nbl = (P->nl + 255) / 256;
    LbaIterArgs A{};
    A.K = CamD{P->cam.fx, P->cam.fy, P->cam.cx, P->cam.cy, (double)P->cam.width, (double)P->cam.height};
    A.th = P->th;
    A.compat_iter = (compat_flags & PLSLAM_LBA_COMPAT_ITER_PASS) ? 1 : 0;
    A.transpose_ls_cross = (compat_flags & PLSLAM_LBA_COMPAT_GBA) ? 1 : 0;
    A.T = X.T; A.Xw = X.Xw; A.Lw = X.Lw; A.uv = S.uv; A.lobs = S.lobs;
    A.pt_lm = S.pt_lm; A.pt_slot = S.pt_slot; A.pt_kf_loc = S.pt_kf; A.ls_lm = S.ls_lm; A.ls_slot = S.ls_slot; A.ls_kf_loc = S.ls_kf;
    A.np = P->np; A.nl = P->nl; A.nbp = nbp; A.nbl = nbl; A.n_slots = P->n_slots;
    A.pJp = R.pJp; A.pJl = R.pJl; A.pr = R.pr; A.pw = R.pw; A.lJp = R.lJp; A.lJl = R.lJl; A.lr = R.lr; A.lw = R.lw;
    A.Wp = O.W_pt; A.Wl = O.W_ls; A.err_part = O.err_part;
    if (nbp + nbl > 0 && ctl) hipLaunchKernelGGL(k_lba_rows_cross_lm, dim3(nbp + nbl), dim3(256), 0, s, A, ctl);
    else if (nbp + nbl > 0) hipLaunchKernelGGL(k_lba_rows_cross, dim3(nbp + nbl), dim3(256), 0, s, A);
    LbaBlockArgs B = lba_block_args(P);
    const bool fused = fused_lambda >= 0.0;
    if (fused) {
        const LbaSchurView& C = P->sc;
        B.lambda = fused_lambda;
        B.Vp = C.Vp; B.Vl = C.Vl; B.tp = C.tp; B.tl = C.tl;
        B.nsing = C.tail.sing + P->schur_parity;
    }
    const int32_t nchunk_wgs = (P->nkf * P->max_chunks + 3) / 4;
    if (B.nb3 + B.nb6 + nchunk_wgs > 0 && ctl)
        hipLaunchKernelGGL(k_lba_blocks_lm, dim3(B.nb3 + B.nb6 + nchunk_wgs), dim3(256), 0, s, B, ctl);
    else if (B.nb3 + B.nb6 + nchunk_wgs > 0)
        hipLaunchKernelGGL(k_lba_blocks, dim3(B.nb3 + B.nb6 + nchunk_wgs), dim3(256), 0, s, B);
    if (!fused && ctl) hipLaunchKernelGGL(k_lba_finish_lm, dim3(P->nkf + 1), dim3(256), 0, s, B, ctl);
    else if (!fused) hipLaunchKernelGGL(k_lba_finish, dim3(P->nkf + 1), dim3(256), 0, s, B);
    PLSLAM_HIP_CHECK(hipGetLastError());
    P->blocks_valid = true;
    P->blocks_gba = (compat_flags & PLSLAM_LBA_COMPAT_GBA) != 0;
    P->schur_done = false;             // (the blocks have changed: the landmark inverses of an earlier Schur step are stale)
    return PLSLAM_OK;
}

}  // namespace plslam

// The four buffers and the image of `dyn` are laid out HERE and nowhere else.  Called twice: before the buffers exist (null
// bases: only the sizes are wanted) and over their addresses.
namespace plslam {
LbaPlanBytes lba_plan_carve(plslam_lba_plan* P)
{
    const size_t np = (size_t)P->np, nl = (size_t)P->nl, N = P->n_unknowns();
    ArrCarver cs{P->stat.as<char>()}, cd{P->dyn.as<char>()}, ch{P->pin_in.as<char>()}, cr{P->rows.as<char>()}, co{P->out.as<char>()};
    LbaStatView& S = P->st;
    S.pt_lm = cs.take<int32_t>(np * 4); S.pt_slot = cs.take<int32_t>(np * 4); S.pt_kf = cs.take<int32_t>(np * 4); S.uv = cs.take<double>(np * 16);
    S.ls_lm = cs.take<int32_t>(nl * 4); S.ls_slot = cs.take<int32_t>(nl * 4); S.ls_kf = cs.take<int32_t>(nl * 4); S.lobs = cs.take<double>(nl * 24);
    // (every observation names a landmark: the landmark lists hold them all; the keyframe list those of optimised keyframes)
    S.pt_ptr = cs.take<int32_t>(((size_t)P->npt + 1) * 4); S.pt_ids = cs.take<int32_t>(np * 4, 4);
    S.ls_ptr = cs.take<int32_t>(((size_t)P->nls + 1) * 4); S.ls_ids = cs.take<int32_t>(nl * 4, 4);
    S.kf_ptr = cs.take<int32_t>(((size_t)P->nkf + 1) * 4); S.kf_ids = cs.take<int32_t>((size_t)P->n_kfi_cap * 4, 4);
    S.kf_ids.bytes = (size_t)P->n_kfi * 4;
    for (auto [c, X] : {std::pair{&cd, &P->x}, std::pair{&ch, &P->hx}}) {
        X->T = c->take<double>((size_t)P->n_slots * 128, 8); X->Xw = c->take<double>((size_t)P->npt * 24, 8); X->Lw = c->take<double>((size_t)P->nls * 48, 8);
    }
    LbaRowsView& R = P->rw;
    R.pJp = cr.take<double>(np * 48, 8); R.pJl = cr.take<double>(np * 24, 8); R.pr = cr.take<double>(np * 8, 8); R.pw = cr.take<double>(np * 8, 8);
    R.lJp = cr.take<double>(nl * 48, 8); R.lJl = cr.take<double>(nl * 48, 8); R.lr = cr.take<double>(nl * 8, 8); R.lw = cr.take<double>(nl * 8, 8);
    LbaOutView& O = P->o;
    O.g = co.take<double>(N * 8, 8); O.H_pose = co.take<double>((size_t)P->nkf * 288, 8); O.H_pt = co.take<double>((size_t)P->npt * 72, 8);
    O.H_ls = co.take<double>((size_t)P->nls * 288, 8); O.W_pt = co.take<double>(np * 144, 8); O.W_ls = co.take<double>(nl * 288, 8);
    O.err_part = co.take<double>(8 * ((np + 255) / 256 + (nl + 255) / 256), 8);      // the row workgroups' partial sums of err
    O.pose_part = co.take<double>((size_t)P->nkf * (size_t)P->max_chunks * 42 * 8, 8);
    if (P->out.p) {
        O.err = {O.g + N, 8};                      // err: the double right behind g (one copy brings both back)
        P->hg = {P->pin_out.as<double>(), N * 8};  // pin_out: g, and err behind it
        P->herr = P->hg + N;
    }
    return {cs.size(), cd.size(), cr.size(), co.size()};
}
}  // namespace plslam

extern "C" int plslam_lba_plan_create(plslam_ctx* ctx, const plslam_cam* K, double homog_th, int32_t n_pose_slots,
                                      int32_t nkf, int32_t npt, int32_t nls, const int32_t* pt_lm_loc,
                                      const int32_t* pt_pose_slot, const int32_t* pt_kf_loc, const double* pt_obs_uv,
                                      int32_t n_pt_obs, const int32_t* ls_lm_loc, const int32_t* ls_pose_slot,
                                      const int32_t* ls_kf_loc, const double* ls_l_obs, int32_t n_ls_obs,
                                      plslam_lba_plan** out)
{
    PLSLAM_REQUIRE(ctx && K && out && n_pose_slots >= 0 && nkf >= 0 && npt >= 0 && nls >= 0, PLSLAM_EINVAL);
    PLSLAM_REQUIRE(n_pt_obs >= 0 && n_ls_obs >= 0, PLSLAM_EINVAL);
    PLSLAM_REQUIRE(n_pt_obs == 0 || (pt_lm_loc && pt_pose_slot && pt_kf_loc && pt_obs_uv), PLSLAM_EINVAL);
    PLSLAM_REQUIRE(n_ls_obs == 0 || (ls_lm_loc && ls_pose_slot && ls_kf_loc && ls_l_obs), PLSLAM_EINVAL);
    *out = nullptr;
    for (int32_t o = 0; o < n_pt_obs; ++o)
        PLSLAM_REQUIRE(pt_lm_loc[o] >= 0 && pt_lm_loc[o] < npt && pt_kf_loc[o] >= -1 && pt_kf_loc[o] < nkf &&
                       pt_pose_slot[o] >= 0 && pt_pose_slot[o] < n_pose_slots, PLSLAM_EINVAL);
    for (int32_t o = 0; o < n_ls_obs; ++o)
        PLSLAM_REQUIRE(ls_lm_loc[o] >= 0 && ls_lm_loc[o] < nls && ls_kf_loc[o] >= -1 && ls_kf_loc[o] < nkf &&
                       ls_pose_slot[o] >= 0 && ls_pose_slot[o] < n_pose_slots, PLSLAM_EINVAL);
    plslam_lba_plan* P = new (std::nothrow) plslam_lba_plan();
    PLSLAM_REQUIRE(P != nullptr, PLSLAM_ENOMEM);
    P->ctx = ctx; P->cam = *K; P->th = homog_th; P->n_slots = n_pose_slots; P->nkf = nkf; P->npt = npt; P->nls = nls;
    P->np = n_pt_obs; P->nl = n_ls_obs;
    CsrLists& c = P->csr;
    build_csr(pt_lm_loc, pt_kf_loc, n_pt_obs, ls_lm_loc, ls_kf_loc, n_ls_obs, nkf, npt, nls, c);
    if (n_pt_obs) P->h_pt_kf.assign(pt_kf_loc, pt_kf_loc + n_pt_obs);
    if (n_ls_obs) P->h_ls_kf.assign(ls_kf_loc, ls_kf_loc + n_ls_obs);
    P->max_chunks = pose_max_chunks(c.kfp);
    P->n_kfi = P->n_kfi_cap = (int32_t)c.kfi.size();
    const LbaPlanBytes need = lba_plan_carve(P);
    P->dyn_bytes = need.dyn;
    auto fail = [P](int rc) { P->release(); delete P; return rc; };
    int rc;
    if ((rc = P->stat.reserve(need.stat + 256)) || (rc = P->dyn.reserve(need.dyn + 256)) || (rc = P->rows.reserve(need.rows + 256)) ||
        (rc = P->out.reserve(need.out + 256)) || (rc = P->pin_in.reserve(need.dyn + 256)) || (rc = P->pin_out.reserve(P->n_unknowns() * 8 + 256)))
        return fail(rc);
    lba_plan_carve(P);
    std::lock_guard<std::mutex> lk(ctx->mu);
    DeviceGuard dg_(ctx->device);    // every entry point runs on the context's device, whatever the calling thread's current one
    hipStream_t s = ctx->stream;
    auto up = [&](const auto& dst, const void* src) -> int {
        if (dst.bytes) PLSLAM_HIP_CHECK(hipMemcpyAsync(dst.p, src, dst.bytes, hipMemcpyHostToDevice, s));
        return PLSLAM_OK;
    };
    const LbaStatView& V = P->st;
    if ((rc = up(V.pt_lm, pt_lm_loc)) || (rc = up(V.pt_slot, pt_pose_slot)) || (rc = up(V.pt_kf, pt_kf_loc)) || (rc = up(V.uv, pt_obs_uv)) ||
        (rc = up(V.ls_lm, ls_lm_loc)) || (rc = up(V.ls_slot, ls_pose_slot)) || (rc = up(V.ls_kf, ls_kf_loc)) || (rc = up(V.lobs, ls_l_obs)) ||
        (rc = up(V.pt_ptr, c.ptp.data())) || (rc = up(V.pt_ids, c.pti.data())) || (rc = up(V.ls_ptr, c.lsp.data())) ||
        (rc = up(V.ls_ids, c.lsi.data())) || (rc = up(V.kf_ptr, c.kfp.data())) || (rc = up(V.kf_ids, c.kfi.data())) ||
        (hipStreamSynchronize(s) != hipSuccess && (rc = PLSLAM_EHIP))) {   // the staging vectors die here
        (void)hipStreamSynchronize(s);
        return fail(rc);
    }
    *out = P;
    return PLSLAM_OK;
}

// g (+ err) down by a KERNEL that writes the page-locked block where the device can address it: a copy command of this size runs on
// the copy engine, which starts ~13 us after the kernel in front of it (profiles/r6_r_call_timeline_map2kf_points_fast.txt: the
// same pattern); a kernel starts 2-3 us after, and 0.34 MB of posted writes cross PCIe in ~7 us either way
__global__ void __launch_bounds__(256)
k_copy_out(const double* __restrict__ src, double* __restrict__ dst, size_t n)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) dst[i] = src[i];
}

// device -> host copies on the plan's stream (NULL destinations and empty arrays are skipped), then one synchronise.  A copy
// that fails drains the stream first: nothing is left in flight into the caller's arrays.
struct LbaDown { void* dst; Arr<double> src; };
template <size_t N>
static int lba_download(hipStream_t s, const LbaDown (&copies)[N])
{
    StreamSyncOnError drain(s);
    for (const LbaDown& c : copies)
        if (c.dst && c.src.bytes) PLSLAM_HIP_CHECK(hipMemcpyAsync(c.dst, c.src.p, c.src.bytes, hipMemcpyDeviceToHost, s));
    PLSLAM_HIP_CHECK(hipStreamSynchronize(s));
    drain.dismiss();
    return PLSLAM_OK;
}

// the blocks of the last iteration to the host
static int lba_plan_download(plslam_lba_plan* P, double* g, double* H_pose, double* H_pt, double* H_ls, double* W_pt,
                             double* W_ls, double* err)
{
    hipStream_t s = P->ctx->stream;
    const LbaOutView& O = P->o;
    if (!H_pose && !H_pt && !H_ls && !W_pt && !W_ls) {
        // g and err (or err alone): one copy into page-locked memory, then out of it
        // err alone lands in the slot it has in the g + err copy, BEHIND the image's g (plslam_lba_plan_host_state hands
        // out the image as g: an err-only iteration -- a rejected LM trial step -- must leave the gradient there untouched)
        if (g && P->pin_out.dev) {
            const size_t nd = P->n_unknowns() + 1;
            hipLaunchKernelGGL(k_copy_out, dim3((unsigned)((nd + 255) / 256)), dim3(256), 0, s, (const double*)O.g,
                               static_cast<double*>(P->pin_out.dev), nd);
            PLSLAM_HIP_CHECK(hipGetLastError());
        } else if (g) {
            PLSLAM_HIP_CHECK(hipMemcpyAsync(P->hg, O.g, O.g.bytes + O.err.bytes, hipMemcpyDeviceToHost, s));
        } else {
            PLSLAM_HIP_CHECK(hipMemcpyAsync(P->herr, O.err, O.err.bytes, hipMemcpyDeviceToHost, s));
        }
        PLSLAM_HIP_CHECK(hipStreamSynchronize(s));
        if (g && g != P->hg) memcpy(g, P->hg, P->hg.bytes);      // (g = the page-locked image itself: plslam_lba_plan_host_state)
        if (err) *err = *P->herr;
        return PLSLAM_OK;
    }
    return lba_download(s, {{g, O.g}, {H_pose, O.H_pose}, {H_pt, O.H_pt}, {H_ls, O.H_ls}, {W_pt, O.W_pt}, {W_ls, O.W_ls}, {err, O.err}});
}

extern "C" int plslam_lba_plan_iterate(plslam_lba_plan* P, const double* T_kf_w, const double* Xw, const double* Lw,
                                       int compat_flags, double* g, double* H_pose, double* H_pt, double* H_ls,
                                       double* W_pt, double* W_ls, double* err)
{
    PLSLAM_REQUIRE(P && g && err, PLSLAM_EINVAL);
    PLSLAM_REQUIRE((P->n_slots == 0 || T_kf_w) && (P->npt == 0 || (Xw && H_pt)) && (P->nls == 0 || (Lw && H_ls)), PLSLAM_EINVAL);
    PLSLAM_REQUIRE((P->nkf == 0 || H_pose) && (P->np == 0 || W_pt) && (P->nl == 0 || W_ls), PLSLAM_EINVAL);
    plslam_ctx* ctx = P->ctx;
    std::lock_guard<std::mutex> lk(ctx->mu);
    DeviceGuard dg_(ctx->device);    // every entry point runs on the context's device, whatever the calling thread's current one
    int rc = lba_plan_enqueue(P, T_kf_w, Xw, Lw, compat_flags);
    if (rc) { (void)hipStreamSynchronize(ctx->stream); return rc; }
    return lba_plan_download(P, g, H_pose, H_pt, H_ls, W_pt, W_ls, err);
}

// The same iteration with the blocks LEFT ON THE DEVICE: what crosses PCIe is X up (0.34 MB at C3) and err (+ g when
// asked for) down, not the 11.5 MB of blocks.  plslam_lba_plan_device_blocks names them for a device-side solver;
// plslam_lba_plan_blocks fetches any of them later.
extern "C" int plslam_lba_plan_iterate_dev(plslam_lba_plan* P, const double* T_kf_w, const double* Xw, const double* Lw,
                                           int compat_flags, double* g, double* err)
{
    PLSLAM_REQUIRE(P && err, PLSLAM_EINVAL);
    PLSLAM_REQUIRE((P->n_slots == 0 || T_kf_w) && (P->npt == 0 || Xw) && (P->nls == 0 || Lw), PLSLAM_EINVAL);
    plslam_ctx* ctx = P->ctx;
    std::lock_guard<std::mutex> lk(ctx->mu);
    DeviceGuard dg_(ctx->device);
    int rc = lba_plan_enqueue(P, T_kf_w, Xw, Lw, compat_flags);
    if (rc) { (void)hipStreamSynchronize(ctx->stream); return rc; }
    return lba_plan_download(P, g, nullptr, nullptr, nullptr, nullptr, nullptr, err);
}

// The iteration on the state that already lives on the device: nothing goes up, err comes down.  For a device-side solver
// (plslam_lba_plan_device_state names T / Xw / Lw: it updates them in place on the context's stream between iterations).
extern "C" int plslam_lba_plan_iterate_resident(plslam_lba_plan* P, int compat_flags, double* err)
{
    PLSLAM_REQUIRE(P && err, PLSLAM_EINVAL);
    PLSLAM_REQUIRE(P->state_valid, PLSLAM_EINVAL);         // one plslam_lba_plan_iterate(_dev) first: it uploads the state
    plslam_ctx* ctx = P->ctx;
    std::lock_guard<std::mutex> lk(ctx->mu);
    DeviceGuard dg_(ctx->device);
    int rc = lba_plan_enqueue(P, nullptr, nullptr, nullptr, compat_flags, false);
    if (rc) { (void)hipStreamSynchronize(ctx->stream); return rc; }
    return lba_plan_download(P, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, err);
}

extern "C" int plslam_lba_plan_device_state(plslam_lba_plan* P, plslam_lba_state* out)
{
    PLSLAM_REQUIRE(P && out, PLSLAM_EINVAL);
    out->T_kf_w = P->x.T; out->Xw = P->x.Xw; out->Lw = P->x.Lw;
    out->n_pose_slots = P->n_slots; out->npt = P->npt; out->nls = P->nls;
    out->stream = P->ctx->stream;
    return PLSLAM_OK;
}

// The plan's page-locked images by name: a host solver that keeps T / Xw / Lw there and reads g from there hands these very
// pointers to plslam_lba_plan_iterate / _iterate_dev, which then skip their staging copies (0.34 MB in, 0.34 MB out at C3).
extern "C" int plslam_lba_plan_host_state(plslam_lba_plan* P, plslam_lba_host_state* out)
{
    PLSLAM_REQUIRE(P && out, PLSLAM_EINVAL);
    out->T_kf_w = P->hx.T; out->Xw = P->hx.Xw; out->Lw = P->hx.Lw;      // (fixed at plan creation: nothing to lock)
    out->g = P->hg;
    out->n_pose_slots = P->n_slots; out->npt = P->npt; out->nls = P->nls;
    out->n = (int64_t)P->n_unknowns();
    return PLSLAM_OK;
}

extern "C" int plslam_lba_plan_device_blocks(plslam_lba_plan* P, plslam_lba_blocks* out)
{
    PLSLAM_REQUIRE(P && out, PLSLAM_EINVAL);
    const LbaOutView& O = P->o;
    out->g = O.g; out->H_pose = O.H_pose; out->H_pt = O.H_pt; out->H_ls = O.H_ls; out->W_pt = O.W_pt; out->W_ls = O.W_ls;
    out->err = O.err;
    out->stream = P->ctx->stream;
    return PLSLAM_OK;
}

extern "C" int plslam_lba_plan_blocks(plslam_lba_plan* P, double* g, double* H_pose, double* H_pt, double* H_ls,
                                      double* W_pt, double* W_ls, double* err)
{
    PLSLAM_REQUIRE(P != nullptr, PLSLAM_EINVAL);
    plslam_ctx* ctx = P->ctx;
    std::lock_guard<std::mutex> lk(ctx->mu);
    DeviceGuard dg_(ctx->device);
    return lba_plan_download(P, g, H_pose, H_pt, H_ls, W_pt, W_ls, err);
}

// the rows of the last iterate() (device -> host), e.g. for the outlier logic of :1831-1846
extern "C" int plslam_lba_plan_rows(plslam_lba_plan* P, double* pt_J_pose, double* pt_J_lm, double* pt_r, double* pt_w,
                                    double* ls_J_pose, double* ls_J_lm, double* ls_r, double* ls_w)
{
    PLSLAM_REQUIRE(P != nullptr, PLSLAM_EINVAL);
    plslam_ctx* ctx = P->ctx;
    std::lock_guard<std::mutex> lk(ctx->mu);
    DeviceGuard dg_(ctx->device);    // every entry point runs on the context's device, whatever the calling thread's current one
    const LbaRowsView& R = P->rw;
    return lba_download(ctx->stream, {{pt_J_pose, R.pJp}, {pt_J_lm, R.pJl}, {pt_r, R.pr}, {pt_w, R.pw},
                                      {ls_J_pose, R.lJp}, {ls_J_lm, R.lJl}, {ls_r, R.lr}, {ls_w, R.lw}});
}

extern "C" void plslam_lba_plan_destroy(plslam_lba_plan* P)
{
    if (!P) return;
    (void)hipStreamSynchronize(P->ctx->stream);
    P->release();
    delete P;
}

// The resident landmarks, device -> host (round 6): what plslam_lba_plan_backsub(apply) has updated in place comes back -- into
// the plan's page-locked images first (plslam_lba_plan_host_state: the image no longer holds the landmarks of BEFORE the step, so
// a later plslam_lba_plan_iterate / _iterate_dev with the image's own pointers does not revert it -- ADVICE r5), then to the
// caller's arrays (either may be NULL).  The reference's write-back reads them there (src/mapHandler.cpp:1822-1852).
extern "C" int plslam_lba_plan_get_landmarks(plslam_lba_plan* P, double* Xw, double* Lw)
{
    PLSLAM_REQUIRE(P != nullptr, PLSLAM_EINVAL);
    plslam_ctx* ctx = P->ctx;
    std::lock_guard<std::mutex> lk(ctx->mu);
    DeviceGuard dg_(ctx->device);
    PLSLAM_REQUIRE(P->state_valid, PLSLAM_EINVAL);         // one plslam_lba_plan_iterate(_dev) first: it uploads the state
    hipStream_t s = ctx->stream;
    const LbaStateView &X = P->x, &HX = P->hx;
    const size_t bx = X.Xw.bytes, bl = X.Lw.bytes;
    if (bx) PLSLAM_HIP_CHECK(hipMemcpyAsync(HX.Xw, X.Xw, bx, hipMemcpyDeviceToHost, s));
    if (bl) PLSLAM_HIP_CHECK(hipMemcpyAsync(HX.Lw, X.Lw, bl, hipMemcpyDeviceToHost, s));
    PLSLAM_HIP_CHECK(hipStreamSynchronize(s));
    if (Xw && bx && Xw != HX.Xw) memcpy(Xw, HX.Xw, bx);
    if (Lw && bl && Lw != HX.Lw) memcpy(Lw, HX.Lw, bl);
    return PLSLAM_OK;
}

// the optimised poses alone (the host has applied dp to them: expmap / logmap of SE(3) stay with the caller, :1560-1566)
extern "C" int plslam_lba_plan_set_poses(plslam_lba_plan* P, const double* T_kf_w)
{
    PLSLAM_REQUIRE(P && (P->n_slots == 0 || T_kf_w), PLSLAM_EINVAL);
    plslam_ctx* ctx = P->ctx;
    std::lock_guard<std::mutex> lk(ctx->mu);
    DeviceGuard dg_(ctx->device);
    // (a device-built plan whose landmarks were copied in at creation: the poses complete its state)
    PLSLAM_REQUIRE(P->state_valid || P->lm_resident, PLSLAM_EINVAL);
    hipStream_t s = ctx->stream;
    if (P->n_slots) {
        memcpy(P->hx.T, T_kf_w, P->hx.T.bytes);
        PLSLAM_HIP_CHECK(hipMemcpyAsync(P->x.T, P->hx.T, P->x.T.bytes, hipMemcpyHostToDevice, s));
        PLSLAM_HIP_CHECK(hipStreamSynchronize(s));
    }
    P->state_valid = true;
    return PLSLAM_OK;
}
