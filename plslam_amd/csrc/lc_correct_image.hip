// lc_correct_image.hip -- the loop-closure map correction (MapHandler::loopClosureOptimizationCovGraphG2O,
// src/mapHandler.cpp:4306-4355 / :4364-4397) on the device-resident map image, without anchor lists: in the code the reference
// runs, map_*_kf_idx[k] is the ascending list of the valid landmarks whose first observation is keyframe k,
// so a landmark takes ONE transform, T_corr of obs_kf[obs_ptr[j]], and so does every row of its dir_list.
//   K105 k_lci_landmarks   a lane per landmark of either kind: the decision, X and med_dir in place; a lane per keyframe slot: the
//                          x_kf_w row of a corrected slot
//   K106 k_lci_dirs        a lane per row of dir of either kind: its landmark by bisection of obs_ptr between the landmarks of the
//                          tile's first and last row (found once per tile by the whole workgroup), the landmark's decision and transform
//   K107 k_lci_publish     the four counts to the page-locked block
// Both passes move their rows through LDS so that every global access of a workgroup is contiguous, 8 bytes per lane; only the
// doubles of transformed rows are stored.  The counts are sums: their atomics order nothing, K107 reads them in stream order.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "common.hpp"
#include "lc_image_plan.hpp"
#include "map_image_dev.hpp"
#include "se3_dev.hpp"

namespace plslam {
namespace {

enum { W_PT = 0, W_LS = 1, W_PT_DIR = 2, W_LS_DIR = 3, W_WORDS = 4 };
constexpr unsigned LCI_MAX_GRID = 2048;      // workgroups of a pass at most: the tiles beyond are walked (memory-bound passes)

struct LciKind {                             // one kind: the image that is read, the arrays that are written (NULL: not carried)
    MapKindSrc S;
    double *X, *med, *dir;
};
struct LciCall {
    int32_t nk;
    const double* T;                         // nk x 16
    const uint8_t* corrected;                // nk
    const double* x_new;                     // nk x 6 or NULL
    double* x_kf_w;
    int32_t* cnt;                            // W_WORDS zeroed words
};

// The slot whose T_corr landmark j takes, or -1: the landmark is valid, its list is a non-empty list inside obs_kf (old_len), its
// first observer is a slot of the map and that slot is corrected.
__device__ __forceinline__ int32_t anchor_slot(const MapKindSrc& S, int32_t j, int32_t nk, const uint8_t* __restrict__ corrected)
{
    if (!S.valid[j] || old_len(S, j) == 0) return -1;
    const int32_t k = S.obs_kf[S.obs_ptr[j]];
    return k >= 0 && k < nk && corrected[k] ? k : -1;
}
__device__ __forceinline__ void load_rt(const double* __restrict__ T, int32_t k, double c[12])
{
#pragma unroll
    for (int q = 0; q < 12; ++q) c[q] = k >= 0 ? T[16 * (size_t)k + q] : 0.0;
}

// Rows [row0, row0 + MAP_TILE) of an array of nrows rows of W doubles (W / 3 positions each), in place: lane t transforms row
// row0 + t by c where `mine`.  Called by every lane of the workgroup.  Nothing is read where no lane has a row to transform.
template <int W>
__device__ __forceinline__ void tile_xform(double* __restrict__ base, int64_t row0, int64_t nrows, bool mine, const double c[12],
                                           double* sh, uint8_t* flag)
{
    const int t = threadIdx.x;
    if (!__syncthreads_or(mine ? 1 : 0)) return;            // (also: the tile before this one is out of sh)
    const int64_t d0 = row0 * W;
    const int64_t left = nrows - row0;
    const int nd = (int)(left < MAP_TILE ? left : MAP_TILE) * W;
#pragma unroll
    for (int q = 0; q < W; ++q) {
        const int i = q * MAP_TILE + t;
        if (i < nd) sh[i] = base[d0 + i];
    }
    flag[t] = mine ? 1 : 0;
    __syncthreads();
    if (mine) {
#pragma unroll
        for (int h = 0; h < W / 3; ++h) {
            double p[3];
            xform(c, sh + W * t + 3 * h, p);
#pragma unroll
            for (int q = 0; q < 3; ++q) sh[W * t + 3 * h + q] = p[q];
        }
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < W; ++q) {
        const int i = q * MAP_TILE + t;
        if (i < nd && flag[i / W]) base[d0 + i] = sh[i];
    }
}

template <int DL>
__device__ __forceinline__ bool landmark_tile(const LciKind& K, const LciCall& C, uint32_t tile, double* sh, uint8_t* flag)
{
    const int64_t row0 = (int64_t)tile * MAP_TILE, j = row0 + threadIdx.x;
    const int32_t k = j < K.S.n ? anchor_slot(K.S, (int32_t)j, C.nk, C.corrected) : -1;
    double c[12];
    load_rt(C.T, k, c);
    tile_xform<DL>(K.X, row0, K.S.n, k >= 0, c, sh, flag);
    if (K.med) tile_xform<3>(K.med, row0, K.S.n, k >= 0, c, sh, flag);
    return k >= 0;
}

// a wave adds its lanes with `ok` to its running count (the same in every lane of the wave)
__device__ __forceinline__ void wave_tally(bool ok, int32_t& n) { n += (int32_t)__popcll(__ballot(ok)); }
__device__ __forceinline__ void wave_add(int32_t* __restrict__ word, int32_t n)
{
    if ((threadIdx.x & 63) == 0 && n) atomic_add_global(word, n);
}

// K105: tiles [0, tp) are the points', [tp, tp + tl) the lines', [tp + tl, tp + tl + tk) the keyframe slots'
__global__ void __launch_bounds__(MAP_TILE)
k_lci_landmarks(LciKind P, LciKind L, LciCall C, uint32_t tp, uint32_t tl, uint32_t tk)
{
    __shared__ double sh[MAP_TILE * 6];
    __shared__ uint8_t flag[MAP_TILE];
    int32_t n_pt = 0, n_ls = 0;
    for (uint32_t tile = blockIdx.x; tile < tp + tl + tk; tile += gridDim.x) {
        if (tile < tp) wave_tally(landmark_tile<3>(P, C, tile, sh, flag), n_pt);
        else if (tile < tp + tl) wave_tally(landmark_tile<6>(L, C, tile - tp, sh, flag), n_ls);
        else {
            const int64_t k = (int64_t)(tile - tp - tl) * MAP_TILE + threadIdx.x;
            if (k < C.nk && C.corrected[k]) {
#pragma unroll
                for (int q = 0; q < 6; ++q) C.x_kf_w[6 * k + q] = C.x_new[6 * k + q];
            }
        }
    }
    wave_add(C.cnt + W_PT, n_pt);
    wave_add(C.cnt + W_LS, n_ls);
}

// the last j in [lo, hi] with ptr[j] <= o, lo where there is none; lo <= hi, both inside ptr
__device__ __forceinline__ int32_t last_not_above(const int32_t* __restrict__ ptr, int32_t lo, int32_t hi, int64_t o)
{
    while (hi > lo) {
        const int32_t mid = lo + ((hi - lo + 1) >> 1);
        if (ptr[mid] <= o) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// For the two rows o[0] <= o[1] of a tile, the last j in [0, n) with ptr[j] <= o[r] (0 where there is none), found by the whole
// workgroup: a round cuts each range into MAP_TILE pieces, a lane probes the start of one piece per row, and the number of probes
// not above the row picks the piece -- three rounds at a million landmarks, where a bisection makes twenty dependent loads.
// Called by every lane; every probe lies inside ptr[0 .. n), whatever the array holds.  red: 2 * MAP_NW words of LDS.
__device__ __forceinline__ void tile_bounds(const int32_t* __restrict__ ptr, int32_t n, const int64_t o[2], int32_t j[2], int32_t* red)
{
    const int t = threadIdx.x;
    int32_t lo[2] = {0, 0}, len[2] = {n, n};                // the answer of row r lies in [lo[r], lo[r] + len[r])
    while (len[0] > 1 || len[1] > 1) {                      // (the same in every lane)
        int32_t step[2];
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            step[r] = (len[r] + MAP_TILE - 1) / MAP_TILE;
            const int64_t off = (int64_t)t * step[r];
            const bool hit = off < len[r] && ptr[lo[r] + off] <= o[r];
            const unsigned long long b = __ballot(hit);
            if ((t & 63) == 0) red[r * MAP_NW + (t >> 6)] = (int32_t)__popcll(b);
        }
        __syncthreads();
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            int32_t c = 0;
#pragma unroll
            for (int w = 0; w < MAP_NW; ++w) c += red[r * MAP_NW + w];
            if (c == 0) len[r] = 1;                         // no piece starts at or below the row: the answer is lo
            else {
                const int32_t end = lo[r] + len[r];
                lo[r] += (c - 1) * step[r];                 // (c - 1) * step < len: c counts lanes whose piece starts inside the range
                len[r] = end - lo[r] < step[r] ? end - lo[r] : step[r];
            }
        }
        __syncthreads();                                    // red is written again in the next round
    }
    j[0] = lo[0];
    j[1] = lo[1];
}

__device__ __forceinline__ bool dir_tile(const LciKind& K, const LciCall& C, uint32_t tile, double* sh, uint8_t* flag, int32_t* red)
{
    const MapKindSrc& S = K.S;
    const int64_t row0 = (int64_t)tile * MAP_TILE, o = row0 + threadIdx.x;
    // once per tile: the landmarks of the tile's first and last row bound every row's
    const int64_t ends[2] = {row0, row0 + MAP_TILE <= S.n_obs ? row0 + MAP_TILE - 1 : (int64_t)S.n_obs - 1};
    int32_t jb[2];
    tile_bounds(S.obs_ptr, S.n, ends, jb, red);
    if (jb[1] < jb[0]) { jb[0] = 0; jb[1] = S.n - 1; }      // (obs_ptr does not ascend: no bound)
    int32_t k = -1;
    if (o < S.n_obs) {
        const int32_t j = last_not_above(S.obs_ptr, jb[0], jb[1], o);
        const int32_t b = S.obs_ptr[j], e = S.obs_ptr[j + 1];
        if (b >= 0 && e > b && e <= S.n_obs && o >= b && o < e) k = anchor_slot(S, j, C.nk, C.corrected);
    }
    double c[12];
    load_rt(C.T, k, c);
    tile_xform<3>(K.dir, row0, S.n_obs, k >= 0, c, sh, flag);
    return k >= 0;
}

// K106: tiles [0, tp) are rows of the points' dir, [tp, tp + tl) of the lines'
__global__ void __launch_bounds__(MAP_TILE)
k_lci_dirs(LciKind P, LciKind L, LciCall C, uint32_t tp, uint32_t tl)
{
    __shared__ double sh[MAP_TILE * 3];
    __shared__ uint8_t flag[MAP_TILE];
    __shared__ int32_t red[2 * MAP_NW];
    int32_t n_pt = 0, n_ls = 0;
    for (uint32_t tile = blockIdx.x; tile < tp + tl; tile += gridDim.x) {
        if (tile < tp) wave_tally(dir_tile(P, C, tile, sh, flag, red), n_pt);
        else wave_tally(dir_tile(L, C, tile - tp, sh, flag, red), n_ls);
    }
    wave_add(C.cnt + W_PT_DIR, n_pt);
    wave_add(C.cnt + W_LS_DIR, n_ls);
}

// K107: the call's last kernel: the counts to the page-locked block
__global__ void __launch_bounds__(64)
k_lci_publish(const int32_t* __restrict__ cnt, int32_t* __restrict__ pinned)
{
    if (threadIdx.x < W_WORDS) pinned[threadIdx.x] = cnt[threadIdx.x];
}

}  // namespace
}  // namespace plslam

using namespace plslam;

extern "C" {

int plslam_lc_correct_image(plslam_ctx* ctx, const plslam_map_index* map, const double* T_corr, const uint8_t* corrected,
                            const double* x_kf_w_new, const plslam_lc_image_dst* dst, plslam_lc_image_counts* counts)
{
    PLSLAM_REQUIRE(ctx, PLSLAM_EINVAL);
    LcImagePlan P;
    int rc = lc_image_plan(map, T_corr, corrected, x_kf_w_new, dst, &P);
    if (rc) {
        set_last_error("plslam_lc_correct_image: refused: %s", P.why);
        return rc;
    }
    std::lock_guard<std::mutex> lk(ctx->mu);
    DeviceGuard dg_(ctx->device);
    hipStream_t s = ctx->stream;
    // the scratch is the context's: whatever used it before is finished first
    PLSLAM_HIP_CHECK(hipStreamSynchronize(s));
    const size_t head = lc_image_align(W_WORDS * 4);
    if ((rc = ctx->pgo_scratch.reserve(head + P.stage_bytes + 256))) return rc;
    if ((rc = ctx->lc_image_pin.reserve(head + P.stage_bytes))) return rc;
    PLSLAM_REQUIRE(ctx->lc_image_pin.dev, PLSLAM_ENOTSUP);       // the counters are written where the host reads them
    char* d = ctx->pgo_scratch.as<char>();
    char* h = ctx->lc_image_pin.as<char>();
    lc_image_pack(P, T_corr, corrected, x_kf_w_new, h + head);
    StreamSyncOnError guard(s);
    PLSLAM_HIP_CHECK(hipMemsetAsync(d, 0, head, s));
    PLSLAM_HIP_CHECK(hipMemcpyAsync(d + head, h + head, P.stage_bytes, hipMemcpyHostToDevice, s));
    const char* st = d + head;
    const LciCall C{P.nk, (const double*)(st + P.o_T), (const uint8_t*)(st + P.o_corr), P.with_x ? (const double*)(st + P.o_x) : nullptr,
                    P.with_x ? dst->x_kf_w : nullptr, (int32_t*)d};
    const LciKind Kp{map_kind_src(map->points, 0), dst->pt_X, P.with_med[0] ? dst->pt_med_dir : nullptr, P.with_dir[0] ? dst->pt_dir : nullptr};
    const LciKind Kl{map_kind_src(map->lines, 1), dst->ls_X, P.with_med[1] ? dst->ls_med_dir : nullptr, P.with_dir[1] ? dst->ls_dir : nullptr};
    auto tiles = [](int64_t n) { return (uint32_t)((n + MAP_TILE - 1) / MAP_TILE); };
    const uint32_t tp = tiles(Kp.S.n), tl = tiles(Kl.S.n), tk = P.with_x ? tiles(P.nk) : 0;
    const uint32_t dp = Kp.dir ? tiles(Kp.S.n_obs) : 0, dl = Kl.dir ? tiles(Kl.S.n_obs) : 0;
    if (tp + tl + tk)
        hipLaunchKernelGGL(k_lci_landmarks, dim3(std::min(tp + tl + tk, LCI_MAX_GRID)), dim3(MAP_TILE), 0, s, Kp, Kl, C, tp, tl, tk);
    if (dp + dl) hipLaunchKernelGGL(k_lci_dirs, dim3(std::min(dp + dl, LCI_MAX_GRID)), dim3(MAP_TILE), 0, s, Kp, Kl, C, dp, dl);
    hipLaunchKernelGGL(k_lci_publish, dim3(1), dim3(64), 0, s, (const int32_t*)C.cnt, (int32_t*)ctx->lc_image_pin.dev);
    PLSLAM_HIP_CHECK(hipGetLastError());
    PLSLAM_HIP_CHECK(hipStreamSynchronize(s));
    guard.dismiss();
    const int32_t* r = ctx->lc_image_pin.as<int32_t>();
    if (counts) *counts = plslam_lc_image_counts{r[W_PT], r[W_LS], r[W_PT_DIR], r[W_LS_DIR]};
    return PLSLAM_OK;
}

}  // extern "C"
