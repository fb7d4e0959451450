// map_lists.hip -- desc_list / dir_list / pts_list and the representative descriptor of the device-resident map
// (plslam_map_lists, include/plslam_hip.h): the lists follow plslam_map_insert_* and plslam_lc_fuse_run out of place, and
// MapPoint / MapLine::updateAverageDescDir (src/mapFeatures.cpp:51-84, :121-157) runs for exactly the landmarks the reference runs
// it for (:41-49, :110-119; src/mapHandler.cpp:4515, :4663).  The argument checks, the geometry and the scratch layout are
// map_lists_plan.hpp's.  Per landmark kind, all on the context's stream, nothing waited for:
//   K85 k_lists_carry: a gather by obs_src.  LISTS_LANES_PER_OBS = 8 lanes per DESTINATION observation: lanes 0-1 the descriptor
//       (2 x 16 bytes), 2-4 the direction (3 x 8), 5-6 pts (2 x 16, lines), lane 7 idle.  The row comes from the source lists
//       (obs_src >= 0) or from the caller's keyframe / tuple rows and the handle's direction records.  Memory-bound; 16-byte
//       accesses need desc / pts 16-byte aligned (dir rows are 24 bytes: 8-byte accesses), which the plan has checked.
//   K86 k_lists_touched: a lane per destination landmark.  TOUCHED = new, or the list's length changed, or the valid flag did.
//       One stable compaction with two look-back chains: the touched landmarks, and the offsets of their lists in the row space
//       of K87.  An untouched landmark's med_idx / med_desc are copied; a touched one's slot is set to the key maximum.
//   K87 k_lists_row_medians: a lane per (touched landmark, observation) = one row of conf: K12's order statistic
//       (median_desc_dev.hpp, the ROW_CACHE split included) and an atomic minimum of the key (value << 23 | i): "smallest value,
//       then first row" in any order.  The launch covers the destination's n_obs lanes (the host knows no tighter bound without
//       waiting); the lanes beyond the touched rows leave at once.
//   K88 k_lists_select: a lane per touched landmark decodes the slot and gathers the winner's 32 bytes (zeros for an empty list).
// Every index read from a record is range-checked before it is used as an address; a row that cannot be resolved is zeros.
#include "common.hpp"
#include "lookback_dev.hpp"
#include "map_image_dev.hpp"
#include "map_lists_plan.hpp"
#include "median_desc_dev.hpp"

namespace plslam {
namespace {

static_assert(LISTS_TILE == MAP_TILE && LISTS_TILE == MEDIAN_NT, "one tile for the look-back, the row cache and the plan's geometry");

struct ListsSrcD { const uint8_t* desc; const double *dir, *pts; const int32_t* med_idx; const uint8_t* med_desc; };
struct ListsDstD { uint8_t* desc; double *dir, *pts; int32_t* med_idx; uint8_t *med_desc, *refreshed; };
struct CarryD {                          // one kind of one carry
    int32_t src_n, src_obs, dst_n, dst_obs, n_ev, ev_stride, bound0, bound1;
    const int32_t *obs_src, *ev;
    const double* ev_dir;
    const uint8_t *rdesc0, *rdesc1;
    const double *rpts0, *rpts1;
    const int32_t *src_ptr, *dst_ptr;
    const uint8_t *src_valid, *dst_valid;
    uint32_t* part;                      // 2 x gridDim.x chain words of K86
    int32_t *cnt, *tl, *toff;            // cnt[0] touched landmarks, cnt[1] their observations; tl[r] the r-th touched landmark,
};                                       // toff[r] the offset of its list among the touched rows

// K85: the gather.  8 lanes per destination observation.
__global__ void __launch_bounds__(LISTS_TILE)
k_lists_carry(ListsSrcD S, ListsDstD D, CarryD C)
{
    const int64_t t = (int64_t)blockIdx.x * LISTS_TILE + threadIdx.x, j = t / LISTS_LANES_PER_OBS;
    const int part = (int)(t % LISTS_LANES_PER_OBS);
    if (j >= C.dst_obs || part == 7 || (part >= 5 && !D.pts)) return;
    const int32_t s = C.obs_src[j];
    // where the row comes from: row `row` of the source lists (from = 0), of the side-0 / side-1 rows (1 / 2), or nowhere (-1)
    int from = -1;
    int64_t row = 0, drow = -1;          // drow: the row of 3 doubles in ev_dir
    if (s >= 0) {
        if (s < C.src_obs) { from = 0; row = s; }
    } else {
        const int64_t u = -1 - (int64_t)s, e = u >> 1;
        const int w = (int)(u & 1);
        if (e < C.n_ev) {
            drow = 2 * e + w;
            const int64_t r = C.ev_stride ? (int64_t)C.ev[C.ev_stride * e + 1 + w] : e;
            if (r >= 0 && r < (w ? C.bound1 : C.bound0)) { from = 1 + w; row = r; }
        }
    }
    if (part < 2) {
        gvec4_t v = {0u, 0u, 0u, 0u};
        if (from == 0) v = g_((const gvec4_t*)S.desc)[2 * row + part];
        else if (from == 1 && C.rdesc0) v = g_((const gvec4_t*)C.rdesc0)[2 * row + part];
        else if (from == 2 && C.rdesc1) v = g_((const gvec4_t*)C.rdesc1)[2 * row + part];
        g_((gvec4_t*)D.desc)[2 * j + part] = v;
    } else if (part < 5) {
        const int a = part - 2;
        double v = 0.0;
        if (from == 0) v = g_(S.dir)[3 * row + a];
        else if (drow >= 0) v = g_(C.ev_dir)[3 * drow + a];
        g_(D.dir)[3 * j + a] = v;
    } else {
        const int a = part - 5;
        gvec4_t v = {0u, 0u, 0u, 0u};
        if (from == 0 && S.pts) v = g_((const gvec4_t*)S.pts)[2 * row + a];
        else if (from == 1 && C.rpts0) v = g_((const gvec4_t*)C.rpts0)[2 * row + a];
        else if (from == 2 && C.rpts1) v = g_((const gvec4_t*)C.rpts1)[2 * row + a];
        g_((gvec4_t*)D.pts)[2 * j + a] = v;
    }
}

// the length of landmark i's list in obs_ptr, 0 where that is no list inside n_obs observations
__device__ __forceinline__ int32_t list_len(const int32_t* __restrict__ ptr, int32_t i, int32_t n_obs)
{
    const int32_t b = g_(ptr)[i], e = g_(ptr)[i + 1];
    return b >= 0 && e > b && e <= n_obs ? e - b : 0;
}

// K86: the touched landmarks.  A lane per destination landmark; every lane of every workgroup takes part in the two chains.
__global__ void __launch_bounds__(LISTS_TILE)
k_lists_touched(ListsSrcD S, ListsDstD D, CarryD C)
{
    __shared__ uint32_t s_t[MAP_NW], s_r[MAP_NW], s_before_t, s_before_r;
    const int tid = (int)threadIdx.x, lane = tid & 63, wv = tid >> 6, b = (int)blockIdx.x;
    const int32_t i = b * LISTS_TILE + tid;
    const bool in = i < C.dst_n;
    bool touched = false;
    uint32_t len = 0;
    if (in) {
        len = (uint32_t)list_len(C.dst_ptr, i, C.dst_obs);
        touched = i >= C.src_n || (uint32_t)list_len(C.src_ptr, i, C.src_obs) != len || (g_(C.src_valid)[i] != 0) != (g_(C.dst_valid)[i] != 0);
    }
    const uint32_t rows = touched ? len : 0u;
    const uint64_t mt = __ballot(touched);
    const uint32_t incl = wave_inclusive_sum(rows);
    if (lane == 0) s_t[wv] = (uint32_t)__popcll(mt);
    if (lane == 63) s_r[wv] = incl;
    __syncthreads();                                            // (one barrier for the two chains)
    uint32_t own_t, in_t, own_r, in_r;
    waves_before_and_all<MAP_NW>(s_t, wv, in_t, own_t);
    waves_before_and_all<MAP_NW>(s_r, wv, in_r, own_r);
    const uint32_t before_t = lookback_exclusive(C.part, b, own_t, &s_before_t);
    const uint32_t before_r = lookback_exclusive(C.part + gridDim.x, b, own_r, &s_before_r);
    if (touched) {
        const uint32_t r = before_t + in_t + (uint32_t)__popcll(mt & ((1ull << lane) - 1ull));
        g_(C.tl)[r] = i;
        g_(C.toff)[r] = (int32_t)(before_r + in_r + incl - rows);
        g_(D.med_idx)[i] = -1;                                  // K87's slot: the key maximum
    } else if (in) {
        g_(D.med_idx)[i] = g_(S.med_idx)[i];
        g_((gvec4_t*)D.med_desc)[2 * (int64_t)i] = g_((const gvec4_t*)S.med_desc)[2 * (int64_t)i];
        g_((gvec4_t*)D.med_desc)[2 * (int64_t)i + 1] = g_((const gvec4_t*)S.med_desc)[2 * (int64_t)i + 1];
    }
    if (in && D.refreshed) g_(D.refreshed)[i] = touched ? 1 : 0;
    if (b == (int)gridDim.x - 1 && tid == 0) {
        g_(C.cnt)[0] = (int32_t)(before_t + own_t);
        g_(C.cnt)[1] = (int32_t)(before_r + own_r);
        g_(C.toff)[before_t + own_t] = (int32_t)(before_r + own_r);
    }
}

// K87: a lane per (touched landmark, observation): the row's order statistic, folded into the landmark's slot
__global__ void __launch_bounds__(LISTS_TILE)
k_lists_row_medians(ListsDstD D, CarryD C)
{
    __shared__ uint16_t row_cache[MEDIAN_ROW_CACHE][MEDIAN_NT];
    const int64_t t = (int64_t)blockIdx.x * LISTS_TILE + threadIdx.x;
    const int32_t n_t = g_(C.cnt)[0], total = g_(C.cnt)[1];
    if (t >= total || n_t <= 0 || n_t > C.dst_n) return;
    const int32_t r = segment_of(C.toff, n_t, (int32_t)t), lm = g_(C.tl)[r], i = (int32_t)t - g_(C.toff)[r];
    if (lm < 0 || lm >= C.dst_n) return;
    const int32_t n = list_len(C.dst_ptr, lm, C.dst_obs);
    if (i < 0 || i >= n) return;
    uint32_t* slot = reinterpret_cast<uint32_t*>(D.med_idx) + lm;
    if (n == 1) {                        // a single observation is its own representative
        g_(slot)[0] = 0u;
        return;
    }
    atomicMin(slot, median_row_key(reinterpret_cast<const uint32_t*>(D.desc), (int64_t)g_(C.dst_ptr)[lm], n, i, row_cache));
}

// K88: a lane per touched landmark: the slot decoded, the winner's row gathered
__global__ void __launch_bounds__(LISTS_TILE)
k_lists_select(ListsDstD D, CarryD C)
{
    const int64_t r = (int64_t)blockIdx.x * LISTS_TILE + threadIdx.x;
    const int32_t n_t = g_(C.cnt)[0];
    if (r >= n_t || n_t > C.dst_n) return;
    const int32_t lm = g_(C.tl)[r];
    if (lm < 0 || lm >= C.dst_n) return;
    const int32_t n = list_len(C.dst_ptr, lm, C.dst_obs);
    int32_t idx = n > 0 ? (int32_t)((uint32_t)g_(D.med_idx)[lm] & MEDIAN_IDX_MASK) : -1;
    if (idx >= n) idx = -1;
    g_(D.med_idx)[lm] = idx;
    gvec4_t lo = {0u, 0u, 0u, 0u}, hi = {0u, 0u, 0u, 0u};
    if (idx >= 0) {
        const int64_t row = (int64_t)g_(C.dst_ptr)[lm] + idx;
        lo = g_((const gvec4_t*)D.desc)[2 * row];
        hi = g_((const gvec4_t*)D.desc)[2 * row + 1];
    }
    g_((gvec4_t*)D.med_desc)[2 * (int64_t)lm] = lo;
    g_((gvec4_t*)D.med_desc)[2 * (int64_t)lm + 1] = hi;
}

// a list the context's device can address as its own memory
bool on_device(const void* p, int device)
{
    if (!p) return true;
    hipPointerAttribute_t at;
    if (hipPointerGetAttributes(&at, p) != hipSuccess) { (void)hipGetLastError(); return false; }
    return at.type == hipMemoryTypeDevice && at.device == device;
}
bool lists_on_device(const plslam_map_lists* L, int device)
{
    for (const plslam_map_lists_kind* k : {&L->points, &L->lines})
        for (const void* p : {(const void*)k->desc, (const void*)k->dir, (const void*)k->pts, (const void*)k->med_idx, (const void*)k->med_desc,
                              (const void*)k->refreshed})
            if (!on_device(p, device)) return false;
    return true;
}

int carry(const char* who, plslam_ctx* ctx, const ListsRecords* R, const plslam_map_index* src_map, const plslam_map_lists* src_lists,
          const plslam_map_index* dst_map, const plslam_map_lists* dst_lists, const ListsRows rows[2])
{
    PLSLAM_REQUIRE(ctx && R, PLSLAM_EINVAL);
    ListsPlan P;
    const int rc = lists_carry_plan(*R, src_map, src_lists, dst_map, dst_lists, rows, &P);
    if (rc) {
        set_last_error("%s: refused: %s", who, P.why);
        return rc;
    }
    std::lock_guard<std::mutex> lk(ctx->mu);
    DeviceGuard dg_(ctx->device);
    if (!lists_on_device(src_lists, ctx->device) || !lists_on_device(dst_lists, ctx->device)) {
        set_last_error("%s: refused: a list is not memory of the context's device", who);
        return PLSLAM_EINVAL;
    }
    hipStream_t s = ctx->stream;
    const int rr = ctx->lists_scratch.reserve(P.scratch_bytes + 256);   // (a grow frees the old block: hipFree waits for the device)
    if (rr) return rr;
    char* d = ctx->lists_scratch.as<char>();
    PLSLAM_HIP_CHECK(hipMemsetAsync(d, 0, P.zero_bytes, s));
    const plslam_map_landmarks *SM[2] = {&src_map->points, &src_map->lines}, *DM[2] = {&dst_map->points, &dst_map->lines};
    const plslam_map_lists_kind *SL[2] = {&src_lists->points, &src_lists->lines}, *DL[2] = {&dst_lists->points, &dst_lists->lines};
    for (int k = 0; k < 2; ++k) {
        const ListsKindPlan& K = P.k[k];
        const ListsKindRecords& r = R->k[k];
        const ListsSrcD S{SL[k]->desc, SL[k]->dir, K.with_pts ? SL[k]->pts : nullptr, SL[k]->med_idx, SL[k]->med_desc};
        const ListsDstD D{DL[k]->desc, DL[k]->dir, K.with_pts ? DL[k]->pts : nullptr, DL[k]->med_idx, DL[k]->med_desc, DL[k]->refreshed};
        CarryD C{};
        C.src_n = K.src_n; C.src_obs = K.src_obs; C.dst_n = K.dst_n; C.dst_obs = K.dst_obs;
        C.n_ev = r.n_ev; C.ev_stride = r.ev_stride; C.bound0 = r.need_side0 ? r.bound[0] : 0; C.bound1 = r.bound[1];
        C.obs_src = r.obs_src; C.ev = r.ev; C.ev_dir = r.dir;
        C.rdesc0 = rows[k].desc[0]; C.rdesc1 = rows[k].desc[1]; C.rpts0 = rows[k].pts[0]; C.rpts1 = rows[k].pts[1];
        C.src_ptr = SM[k]->obs_ptr; C.dst_ptr = DM[k]->obs_ptr; C.src_valid = SM[k]->valid; C.dst_valid = DM[k]->valid;
        C.part = (uint32_t*)(d + K.o_part); C.cnt = (int32_t*)(d + K.o_cnt); C.tl = (int32_t*)(d + K.o_tl); C.toff = (int32_t*)(d + K.o_toff);
        if (K.g_carry) hipLaunchKernelGGL(k_lists_carry, dim3(K.g_carry), dim3(LISTS_TILE), 0, s, S, D, C);
        if (K.g_lm) hipLaunchKernelGGL(k_lists_touched, dim3(K.g_lm), dim3(LISTS_TILE), 0, s, S, D, C);
        if (K.g_rows) hipLaunchKernelGGL(k_lists_row_medians, dim3(K.g_rows), dim3(LISTS_TILE), 0, s, D, C);
        if (K.g_lm) hipLaunchKernelGGL(k_lists_select, dim3(K.g_lm), dim3(LISTS_TILE), 0, s, D, C);
    }
    PLSLAM_HIP_CHECK(hipGetLastError());
    return PLSLAM_OK;
}

}  // namespace
}  // namespace plslam

using namespace plslam;

extern "C" {

int plslam_map_lists_refresh(plslam_ctx* ctx, const plslam_map_index* map, const plslam_map_lists* lists)
{
    PLSLAM_REQUIRE(ctx, PLSLAM_EINVAL);
    const char* why;
    const int rc = lists_refresh_check(map, lists, &why);
    if (rc) {
        set_last_error("plslam_map_lists_refresh: refused: %s", why);
        return rc;
    }
    std::lock_guard<std::mutex> lk(ctx->mu);
    DeviceGuard dg_(ctx->device);
    if (!lists_on_device(lists, ctx->device)) {
        set_last_error("plslam_map_lists_refresh: refused: a list is not memory of the context's device");
        return PLSLAM_EINVAL;
    }
    const plslam_map_landmarks* M[2] = {&map->points, &map->lines};
    const plslam_map_lists_kind* L[2] = {&lists->points, &lists->lines};
    for (int k = 0; k < 2; ++k) {
        if (M[k]->n <= 0) continue;
        const int rr = launch_median_desc(L[k]->desc, M[k]->obs_ptr, M[k]->n, M[k]->n_obs, L[k]->med_idx, L[k]->med_desc, ctx->stream);
        if (rr) return rr;
        if (L[k]->refreshed) PLSLAM_HIP_CHECK(hipMemsetAsync(L[k]->refreshed, 1, (size_t)M[k]->n, ctx->stream));
    }
    return PLSLAM_OK;
}

int plslam_map_insert_carry(plslam_map_insert* mi, const plslam_map_index* src_map, const plslam_map_lists* src_lists,
                            const plslam_map_index* dst_map, const plslam_map_lists* dst_lists,
                            const plslam_map_insert_rows* points, const plslam_map_insert_rows* lines)
{
    plslam_ctx* ctx = nullptr;
    const ListsRecords* R = map_insert_lists_records(mi, &ctx);
    ListsRows rows[2];
    const plslam_map_insert_rows* in[2] = {points, lines};
    for (int k = 0; k < 2; ++k)
        if (in[k]) { rows[k].desc[0] = in[k]->desc1; rows[k].desc[1] = in[k]->desc2; rows[k].pts[0] = in[k]->pts1; rows[k].pts[1] = in[k]->pts2; }
    rows[0].pts[0] = rows[0].pts[1] = nullptr;                  // (points have no pts_list)
    return carry("plslam_map_insert_carry", ctx, R, src_map, src_lists, dst_map, dst_lists, rows);
}

int plslam_lc_fuse_carry(plslam_lc_fuse* lf, const plslam_map_index* src_map, const plslam_map_lists* src_lists,
                         const plslam_map_index* dst_map, const plslam_map_lists* dst_lists,
                         const plslam_lc_fuse_rows* points, const plslam_lc_fuse_rows* lines)
{
    plslam_ctx* ctx = nullptr;
    const ListsRecords* R = lc_fuse_lists_records(lf, &ctx);
    ListsRows rows[2];
    const plslam_lc_fuse_rows* in[2] = {points, lines};
    for (int k = 0; k < 2; ++k)
        if (in[k]) { rows[k].desc[0] = in[k]->desc0; rows[k].desc[1] = in[k]->desc1; rows[k].pts[0] = in[k]->pts0; rows[k].pts[1] = in[k]->pts1; }
    rows[0].pts[0] = rows[0].pts[1] = nullptr;
    return carry("plslam_lc_fuse_carry", ctx, R, src_map, src_lists, dst_map, dst_lists, rows);
}

}  // extern "C"
