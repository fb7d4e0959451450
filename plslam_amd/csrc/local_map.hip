// local_map.hip -- the three host loops MapHandler::addKeyFrame runs over the whole map every keyframe
// (src/mapHandler.cpp:212-225), on a device-resident CSR image of the map (plslam_map_index):
//   formLocalMap() / formLocalMap(kf)   :836-968    K55 keyframe flags, K56 a lane per feature of a local keyframe, K57 counts
//   the candidate mask of matchMap2KF*  :547, :649  K58
//   the gather of localBundleAdjustment :1225-1321  K59 / K60 stable compactions + observation offsets (decoupled look-back,
//                                                   lookback_dev.hpp), K61 a lane per output observation
//   removeBadMapLandmarks               :2705-2786  K62
//   the write-back of the local BA      :1828-1855  K84 from an LBA plan's resident landmarks into the image
//   the gather of globalBundleAdjustment :1995-2092 K97 every flag set (form_all), then K59-K61 as they are
//   the write-back of the global BA     :2681-2697  K84 with the moved test switched off, from a GBA plan's resident landmarks
// Every output is an integer, a flag or a verbatim copy of a double: bit-exact against the sequential loops (tests/local_map_ref.py).
// Each entry point: its check, the context's lock, device and stream, the launches, one synchronisation, the commit; counts through
// page-locked memory written by the call's last kernel.  The host decisions -- the counter words, the image check, the layout of
// the handle's buffer, the handle's state with its checks and transitions, the table of the buffers -- are local_map_plan.hpp (no
// HIP in it; tests/cpp/test_local_map_plan.cpp).  Every index read from the image is range-checked before it is used as an address.
#include <cstring>

#include "common.hpp"
#include "gba_plan.hpp"
#include "lba_plan.hpp"
#include "local_map_plan.hpp"
#include "lookback_dev.hpp"
#include "map_image_dev.hpp"
#include "publish_dev.hpp"

namespace plslam {
namespace {

// The counters of a call's LAST kernel (publish_dev.hpp): NC flags per lane counted into cnt[0 .. NC), then the ticket
template <int NC>
__device__ __forceinline__ void count_and_publish(const bool (&ok)[NC], int32_t* __restrict__ cnt, const Publish& pub)
{
#pragma unroll
    for (int c = 0; c < NC; ++c) wave_count_and_wait(ok[c], cnt + c);
    publish_from_last_workgroup(pub);
}

// K55: the keyframe flags of formLocalMap (:859 / :925 the anchor, :881-885 / :947-951 the graph loop over the LAST row); a lane per
// slot.  A NULL slot is never local (deviation: the reference dereferences it, :885).
__global__ void __launch_bounds__(MAP_TILE)
k_lm_kf_flags(int32_t n_map_kf, int32_t anchor, const uint8_t* __restrict__ kf_valid, const int32_t* __restrict__ row,
              int32_t min_cov, int32_t window, uint8_t* __restrict__ kf_local)
{
    const int32_t i = (int32_t)blockIdx.x * MAP_TILE + (int32_t)threadIdx.x;
    if (i >= n_map_kf) return;
    const int32_t g = n_map_kf - 1;
    const bool loc = kf_valid[i] != 0 && (i == anchor || (i < g && (row[i] >= min_cov || g - i <= window)));
    kf_local[i] = loc ? 1 : 0;
}

// K56: the landmark flags (:860-877, :887-898): a lane per feature of either kind; the features of a local keyframe set the flag
// of the landmark they name (idx != -1 && valid; PLSLAM_FEAT_NULL = a NULL feature: skipped).  Many lanes store the same byte 1.
__global__ void __launch_bounds__(MAP_TILE)
k_lm_feat_flags(int32_t n_map_kf, const uint8_t* __restrict__ kf_local, MapKindSrc P, MapKindSrc L, uint8_t* __restrict__ pt_local,
                uint8_t* __restrict__ ls_local)
{
    const int64_t t = (int64_t)blockIdx.x * MAP_TILE + threadIdx.x;
    if (t >= (int64_t)P.n_feat + L.n_feat) return;
    const bool lines = t >= P.n_feat;
    const int32_t f = (int32_t)(lines ? t - P.n_feat : t);
    const int32_t* __restrict__ feat_ptr = lines ? L.feat_ptr : P.feat_ptr;
    const int32_t* __restrict__ feat_idx = lines ? L.feat_idx : P.feat_idx;
    const uint8_t* __restrict__ valid = lines ? L.valid : P.valid;
    uint8_t* __restrict__ local = lines ? ls_local : pt_local;
    const int32_t n = lines ? L.n : P.n;
    const int k = segment_of(feat_ptr, n_map_kf, f);
    if (!kf_local[k]) return;
    const int32_t idx = feat_idx[f];
    if (idx >= 0 && idx < n && valid[idx]) local[idx] = 1;
}

// K57: the three counts of form; a lane per flag of the three arrays
__global__ void __launch_bounds__(MAP_TILE)
k_lm_count_flags(const uint8_t* __restrict__ kf_local, int32_t nkf, const uint8_t* __restrict__ pt_local, int32_t npt,
                 const uint8_t* __restrict__ ls_local, int32_t nls, int32_t* __restrict__ cnt, Publish pub)
{
    const int64_t t = (int64_t)blockIdx.x * MAP_TILE + threadIdx.x;
    bool ok[3] = {false, false, false};
    if (t < nkf) ok[0] = kf_local[t] != 0;
    else if (t < (int64_t)nkf + npt) ok[1] = pt_local[t - nkf] != 0;
    else if (t < (int64_t)nkf + npt + nls) ok[2] = ls_local[t - nkf - npt] != 0;
    count_and_publish<3>(ok, cnt, pub);
}

// K58: candidate[i] = valid && local && kf_obs_list.back() != kf2_idx (:547, :649); no observation: 0
__global__ void __launch_bounds__(MAP_TILE)
k_lm_candidates(MapKindSrc P, MapKindSrc L, const uint8_t* __restrict__ pt_local, const uint8_t* __restrict__ ls_local, int32_t kf2_idx,
                uint8_t* __restrict__ pt_cand, uint8_t* __restrict__ ls_cand)
{
    const int64_t t = (int64_t)blockIdx.x * MAP_TILE + threadIdx.x;
    if (t >= (int64_t)P.n + L.n) return;
    const bool lines = t >= P.n;
    const int32_t i = (int32_t)(lines ? t - P.n : t);
    const uint8_t* __restrict__ valid = lines ? L.valid : P.valid;
    const uint8_t* __restrict__ local = lines ? ls_local : pt_local;
    const int32_t* __restrict__ obs_ptr = lines ? L.obs_ptr : P.obs_ptr;
    const int32_t* __restrict__ obs_kf = lines ? L.obs_kf : P.obs_kf;
    uint8_t c = 0;
    if (valid[i] && local[i]) {
        const int32_t len = lines ? old_len(L, i) : old_len(P, i);
        if (len > 0) c = obs_kf[obs_ptr[i] + len - 1] != kf2_idx ? 1 : 0;
    }
    (lines ? ls_cand : pt_cand)[i] = c;
}

// K59: kf_list (:1226-1239): the valid, local slots other than 0, ascending; the inverse table the observations' keyframe local
// index comes from (kf_list has no repeats: the reference's linear search :1265-1272 finds the same position); X_aux's poses.
__global__ void __launch_bounds__(MAP_TILE)
k_lm_compact_kf(int32_t n_map_kf, const uint8_t* __restrict__ kf_valid, const uint8_t* __restrict__ kf_local,
                const double* __restrict__ x_kf_w, int32_t* __restrict__ kf_list, int32_t* __restrict__ kf_inv,
                double* __restrict__ X_aux, int32_t* __restrict__ cnt, uint32_t* __restrict__ part)
{
    __shared__ uint32_t s_w[MAP_NW], s_before;
    const int tid = (int)threadIdx.x, b = (int)blockIdx.x;
    const int32_t i = b * MAP_TILE + tid;
    const bool v = i < n_map_kf && i != 0 && kf_valid[i] && kf_local[i];
    const TileScan sc = lookback_rank<MAP_NW>(v, part, b, s_w, &s_before);
    const uint32_t pos = sc.pos;
    if (i < n_map_kf) kf_inv[i] = v ? (int32_t)pos : -1;
    if (v) {
        kf_list[pos] = i;
#pragma unroll
        for (int c = 0; c < 6; ++c) X_aux[6 * (size_t)pos + c] = x_kf_w[6 * (size_t)i + c];
    }
    if (b == (int)gridDim.x - 1 && tid == 0) cnt[C_NKF] = (int32_t)sc.upto;
}

// K60: pt_list / ls_list (:1245-1249, :1277; :1286-1290, :1318): the stable compaction of the valid, local landmarks, and in the
// same pass the offset of each listed landmark's observations in the observation list (a second chain: the exclusive sum of the
// listed landmarks' list lengths) and X_aux's landmark block (:1251-1253, :1292-1294), which starts behind the blocks in front of
// it: their lengths are device words of the launches before this one.
__global__ void __launch_bounds__(MAP_TILE)
k_lm_compact_lm(MapKindSrc K, int lines, const uint8_t* __restrict__ local, int32_t* __restrict__ list, int32_t* __restrict__ off,
                double* __restrict__ X_aux, int32_t* __restrict__ cnt, uint32_t* __restrict__ part_n, uint32_t* __restrict__ part_o)
{
    __shared__ uint32_t s_w[MAP_NW], s_o[MAP_NW], s_before_n, s_before_o;
    const int tid = (int)threadIdx.x, lane = tid & 63, wv = tid >> 6, b = (int)blockIdx.x;
    const int32_t i = b * MAP_TILE + tid;
    const bool v = i < K.n && K.valid[i] && local[i];
    uint32_t c = 0;                                         // the landmark's observations
    if (v) {                                                // (NOT old_len: d clamped to n_obs, b >= 0 and e <= n_obs untested -- another
        const int32_t d = K.obs_ptr[i + 1] - K.obs_ptr[i];  //  function on a malformed image, kept; K61 range-checks every source position)
        c = d > 0 ? (uint32_t)(d < K.n_obs ? d : K.n_obs) : 0u;
    }
    const uint64_t m = __ballot(v);
    const uint32_t incl = wave_inclusive_sum(c);
    if (lane == 0) s_w[wv] = (uint32_t)__popcll(m);
    if (lane == 63) s_o[wv] = incl;
    __syncthreads();                                        // (one barrier for the two chains)
    uint32_t own_n, in_n, own_o, in_o;
    waves_before_and_all<MAP_NW>(s_w, wv, in_n, own_n);
    waves_before_and_all<MAP_NW>(s_o, wv, in_o, own_o);
    const uint32_t before_n = lookback_exclusive(part_n, b, own_n, &s_before_n);
    const uint32_t before_o = lookback_exclusive(part_o, b, own_o, &s_before_o);
    if (v) {
        const uint32_t pos = before_n + in_n + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
        list[pos] = i;
        off[pos] = (int32_t)(before_o + in_o + incl - c);
        const size_t base = lines ? 6 * (size_t)cnt[C_NKF] + 3 * (size_t)cnt[C_NPT] : 6 * (size_t)cnt[C_NKF];
        for (int w = 0; w < K.dl; ++w) X_aux[base + (size_t)K.dl * pos + w] = K.X[(size_t)K.dl * i + w];
    }
    if (b == (int)gridDim.x - 1 && tid == 0) {
        cnt[lines ? C_NLS : C_NPT] = (int32_t)(before_n + own_n);
        cnt[lines ? C_LS_OBS : C_PT_OBS] = (int32_t)(before_o + own_o);
    }
}

// K61: the observation lists (:1255-1274, :1296-1315): a lane per OUTPUT observation of either kind.  The lane finds its landmark
// by bisection of the listed landmarks' offsets (landmarks without observations share an offset with their successor: the last
// one at or below the lane is the owner), then copies: the six Vector6i columns, the columns plslam_lba_plan_create takes and the
// observation itself.  The call's last kernel: workgroup 0 brings the counts to the page-locked block.
struct ExpandOut { int32_t *obs6, *lm_loc, *kf_loc, *pose_slot; double* val; const int32_t *list, *off; };
__global__ void __launch_bounds__(MAP_TILE)
k_lm_expand(MapKindSrc P, MapKindSrc L, ExpandOut op, ExpandOut ol, int32_t n_map_kf, const int32_t* __restrict__ kf_inv,
            const int32_t* __restrict__ cnt, int32_t* __restrict__ pinned)
{
    if (blockIdx.x == 0 && threadIdx.x >= C_NKF && threadIdx.x <= C_LS_OBS) pinned[threadIdx.x] = cnt[threadIdx.x];
    const int64_t t = (int64_t)blockIdx.x * MAP_TILE + threadIdx.x;
    if (t >= (int64_t)P.n_obs + L.n_obs) return;
    const bool lines = t >= P.n_obs;
    const int32_t j = (int32_t)(lines ? t - P.n_obs : t);
    const int32_t n_out = cnt[lines ? C_LS_OBS : C_PT_OBS], n_list = cnt[lines ? C_NLS : C_NPT];
    const int32_t cap = lines ? L.n_obs : P.n_obs;
    if (j >= n_out || j >= cap || n_list <= 0) return;
    const int32_t* __restrict__ list = lines ? ol.list : op.list;
    const int32_t* __restrict__ off = lines ? ol.off : op.off;
    const int32_t* __restrict__ obs_ptr = lines ? L.obs_ptr : P.obs_ptr;
    const int32_t* __restrict__ obs_kf = lines ? L.obs_kf : P.obs_kf;
    const double* __restrict__ obs_val = lines ? L.obs_val : P.obs_val;
    int32_t* __restrict__ obs6 = lines ? ol.obs6 : op.obs6;
    int32_t* __restrict__ lm_loc = lines ? ol.lm_loc : op.lm_loc;
    int32_t* __restrict__ kf_loc = lines ? ol.kf_loc : op.kf_loc;
    int32_t* __restrict__ pose_slot = lines ? ol.pose_slot : op.pose_slot;
    double* __restrict__ val = lines ? ol.val : op.val;
    const int dv = lines ? 3 : 2;
    const int32_t pos = segment_of(off, n_list, j);
    const int32_t lm = list[pos], o = j - off[pos];
    const int64_t src = (int64_t)obs_ptr[lm] + o;
    const bool in = src >= 0 && src < cap;
    const int32_t kf = in ? obs_kf[src] : -1;
    const int32_t kfl = kf >= 0 && kf < n_map_kf ? kf_inv[kf] : -1;
    int32_t* r = obs6 + 6 * (size_t)j;
    r[0] = lm; r[1] = pos; r[2] = o; r[3] = kf; r[4] = kfl; r[5] = 1;
    lm_loc[j] = pos;
    kf_loc[j] = kfl;
    pose_slot[j] = kf;
    for (int w = 0; w < dv; ++w) val[(size_t)dv * j + w] = in ? obs_val[(size_t)dv * src + w] : 0.0;
}

// K62: removeBadMapLandmarks (:2709-2745, :2748-2785): a lane per landmark of either kind.  The removed landmark's lane walks the
// features of its first observer in order and clears the FIRST one that names it (:2720-2728: the `break`): the minimum
// position, whatever the other lanes do -- they only ever rewrite entries that name OTHER landmarks.  A NULL first observer and
// NULL features are skipped (deviation: :2720-2723 dereference them); no observation: not culled.
// (valid and feat_idx are read AND written here: through the mutable pointers only, never through the read-only view)
struct CullKind { uint8_t* valid; int32_t* feat_idx; uint8_t* removed; };
__global__ void __launch_bounds__(MAP_TILE)
k_lm_cull(MapKindSrc P, MapKindSrc L, CullKind wp, CullKind wl, int32_t n_map_kf, const uint8_t* __restrict__ kf_valid,
          const uint8_t* __restrict__ pt_local, const uint8_t* __restrict__ ls_local, int32_t max_kf_idx, int32_t min_lm_obs,
          int32_t* __restrict__ cnt, Publish pub)
{
    const int64_t t = (int64_t)blockIdx.x * MAP_TILE + threadIdx.x;
    bool ok[2] = {false, false};
    if (t < (int64_t)P.n + L.n) {
        const bool lines = t >= P.n;
        const int32_t i = (int32_t)(lines ? t - P.n : t);
        uint8_t* __restrict__ valid = lines ? wl.valid : wp.valid;
        int32_t* __restrict__ feat_idx = lines ? wl.feat_idx : wp.feat_idx;
        const uint8_t* __restrict__ inlier = lines ? L.inlier : P.inlier;
        const uint8_t* __restrict__ local = lines ? ls_local : pt_local;
        const int32_t* __restrict__ obs_ptr = lines ? L.obs_ptr : P.obs_ptr;
        const int32_t* __restrict__ obs_kf = lines ? L.obs_kf : P.obs_kf;
        const int32_t* __restrict__ feat_ptr = lines ? L.feat_ptr : P.feat_ptr;
        const int32_t n_feat = lines ? L.n_feat : P.n_feat;
        bool rem = false;
        if (valid[i] && !local[i]) {
            const int32_t b = obs_ptr[i], len = lines ? old_len(L, i) : old_len(P, i);
            if (len > 0) {
                const int32_t first = obs_kf[b];
                if (max_kf_idx - first > 10 && (!inlier[i] || len < min_lm_obs)) {
                    rem = true;
                    valid[i] = 0;
                    if (first >= 0 && first < n_map_kf && kf_valid[first] && n_feat > 0) {
                        const int32_t fb = feat_ptr[first], fe = feat_ptr[first + 1];
                        for (int32_t f = fb > 0 ? fb : 0; f < fe && f < n_feat; ++f)
                            if (feat_idx[f] == i) {
                                feat_idx[f] = -1;
                                break;
                            }
                    }
                }
            }
        }
        (lines ? wl.removed : wp.removed)[i] = rem ? 1 : 0;
        ok[lines ? 1 : 0] = rem;
    }
    count_and_publish<2>(ok, cnt, pub);
}

// K84: the write-back of localBundleAdjustment (:1828-1855): a lane per LISTED landmark of either kind.  The operations are those
// of LbaPlanSolver::movedLandmarks (plslam_amd/host/lba_rows.hpp): d = after - before per component, s2 summed left to right
// from 0 (no contraction: the build's -ffp-contract=off), sqrt(s2) > th.  inlier is only ever cleared; X is copied verbatim.
// A listed landmark occurs once in its list: no two lanes touch the same landmark, in place on the image is safe.
struct ApplyKind { const int32_t* list; const double* Xnew; double* X; uint8_t* inlier; uint8_t* moved; int32_t n_list, n; };
// TEST = false: the write-back of globalBundleAdjustment (:2681-2697) -- the copy alone: no moved test, inlier and moved untouched,
// nothing counted
template <bool TEST>
__global__ void __launch_bounds__(MAP_TILE)
k_lm_apply_lba(ApplyKind P, ApplyKind L, double th, int32_t* __restrict__ cnt, Publish pub)
{
    const int64_t t = (int64_t)blockIdx.x * MAP_TILE + threadIdx.x;
    bool ok[2] = {false, false};
    if (t < (int64_t)P.n_list + L.n_list) {
        const bool lines = t >= P.n_list;
        const int32_t i = (int32_t)(lines ? t - P.n_list : t);
        const int32_t* __restrict__ list = lines ? L.list : P.list;
        const double* __restrict__ Xnew = lines ? L.Xnew : P.Xnew;
        double* __restrict__ X = lines ? L.X : P.X;
        uint8_t* __restrict__ inlier = lines ? L.inlier : P.inlier;
        const int32_t n = lines ? L.n : P.n;
        const int dl = lines ? 6 : 3;
        const int32_t j = list[i];
        bool mv = false;
        if (j >= 0 && j < n) {                              // (the list is the gather's: in range; checked all the same)
            double s2 = 0.0;
            for (int a = 0; a < dl; ++a) {
                const double v = Xnew[(size_t)dl * i + a];
                if (TEST) {
                    const double d = v - X[(size_t)dl * j + a];
                    s2 += d * d;
                }
                X[(size_t)dl * j + a] = v;
            }
            if (TEST) {
                mv = sqrt(s2) > th;
                if (mv) inlier[j] = 0;
            }
        }
        if (TEST) {
            (lines ? L.moved : P.moved)[i] = mv ? 1 : 0;
            ok[lines ? 1 : 0] = mv;
        }
    }
    if (TEST) count_and_publish<2>(ok, cnt, pub);
}

// K97: the flags of the global BA's gather: every non-NULL keyframe, every non-NULL landmark (:1995-2092 have no ->local test)
__global__ void __launch_bounds__(MAP_TILE)
k_lm_all_flags(int32_t nkf, const uint8_t* __restrict__ kf_valid, int32_t npt, const uint8_t* __restrict__ pt_valid, int32_t nls,
               const uint8_t* __restrict__ ls_valid, uint8_t* __restrict__ kf_local, uint8_t* __restrict__ pt_local, uint8_t* __restrict__ ls_local)
{
    const int64_t t = (int64_t)blockIdx.x * MAP_TILE + threadIdx.x;
    if (t < nkf) kf_local[t] = kf_valid[t] != 0 ? 1 : 0;
    else if (t < (int64_t)nkf + npt) pt_local[t - nkf] = pt_valid[t - nkf] != 0 ? 1 : 0;
    else if (t < (int64_t)nkf + npt + nls) ls_local[t - nkf - npt] = ls_valid[t - nkf - npt] != 0 ? 1 : 0;
}

}  // namespace
}  // namespace plslam

using namespace plslam;

struct plslam_local_map {
    plslam_ctx* ctx = nullptr;
    DevBuf buf;
    HostBuf pin;                                 // C_WORDS counters, then the staged graph row
    LocalMapState st;
    LocalMapLayout lay;                          // of the last form's image
    plslam_local_map_buffers d = {};

    template <class T> T* at(LocalMapSlot slot) { return slice_at<T>(buf.as<char>(), lay.off[slot]); }
    int32_t* cnt() { return at<int32_t>(LM_CNT); }
    uint32_t* chain(int c) { return at<uint32_t>(LM_PART) + lay.chain_off[c]; }
    int32_t* pinned_dev() { return (int32_t*)pin.dev; }
};

namespace {

// form and form_all: the layout for this image, the flags cleared, the graph row staged where the caller has one, the launches that
// set the flags (set_flags(stream): the one step the two differ in), the three counts
template <class SetFlags>
int form(plslam_local_map* lm, const plslam_map_index* map, const int32_t* row, plslam_local_map_counts* counts, SetFlags set_flags)
{
    std::lock_guard<std::mutex> lk(lm->ctx->mu);
    DeviceGuard dg_(lm->ctx->device);
    hipStream_t s = lm->ctx->stream;
    lm->st.begin_form(*map);
    lm->lay = LocalMapLayout(lm->st.z);
    int rc = lm->buf.reserve(lm->lay.total + 256);
    if (rc) return rc;
    if ((rc = lm->pin.reserve(lm->lay.pin_bytes))) return rc;
    local_map_fill_buffers(lm->d, lm->lay, lm->buf.as<char>(), (void*)s);
    PLSLAM_REQUIRE(lm->pin.dev, PLSLAM_ENOTSUP);               // the counters are written where the host reads them
    StreamSyncOnError guard(s);
    const int32_t nk = map->n_map_kf;
    int32_t* h = lm->pin.as<int32_t>();
    if (row) memcpy(h + C_WORDS, row, (size_t)nk * 4);
    PLSLAM_HIP_CHECK(hipMemsetAsync(lm->d.kf_local, 0, lm->lay.zero_bytes, s));
    if (row) PLSLAM_HIP_CHECK(hipMemcpyAsync(lm->at<int32_t>(LM_ROW), h + C_WORDS, (size_t)nk * 4, hipMemcpyHostToDevice, s));
    set_flags(s);
    const Publish pub{lm->cnt() + C_FORM_DONE, lm->cnt(), lm->pinned_dev(), 3};
    hipLaunchKernelGGL(k_lm_count_flags, dim3(map_tiles((int64_t)nk + map->points.n + map->lines.n)), dim3(MAP_TILE), 0, s,
                       (const uint8_t*)lm->d.kf_local, nk, (const uint8_t*)lm->d.pt_local, map->points.n, (const uint8_t*)lm->d.ls_local,
                       map->lines.n, lm->cnt(), pub);
    PLSLAM_HIP_CHECK(hipGetLastError());
    PLSLAM_HIP_CHECK(hipStreamSynchronize(s));
    guard.dismiss();
    lm->st.end_form(h, counts);
    return PLSLAM_OK;
}

}  // namespace

extern "C" {

int plslam_local_map_create(plslam_ctx* ctx, plslam_local_map** out)
{
    PLSLAM_REQUIRE(ctx && out, PLSLAM_EINVAL);
    *out = new plslam_local_map();
    (*out)->ctx = ctx;
    return PLSLAM_OK;
}

void plslam_local_map_destroy(plslam_local_map* lm)
{
    if (!lm) return;
    release_handle_buffers(lm->ctx, lm->buf, lm->pin);
    delete lm;
}

int plslam_local_map_form(plslam_local_map* lm, const plslam_map_index* map, int32_t anchor_kf, const int32_t* row,
                          int32_t min_lm_cov_graph, int32_t min_kf_local_map, plslam_local_map_counts* counts)
{
    PLSLAM_REQUIRE(lm && !LocalMapState::check_form(map, anchor_kf, row, counts), PLSLAM_EINVAL);
    return form(lm, map, row, counts, [=](hipStream_t s) {
        const int32_t nk = map->n_map_kf;
        const MapKindSrc P = map_kind_src(map->points, 0), L = map_kind_src(map->lines, 1);
        hipLaunchKernelGGL(k_lm_kf_flags, dim3(map_tiles(nk)), dim3(MAP_TILE), 0, s, nk, anchor_kf, map->kf_valid,
                           (const int32_t*)lm->at<int32_t>(LM_ROW), min_lm_cov_graph, min_kf_local_map, lm->d.kf_local);
        const int64_t nfeat = (int64_t)P.n_feat + L.n_feat;
        if (nfeat > 0)
            hipLaunchKernelGGL(k_lm_feat_flags, dim3(map_tiles(nfeat)), dim3(MAP_TILE), 0, s, nk, (const uint8_t*)lm->d.kf_local, P, L,
                               lm->d.pt_local, lm->d.ls_local);
    });
}

int plslam_local_map_form_all(plslam_local_map* lm, const plslam_map_index* map, plslam_local_map_counts* counts)
{
    PLSLAM_REQUIRE(lm && !LocalMapState::check_form_all(map, counts), PLSLAM_EINVAL);
    return form(lm, map, nullptr, counts, [=](hipStream_t s) {
        const int32_t nk = map->n_map_kf, npt = map->points.n, nls = map->lines.n;
        hipLaunchKernelGGL(k_lm_all_flags, dim3(map_tiles((int64_t)nk + npt + nls)), dim3(MAP_TILE), 0, s, nk, map->kf_valid, npt,
                           (const uint8_t*)map->points.valid, nls, (const uint8_t*)map->lines.valid, lm->d.kf_local, lm->d.pt_local,
                           lm->d.ls_local);
    });
}

int plslam_local_map_candidates(plslam_local_map* lm, const plslam_map_index* map, int32_t kf2_idx)
{
    PLSLAM_REQUIRE(lm && !lm->st.check_candidates(map), PLSLAM_EINVAL);
    std::lock_guard<std::mutex> lk(lm->ctx->mu);
    DeviceGuard dg_(lm->ctx->device);
    hipStream_t s = lm->ctx->stream;
    const MapKindSrc P = map_kind_src(map->points, 0), L = map_kind_src(map->lines, 1);
    if ((int64_t)P.n + L.n == 0) return PLSLAM_OK;
    StreamSyncOnError guard(s);
    hipLaunchKernelGGL(k_lm_candidates, dim3(map_tiles((int64_t)P.n + L.n)), dim3(MAP_TILE), 0, s, P, L, (const uint8_t*)lm->d.pt_local,
                       (const uint8_t*)lm->d.ls_local, kf2_idx, lm->d.pt_candidate, lm->d.ls_candidate);
    PLSLAM_HIP_CHECK(hipGetLastError());
    PLSLAM_HIP_CHECK(hipStreamSynchronize(s));
    guard.dismiss();
    return PLSLAM_OK;
}

int plslam_local_map_gather(plslam_local_map* lm, const plslam_map_index* map, plslam_local_map_counts* counts)
{
    PLSLAM_REQUIRE(lm && !lm->st.check_gather(map, counts), PLSLAM_EINVAL);
    std::lock_guard<std::mutex> lk(lm->ctx->mu);
    DeviceGuard dg_(lm->ctx->device);
    hipStream_t s = lm->ctx->stream;
    lm->st.begin_gather();
    StreamSyncOnError guard(s);
    const MapKindSrc P = map_kind_src(map->points, 0), L = map_kind_src(map->lines, 1);
    const int32_t nk = map->n_map_kf;
    const LocalMapLayout& Y = lm->lay;
    int32_t *kf_inv = lm->at<int32_t>(LM_KF_INV), *pt_off = lm->at<int32_t>(LM_PT_OFF), *ls_off = lm->at<int32_t>(LM_LS_OFF), *cnt = lm->cnt();
    PLSLAM_HIP_CHECK(hipMemsetAsync(lm->at<uint32_t>(LM_PART), 0, Y.part_words * 4, s));
    hipLaunchKernelGGL(k_lm_compact_kf, dim3((unsigned)Y.chain_words[LM_CHAIN_KF]), dim3(MAP_TILE), 0, s, nk, map->kf_valid,
                       (const uint8_t*)lm->d.kf_local, map->x_kf_w, lm->d.kf_list, kf_inv, lm->d.X_aux, cnt, lm->chain(LM_CHAIN_KF));
    hipLaunchKernelGGL(k_lm_compact_lm, dim3((unsigned)Y.chain_words[LM_CHAIN_PT]), dim3(MAP_TILE), 0, s, P, 0, (const uint8_t*)lm->d.pt_local,
                       lm->d.pt_list, pt_off, lm->d.X_aux, cnt, lm->chain(LM_CHAIN_PT), lm->chain(LM_CHAIN_PT_OBS));
    hipLaunchKernelGGL(k_lm_compact_lm, dim3((unsigned)Y.chain_words[LM_CHAIN_LS]), dim3(MAP_TILE), 0, s, L, 1, (const uint8_t*)lm->d.ls_local,
                       lm->d.ls_list, ls_off, lm->d.X_aux, cnt, lm->chain(LM_CHAIN_LS), lm->chain(LM_CHAIN_LS_OBS));
    const ExpandOut op{lm->d.pt_obs, lm->d.pt_lm_loc, lm->d.pt_kf_loc, lm->d.pt_pose_slot, lm->d.pt_obs_uv, lm->d.pt_list, pt_off};
    const ExpandOut ol{lm->d.ls_obs, lm->d.ls_lm_loc, lm->d.ls_kf_loc, lm->d.ls_pose_slot, lm->d.ls_l_obs, lm->d.ls_list, ls_off};
    hipLaunchKernelGGL(k_lm_expand, dim3(map_tiles((int64_t)P.n_obs + L.n_obs)), dim3(MAP_TILE), 0, s, P, L, op, ol, nk,
                       (const int32_t*)kf_inv, (const int32_t*)cnt, lm->pinned_dev());
    PLSLAM_HIP_CHECK(hipGetLastError());
    PLSLAM_HIP_CHECK(hipStreamSynchronize(s));
    guard.dismiss();
    lm->st.end_gather(lm->pin.as<int32_t>(), counts);
    return PLSLAM_OK;
}

int plslam_local_map_cull(plslam_local_map* lm, const plslam_map_index* map, int32_t max_kf_idx, int32_t min_lm_obs,
                          plslam_local_map_counts* counts)
{
    PLSLAM_REQUIRE(lm && !lm->st.check_cull(map, counts), PLSLAM_EINVAL);
    std::lock_guard<std::mutex> lk(lm->ctx->mu);
    DeviceGuard dg_(lm->ctx->device);
    hipStream_t s = lm->ctx->stream;
    const MapKindSrc P = map_kind_src(map->points, 0), L = map_kind_src(map->lines, 1);
    lm->st.begin_cull(counts);
    if ((int64_t)P.n + L.n == 0) return PLSLAM_OK;
    StreamSyncOnError guard(s);
    // (the two counts and the ticket: C_PT_REM, C_LS_REM ... C_CULL_DONE are consecutive words)
    int32_t* cnt = lm->cnt();
    PLSLAM_HIP_CHECK(hipMemsetAsync(cnt + C_PT_REM, 0, (C_CULL_DONE - C_PT_REM + 1) * 4, s));
    const Publish pub{cnt + C_CULL_DONE, cnt + C_PT_REM, lm->pinned_dev() + C_PT_REM, 2};
    hipLaunchKernelGGL(k_lm_cull, dim3(map_tiles((int64_t)P.n + L.n)), dim3(MAP_TILE), 0, s, P, L,
                       CullKind{map->points.valid, map->points.feat_idx, lm->d.pt_removed},
                       CullKind{map->lines.valid, map->lines.feat_idx, lm->d.ls_removed}, map->n_map_kf, map->kf_valid,
                       (const uint8_t*)lm->d.pt_local, (const uint8_t*)lm->d.ls_local, max_kf_idx, min_lm_obs, cnt + C_PT_REM, pub);
    PLSLAM_HIP_CHECK(hipGetLastError());
    PLSLAM_HIP_CHECK(hipStreamSynchronize(s));
    guard.dismiss();
    lm->st.end_cull(lm->pin.as<int32_t>(), counts);
    return PLSLAM_OK;
}

int plslam_local_map_apply_lba(plslam_local_map* lm, plslam_lba_plan* plan, const plslam_local_map_lba_dst* dst, double moved_th,
                               plslam_local_map_counts* counts)
{
    PLSLAM_REQUIRE(lm && plan && !lm->st.check_apply_lba(plan->ctx == lm->ctx, plan->npt, plan->nls, plan->state_valid, dst, counts),
                   PLSLAM_EINVAL);
    std::lock_guard<std::mutex> lk(lm->ctx->mu);
    DeviceGuard dg_(lm->ctx->device);
    hipStream_t s = lm->ctx->stream;
    const int32_t npt_l = lm->st.h_cnt[C_NPT], nls_l = lm->st.h_cnt[C_NLS];
    lm->st.begin_apply_lba(counts);
    if ((int64_t)npt_l + nls_l == 0) return PLSLAM_OK;
    StreamSyncOnError guard(s);
    // (the two counts and the ticket: C_PT_MOVED, C_LS_MOVED, C_APPLY_DONE are consecutive words)
    int32_t* cnt = lm->cnt();
    PLSLAM_HIP_CHECK(hipMemsetAsync(cnt + C_PT_MOVED, 0, (C_APPLY_DONE - C_PT_MOVED + 1) * 4, s));
    const ApplyKind P{lm->d.pt_list, plan->x.Xw, dst->pt_X, dst->pt_inlier, lm->d.pt_moved, npt_l, lm->st.z.npt};
    const ApplyKind L{lm->d.ls_list, plan->x.Lw, dst->ls_X, dst->ls_inlier, lm->d.ls_moved, nls_l, lm->st.z.nls};
    const Publish pub{cnt + C_APPLY_DONE, cnt + C_PT_MOVED, lm->pinned_dev() + C_PT_MOVED, 2};
    hipLaunchKernelGGL(k_lm_apply_lba<true>, dim3(map_tiles((int64_t)npt_l + nls_l)), dim3(MAP_TILE), 0, s, P, L, moved_th, cnt + C_PT_MOVED, pub);
    PLSLAM_HIP_CHECK(hipGetLastError());
    PLSLAM_HIP_CHECK(hipStreamSynchronize(s));
    guard.dismiss();
    lm->st.end_apply_lba(lm->pin.as<int32_t>(), counts);
    return PLSLAM_OK;
}

int plslam_local_map_apply_gba(plslam_local_map* lm, plslam_gba_plan* plan, const plslam_local_map_lba_dst* dst)
{
    PLSLAM_REQUIRE(lm && plan && plan->lba && !lm->st.check_apply_gba(plan->ctx == lm->ctx, plan->npt, plan->nls, plan->optimized, dst),
                   PLSLAM_EINVAL);
    std::lock_guard<std::mutex> lk(lm->ctx->mu);
    DeviceGuard dg_(lm->ctx->device);
    hipStream_t s = lm->ctx->stream;
    const int32_t npt_l = lm->st.h_cnt[C_NPT], nls_l = lm->st.h_cnt[C_NLS];
    if ((int64_t)npt_l + nls_l == 0) return PLSLAM_OK;
    StreamSyncOnError guard(s);
    const plslam_lba_plan* P_ = plan->lba;
    const ApplyKind P{lm->d.pt_list, P_->x.Xw, dst->pt_X, nullptr, nullptr, npt_l, lm->st.z.npt};
    const ApplyKind L{lm->d.ls_list, P_->x.Lw, dst->ls_X, nullptr, nullptr, nls_l, lm->st.z.nls};
    hipLaunchKernelGGL(k_lm_apply_lba<false>, dim3(map_tiles((int64_t)npt_l + nls_l)), dim3(MAP_TILE), 0, s, P, L, 0.0, (int32_t*)nullptr,
                       Publish{nullptr, nullptr, nullptr, 0});
    PLSLAM_HIP_CHECK(hipGetLastError());
    PLSLAM_HIP_CHECK(hipStreamSynchronize(s));
    guard.dismiss();
    return PLSLAM_OK;
}

int plslam_local_map_device_buffers(plslam_local_map* lm, plslam_local_map_buffers* out)
{
    PLSLAM_REQUIRE(lm && !lm->st.check_device_buffers(out), PLSLAM_EINVAL);
    *out = lm->d;
    return PLSLAM_OK;
}

int plslam_local_map_download(plslam_local_map* lm, const plslam_local_map_buffers* host)
{
    PLSLAM_REQUIRE(lm && !lm->st.check_download(host), PLSLAM_EINVAL);
    std::lock_guard<std::mutex> lk(lm->ctx->mu);
    DeviceGuard dg_(lm->ctx->device);
    DownloadItem items[LOCAL_MAP_N_BUFFERS];
    for (int i = 0; i < LOCAL_MAP_N_BUFFERS; ++i) {
        const LocalMapBuffer& e = LOCAL_MAP_BUFFERS[i];
        items[i] = DownloadItem{local_map_buffer_get(*host, e), local_map_buffer_get(lm->d, e), lm->st.download_bytes(e)};
    }
    return download_items(items, lm->ctx->stream);
}

}  // extern "C"
