// map_insert.hip -- the four insertion loops of MapHandler::addKeyFrame (src/mapHandler.cpp: matchKF2KFPoints :280-360,
// matchKF2KFLines :428-527, matchMap2KFPoints :601-629, matchMap2KFLines :716-749) over the device-resident CSR image of the map
// (plslam_map_index), OUT OF PLACE: the source image is read, every array of the destination is written.  Per landmark kind:
//   K63 the event list: a lane per table entry classifies it from the SOURCE image (no event reads what another one writes: the
//       keyframe-1 features are written by their own event only, keyframe 2's are never read as landmark indices), one stable
//       compaction with three look-back chains (events, new landmarks, (event, old observation) pairs); the event records and
//       directions; integer atomics COUNT the appended observations per landmark and keep the smallest / largest event number
//       per landmark / per keyframe-2 feature -- none of them decides an order
//   K64 the new obs_ptr: a look-back scan over n + n_new landmarks; valid / inlier / X copied, the new rows computed
//   K65 obs_kf / obs_val / obs_src: a lane per OUTPUT observation, its landmark by bisection (K61); the old entry copied or the
//       event's written; obs_src says which (the records plslam_map_insert_carry gathers the side lists by) -- the k-th event of a landmark is found by walking the event list from the landmark's first event, in event order
//   K66 feat_idx (copy; the last event of a keyframe-2 feature wins; a new landmark's keyframe-1 feature) and row_delta: a lane
//       per (event, old observation), int32 atomic adds
//   K67 the counts and row_delta to the page-locked block the host reads
// Every output is an integer, a flag, a verbatim copy of a double or a fixed-order fp64 expression of correctly rounded
// operations: bit-exact against the sequential restatement (tests/map_insert_ref.py).  Every index read from the image or a
// table is range-checked before it is used as an address.
// The host decisions -- the argument checks, the growth bounds, the launch geometry, the layout of the handle's buffer, the packing
// of the staged block -- are map_insert_plan.hpp (no HIP in it; tests/cpp/test_map_insert_plan.cpp); the commit the insert shares
// with the landmark fusion is map_image.hpp's.
#include <cstring>

#include "common.hpp"
#include "lookback_dev.hpp"
#include "map_image_dev.hpp"
#include "map_insert_plan.hpp"
#include "map_lists_plan.hpp"
#include "se3_dev.hpp"

namespace plslam {
namespace {

constexpr unsigned MI_MAX_GRID = 4096;  // K66 strides over its items
// the call counters (device words, mirrored in the page-locked block): four per kind
enum { W_EV = 0, W_NEW, W_PAIRS, W_OBS, W_KIND = 4, W_WORDS = MAP_INSERT_COUNTER_WORDS };
enum { MODE_KF2KF = MAP_INSERT_KF2KF, MODE_MAP2KF = MAP_INSERT_MAP2KF };

struct CallD {                          // one kind's tables and scratch (device), carved from the handle's buffer
    int32_t mode, lines, n_map_kf, kf1, kf2, n_tab, n_prev, n_curr, e_cap;
    const double* T;                    // T_kf1_w, T_kf2_w: 2 x 16
    const int32_t* tab;
    const double *P1, *o1, *P2, *o2;
    int32_t *i1_lm, *ev, *pair_off, *new_ev, *app_cnt, *head, *feat_win, *cnt, *obs_src;
    double* ev_dir;
};

// 0.5 * (sP + eP) of a line feature (6 doubles)
__device__ __forceinline__ void midpoint(const double* __restrict__ se, double m[3])
{
#pragma unroll
    for (int a = 0; a < 3; ++a) m[a] = 0.5 * (se[a] + se[3 + a]);
}

// K63: the event list.  A lane per table entry.
__global__ void __launch_bounds__(MAP_TILE)
k_mi_events(MapKindSrc S, CallD C, uint32_t* __restrict__ part_e, uint32_t* __restrict__ part_n, uint32_t* __restrict__ part_p)
{
    __shared__ uint32_t s_e[MAP_NW], s_n[MAP_NW], s_p[MAP_NW], s_before_e, s_before_n, s_before_p;
    const int tid = (int)threadIdx.x, lane = tid & 63, wv = tid >> 6, b = (int)blockIdx.x;
    const int32_t i1 = b * MAP_TILE + tid;
    bool ev = false, nw = false;
    int32_t lm = -1, i2 = -1;
    uint32_t pairs = 0;
    if (i1 < C.n_tab) {
        i2 = C.tab[i1];
        if (i2 >= 0) {
            int32_t f0, nf;
            slot_features(S, C.kf2, f0, nf);
            const int32_t f2 = i2 < nf && i2 < C.n_curr ? S.feat_idx[f0 + i2] : PLSLAM_FEAT_NULL;
            if (f2 != PLSLAM_FEAT_NULL) {
                if (C.mode == MODE_KF2KF) {
                    slot_features(S, C.kf1, f0, nf);
                    const int32_t f1 = i1 < nf && i1 < C.n_prev ? S.feat_idx[f0 + i1] : PLSLAM_FEAT_NULL;
                    if (f1 == -1) ev = nw = true;                                           // :291 / :439
                    else if (f1 >= 0 && f1 < S.n && S.valid[f1]) { ev = true; lm = f1; }    // :333 / :493
                } else if (i1 < S.n) {                                                      // :615 / :731: no validity check
                    ev = true;
                    lm = i1;
                }
            }
        }
    }
    if (ev) pairs = nw ? 1u : (uint32_t)old_len(S, lm);       // (a new landmark's pair: full_graph[kf2][kf1]++)
    const uint64_t me = __ballot(ev), mn = __ballot(nw);
    const uint32_t incl = wave_inclusive_sum(pairs);
    if (lane == 0) { s_e[wv] = (uint32_t)__popcll(me); s_n[wv] = (uint32_t)__popcll(mn); }
    if (lane == 63) s_p[wv] = incl;
    __syncthreads();                                            // (one barrier for the three chains)
    uint32_t own_e, in_e, own_n, in_n, own_p, in_p;
    waves_before_and_all<MAP_NW>(s_e, wv, in_e, own_e);
    waves_before_and_all<MAP_NW>(s_n, wv, in_n, own_n);
    waves_before_and_all<MAP_NW>(s_p, wv, in_p, own_p);
    const uint32_t before_e = lookback_exclusive(part_e, b, own_e, &s_before_e);
    const uint32_t before_n = lookback_exclusive(part_n, b, own_n, &s_before_n);
    const uint32_t before_p = lookback_exclusive(part_p, b, own_p, &s_before_p);
    const uint64_t below = (1ull << lane) - 1ull;
    const int32_t e = (int32_t)(before_e + in_e + (uint32_t)__popcll(me & below));
    const int32_t r = (int32_t)(before_n + in_n + (uint32_t)__popcll(mn & below));
    if (nw) lm = S.n + r;
    if (C.mode == MODE_KF2KF && i1 < C.n_tab) C.i1_lm[i1] = nw && e < C.e_cap ? lm : -1;
    if (ev && e < C.e_cap) {
        int32_t* rec = C.ev + 4 * (size_t)e;
        rec[0] = lm; rec[1] = i1; rec[2] = i2; rec[3] = nw ? 1 : 0;
        C.pair_off[e] = (int32_t)(before_p + in_p + incl - pairs);
        if (nw) C.new_ev[r] = e;
        else {
            atomicAdd(C.app_cnt + lm, 1);
            atomicMin(C.head + lm, e);
        }
        atomicMax(C.feat_win + i2, e + 1);
        // the observation directions
        double d1[3] = {0.0, 0.0, 0.0}, d2[3], p[3], q[3];
        const double *T1 = C.T, *T2 = C.T + 16;
        if (C.lines) {
            if (nw) {
                double sP[3], eP[3];
                xform(T1, C.P1 + 6 * (size_t)i1, sP);
                xform(T1, C.P1 + 6 * (size_t)i1 + 3, eP);
#pragma unroll
                for (int a = 0; a < 3; ++a) p[a] = 0.5 * (sP[a] + eP[a]);
                normalized3(p, d1);
            }
            midpoint(C.P2 + 6 * (size_t)i2, p);
            xform(T2, p, q);
            normalized3(q, d2);
        } else if (C.mode == MODE_MAP2KF) {
            normalized3(C.P2 + 3 * (size_t)i2, p);                                          // :608
            xform(T2, p, d2);                                                               // :618
        } else {
            if (nw) {
                xform(T1, C.P1 + 3 * (size_t)i1, p);
                normalized3(p, d1);                                                         // :299
            }
            xform(T2, C.P2 + 3 * (size_t)i2, q);
            if (nw) over_norm3(q, d2);                                                      // :311
            else normalized3(q, d2);                                                        // :338
        }
        double* d = C.ev_dir + 6 * (size_t)e;
#pragma unroll
        for (int a = 0; a < 3; ++a) { d[a] = d1[a]; d[3 + a] = d2[a]; }
    }
    if (b == (int)gridDim.x - 1 && tid == 0) {
        const int32_t n_ev = (int32_t)(before_e + own_e);
        C.cnt[W_EV] = n_ev < C.e_cap ? n_ev : C.e_cap;
        C.cnt[W_NEW] = (int32_t)(before_n + own_n) < C.e_cap ? (int32_t)(before_n + own_n) : C.e_cap;
        C.cnt[W_PAIRS] = (int32_t)(before_p + own_p);
    }
}

// K64: obs_ptr of the destination (an exclusive look-back scan of the new list lengths over n + n_new landmarks) and the
// landmark rows: valid / inlier / X copied; a new landmark is valid, an inlier and X = T_kf1_w P (:297, :445-448).
__global__ void __launch_bounds__(MAP_TILE)
k_mi_ptr(MapKindSrc S, MapKindDst D, CallD C, uint32_t* __restrict__ part)
{
    __shared__ uint32_t s_o[MAP_NW], s_before;
    const int tid = (int)threadIdx.x, b = (int)blockIdx.x;
    const int32_t i = b * MAP_TILE + tid;
    int32_t n_new = C.cnt[W_NEW];
    if (n_new > D.cap - S.n) n_new = D.cap - S.n;
    const int32_t n2 = S.n + (n_new > 0 ? n_new : 0);
    uint32_t c = 0;
    if (i < S.n) c = (uint32_t)(old_len(S, i) + C.app_cnt[i]);
    else if (i < n2) c = 2u;
    const TileScan sc = lookback_offset<MAP_NW>(c, part, b, s_o, &s_before);
    if (i < n2) {
        D.obs_ptr[i] = (int32_t)sc.pos;
        if (i < S.n) {
            D.valid[i] = S.valid[i];
            D.inlier[i] = S.inlier[i];
            for (int w = 0; w < S.dl; ++w) D.X[(size_t)S.dl * i + w] = S.X[(size_t)S.dl * i + w];
        } else {
            const int32_t i1 = C.ev[4 * (size_t)C.new_ev[i - S.n] + 1];
            D.valid[i] = 1;
            D.inlier[i] = 1;
            xform(C.T, C.P1 + (size_t)S.dl * i1, D.X + (size_t)S.dl * i);
            if (C.lines) xform(C.T, C.P1 + 6 * (size_t)i1 + 3, D.X + 6 * (size_t)i + 3);
        }
    }
    if (b == (int)gridDim.x - 1 && tid == 0) {
        D.obs_ptr[n2] = (int32_t)sc.upto;
        C.cnt[W_OBS] = (int32_t)sc.upto;
    }
}

// K65: obs_kf / obs_val of the destination: a lane per OUTPUT observation.  Its landmark by bisection of the new obs_ptr (empty
// lists share an offset with their successor: the last one at or below the lane owns it); inside the landmark's list the old
// entries come first, verbatim, then the events' in event order: the k-th event that names the landmark, counted from the
// landmark's first event (the atomics of K63 gave the count and the first event; the ORDER is the event list's).
__global__ void __launch_bounds__(MAP_TILE)
k_mi_obs(MapKindSrc S, MapKindDst D, CallD C)
{
    const int64_t t = (int64_t)blockIdx.x * MAP_TILE + threadIdx.x;
    const int32_t total = C.cnt[W_OBS], n_ev = C.cnt[W_EV];
    int32_t n_new = C.cnt[W_NEW];
    if (n_new > D.cap - S.n) n_new = D.cap - S.n;
    const int32_t n2 = S.n + (n_new > 0 ? n_new : 0);
    if (t >= total || t >= D.obs_cap || n2 <= 0) return;
    const int32_t j = (int32_t)t;
    const int32_t lm = segment_of(D.obs_ptr, n2, j), o = j - D.obs_ptr[lm];
    int32_t kf = -1, tag = INT32_MIN;                           // (tag: an event beyond every list unless found below)
    const double* val = nullptr;
    if (lm < S.n) {
        const int32_t ol = old_len(S, lm);
        if (o < ol) {
            const size_t src = (size_t)S.obs_ptr[lm] + o;
            kf = S.obs_kf[src];
            val = S.obs_val + (size_t)S.dv * src;
            tag = (int32_t)src;
        } else {
            int32_t k = o - ol, e = C.head[lm];
            for (; e >= 0 && e < n_ev; ++e)
                if (C.ev[4 * (size_t)e] == lm && k-- == 0) break;
            if (e >= 0 && e < n_ev) {
                kf = C.kf2;
                val = C.o2 + (size_t)S.dv * C.ev[4 * (size_t)e + 2];
                tag = -1 - (2 * e + 1);
            }
        }
    } else {
        const int32_t e = C.new_ev[lm - S.n];
        const int32_t* rec = C.ev + 4 * (size_t)e;
        kf = o == 0 ? C.kf1 : C.kf2;
        val = o == 0 ? C.o1 + (size_t)S.dv * rec[1] : C.o2 + (size_t)S.dv * rec[2];
        tag = -1 - (2 * e + (o == 0 ? 0 : 1));
    }
    D.obs_kf[j] = kf;
    C.obs_src[j] = tag;
    for (int w = 0; w < S.dv; ++w) D.obs_val[(size_t)S.dv * j + w] = val ? val[w] : 0.0;
}

// K66: feat_idx of the destination and row_delta; the kernel strides over n_feat features, then the (event, old observation)
// pairs.  A feature of keyframe 2 takes the landmark of the LAST event that names it (K63's atomic max of the event number);
// a feature of keyframe 1 whose event made a landmark takes that landmark (its only writer); every other feature is copied.
// A pair adds 1 to row_delta[the observing keyframe] unless that is keyframe 2 (:345, :508, :622, :742) -- int32 adds, exact in
// any order; a new landmark's single pair is keyframe 1 (:320-321).
__global__ void __launch_bounds__(MAP_TILE)
k_mi_feat_rows(MapKindSrc S, MapKindDst D, CallD C, int32_t* __restrict__ row_delta)
{
    const int32_t n_ev = C.cnt[W_EV];
    const int64_t n_items = (int64_t)S.n_feat + C.cnt[W_PAIRS], stride = (int64_t)gridDim.x * MAP_TILE;
    int32_t f1_0, nf1, f2_0, nf2;
    slot_features(S, C.kf2, f2_0, nf2);
    slot_features(S, C.kf1, f1_0, nf1);
    for (int64_t t = (int64_t)blockIdx.x * MAP_TILE + threadIdx.x; t < n_items; t += stride) {
        if (t < S.n_feat) {
            const int32_t f = (int32_t)t;
            int32_t v = S.feat_idx[f];
            if (f >= f2_0 && f - f2_0 < nf2 && f - f2_0 < C.n_curr) {
                const int32_t w = C.feat_win[f - f2_0];
                if (w > 0 && w <= n_ev) v = C.ev[4 * (size_t)(w - 1)];
            } else if (C.mode == MODE_KF2KF && f >= f1_0 && f - f1_0 < nf1 && f - f1_0 < C.n_tab) {
                const int32_t l = C.i1_lm[f - f1_0];
                if (l >= 0) v = l;
            }
            D.feat_idx[f] = v;
        } else if (n_ev > 0) {
            const int32_t p = (int32_t)(t - S.n_feat);
            const int32_t e = segment_of(C.pair_off, n_ev, p), o = p - C.pair_off[e];
            const int32_t* rec = C.ev + 4 * (size_t)e;
            int32_t kf = -1;
            if (rec[3]) kf = o == 0 ? C.kf1 : -1;
            else if (rec[0] >= 0 && rec[0] < S.n && o >= 0 && o < old_len(S, rec[0])) kf = S.obs_kf[(size_t)S.obs_ptr[rec[0]] + o];
            if (kf >= 0 && kf < C.n_map_kf && kf != C.kf2) atomicAdd(row_delta + kf, 1);
        }
    }
}

// K67: the call's last kernel: the counters and row_delta to the page-locked block
__global__ void __launch_bounds__(MAP_TILE)
k_mi_publish(const int32_t* __restrict__ cnt, const int32_t* __restrict__ row_delta, int32_t n_map_kf, int32_t* __restrict__ pinned)
{
    for (int32_t i = (int32_t)threadIdx.x; i < W_WORDS + n_map_kf; i += MAP_TILE) pinned[i] = i < W_WORDS ? cnt[i] : row_delta[i - W_WORDS];
}

}  // namespace
}  // namespace plslam

using namespace plslam;

struct plslam_map_insert {
    plslam_ctx* ctx = nullptr;
    DevBuf buf;
    HostBuf pin;                                 // W_WORDS counters + row_delta, then the staged tables
    bool done = false;
    plslam_map_insert_events d = {};
    int32_t n_ev[2] = {0, 0};
    ListsRecords lists;                          // what plslam_map_insert_carry needs of the last insert
};

namespace {

// one kind's tables and scratch: every slice of the plan's layout as the typed pointer the kernels take
CallD call_of(const MapInsertPlan& P, int k, char* d)
{
    const MapInsertKindPlan& K = P.k[k];
    CallD C{};
    C.mode = P.mode; C.lines = k; C.n_map_kf = P.nk; C.kf1 = P.kf1; C.kf2 = P.kf2;
    C.n_tab = K.n_tab; C.n_prev = K.n_prev; C.n_curr = K.n_curr; C.e_cap = K.m;
    C.T = slice_at<double>(d, P.o_T); C.tab = slice_at<int32_t>(d, K.o_tab);
    C.P1 = slice_at<double>(d, K.o_P1); C.o1 = slice_at<double>(d, K.o_o1);
    C.P2 = slice_at<double>(d, K.o_P2); C.o2 = slice_at<double>(d, K.o_o2);
    C.i1_lm = slice_at<int32_t>(d, K.o_i1lm); C.ev = slice_at<int32_t>(d, K.o_ev); C.pair_off = slice_at<int32_t>(d, K.o_pair);
    C.new_ev = slice_at<int32_t>(d, K.o_new); C.app_cnt = slice_at<int32_t>(d, K.o_app); C.head = slice_at<int32_t>(d, K.o_head);
    C.feat_win = slice_at<int32_t>(d, K.o_win); C.cnt = slice_at<int32_t>(d, P.o_cnt) + W_KIND * k; C.ev_dir = slice_at<double>(d, K.o_dir);
    C.obs_src = slice_at<int32_t>(d, K.o_osrc);
    return C;
}

int insert(plslam_map_insert* mi, int mode, const plslam_map_index* src, plslam_map_insert_dst* dst, int32_t kf1, int32_t kf2,
           const double* T1, const double* T2, const plslam_map_insert_kind* points, const plslam_map_insert_kind* lines,
           int32_t* row_delta, plslam_map_insert_counts* counts)
{
    // ---- validate everything (map_insert_plan.hpp), then commit once ----
    PLSLAM_REQUIRE(mi && row_delta && counts, PLSLAM_EINVAL);
    MapInsertPlan P;
    int rc = map_insert_plan(mode, src, dst, kf1, kf2, T1, T2, points, lines, &P);
    if (rc) {
        set_last_error("plslam_map_insert: refused: %s", P.why);
        return rc;
    }
    const plslam_map_landmarks* S[2] = {&src->points, &src->lines};
    plslam_map_landmarks* Dk[2] = {&dst->map.points, &dst->map.lines};
    const int32_t cap[2] = {dst->pt_cap, dst->ls_cap}, obs_cap[2] = {dst->pt_obs_cap, dst->ls_obs_cap};
    const int32_t nk = P.nk;
    std::lock_guard<std::mutex> lk(mi->ctx->mu);
    DeviceGuard dg_(mi->ctx->device);
    hipStream_t s = mi->ctx->stream;
    mi->done = false;
    mi->lists.valid = false;
    if ((rc = mi->buf.reserve(P.total + 256))) return rc;
    if ((rc = mi->pin.reserve(P.res_bytes + P.stage_bytes))) return rc;
    PLSLAM_REQUIRE(mi->pin.dev, PLSLAM_ENOTSUP);                 // the counters are written where the host reads them
    char* d = mi->buf.as<char>();
    char* staged = mi->pin.as<char>() + P.res_bytes;
    map_insert_pack(P, T1, T2, staged);
    StreamSyncOnError guard(s);
    for (const FillRegion& f : P.fill) PLSLAM_HIP_CHECK(hipMemsetAsync(d + f.off, f.byte, f.bytes, s));
    PLSLAM_HIP_CHECK(hipMemcpyAsync(d + P.stage_off, staged, P.stage_bytes, hipMemcpyHostToDevice, s));
    if (dst->map.kf_valid != src->kf_valid)
        PLSLAM_HIP_CHECK(hipMemcpyAsync((void*)dst->map.kf_valid, src->kf_valid, (size_t)nk, hipMemcpyDeviceToDevice, s));
    if (dst->map.x_kf_w != src->x_kf_w)
        PLSLAM_HIP_CHECK(hipMemcpyAsync((void*)dst->map.x_kf_w, src->x_kf_w, (size_t)nk * 48, hipMemcpyDeviceToDevice, s));
    int32_t* cnt = slice_at<int32_t>(d, P.o_cnt);
    int32_t* row = slice_at<int32_t>(d, P.o_row);
    MapCommitKind done[2];
    for (int k = 0; k < 2; ++k) {
        const MapInsertKindPlan& K = P.k[k];
        const plslam_map_landmarks& A = *S[k];
        plslam_map_landmarks& B = *Dk[k];
        if (A.n_feat > 0 && B.feat_ptr != A.feat_ptr)
            PLSLAM_HIP_CHECK(hipMemcpyAsync((void*)B.feat_ptr, A.feat_ptr, ((size_t)nk + 1) * 4, hipMemcpyDeviceToDevice, s));
        const MapKindSrc Sd = map_kind_src(A, k);
        const MapKindDst Dd = map_kind_dst(B, cap[k], obs_cap[k]);
        const CallD C = call_of(P, k, d);
        uint32_t* part = slice_at<uint32_t>(d, K.o_part);
        hipLaunchKernelGGL(k_mi_events, dim3(K.w_tab), dim3(MAP_TILE), 0, s, Sd, C, part, part + K.w_tab, part + 2 * K.w_tab);
        hipLaunchKernelGGL(k_mi_ptr, dim3(K.w_lm), dim3(MAP_TILE), 0, s, Sd, Dd, C, part + 3 * K.w_tab);
        if (K.need_obs > 0) hipLaunchKernelGGL(k_mi_obs, dim3(map_tiles(K.need_obs)), dim3(MAP_TILE), 0, s, Sd, Dd, C);
        const unsigned g = map_tiles((int64_t)A.n_feat + A.n_obs + K.m);
        hipLaunchKernelGGL(k_mi_feat_rows, dim3(g < MI_MAX_GRID ? g : MI_MAX_GRID), dim3(MAP_TILE), 0, s, Sd, Dd, C, row);
        done[k] = MapCommitKind{0, 0, 0, {K.n_prev, K.n_curr}, C.ev, C.ev_dir, C.obs_src};
    }
    hipLaunchKernelGGL(k_mi_publish, dim3(1), dim3(MAP_TILE), 0, s, (const int32_t*)cnt, (const int32_t*)row, nk, (int32_t*)mi->pin.dev);
    PLSLAM_HIP_CHECK(hipGetLastError());
    PLSLAM_HIP_CHECK(hipStreamSynchronize(s));
    guard.dismiss();
    const int32_t* r = mi->pin.as<int32_t>();
    memcpy(row_delta, r + W_WORDS, (size_t)nk * 4);
    plslam_map_insert_kind_counts* out[2] = {&counts->points, &counts->lines};
    for (int k = 0; k < 2; ++k) {
        const int32_t* w = r + W_KIND * k;
        *out[k] = plslam_map_insert_kind_counts{w[W_EV], w[W_NEW], w[W_EV] + w[W_NEW], P.k[k].m - w[W_EV]};
        mi->n_ev[k] = done[k].n_ev = w[W_EV];
        done[k].n_new = w[W_NEW];
        done[k].n_obs = w[W_OBS];
    }
    map_commit(*src, dst->map, done, 4, mode == MODE_KF2KF, mi->d, mi->lists);
    mi->d.stream = (void*)s;
    mi->done = true;
    return PLSLAM_OK;
}

}  // namespace

const ListsRecords* plslam::map_insert_lists_records(plslam_map_insert* mi, plslam_ctx** ctx)
{
    if (!mi) return nullptr;
    *ctx = mi->ctx;
    return &mi->lists;
}

extern "C" {

int plslam_map_insert_create(plslam_ctx* ctx, plslam_map_insert** out)
{
    PLSLAM_REQUIRE(ctx && out, PLSLAM_EINVAL);
    *out = new plslam_map_insert();
    (*out)->ctx = ctx;
    return PLSLAM_OK;
}

void plslam_map_insert_destroy(plslam_map_insert* mi)
{
    if (!mi) return;
    release_handle_buffers(mi->ctx, mi->buf, mi->pin);
    delete mi;
}

int plslam_map_insert_kf2kf(plslam_map_insert* mi, const plslam_map_index* src, plslam_map_insert_dst* dst, int32_t kf1_idx,
                            int32_t kf2_idx, const double* T_kf1_w, const double* T_kf2_w, const plslam_map_insert_kind* points,
                            const plslam_map_insert_kind* lines, int32_t* row_delta, plslam_map_insert_counts* counts)
{
    return insert(mi, MODE_KF2KF, src, dst, kf1_idx, kf2_idx, T_kf1_w, T_kf2_w, points, lines, row_delta, counts);
}

int plslam_map_insert_map2kf(plslam_map_insert* mi, const plslam_map_index* src, plslam_map_insert_dst* dst, int32_t kf2_idx,
                             const double* T_kf2_w, const plslam_map_insert_kind* points, const plslam_map_insert_kind* lines,
                             int32_t* row_delta, plslam_map_insert_counts* counts)
{
    return insert(mi, MODE_MAP2KF, src, dst, -1, kf2_idx, nullptr, T_kf2_w, points, lines, row_delta, counts);
}

int plslam_map_insert_device_buffers(plslam_map_insert* mi, plslam_map_insert_events* out)
{
    PLSLAM_REQUIRE(mi && out && mi->done, PLSLAM_EINVAL);
    *out = mi->d;
    return PLSLAM_OK;
}

int plslam_map_insert_download(plslam_map_insert* mi, const plslam_map_insert_events* host)
{
    PLSLAM_REQUIRE(mi && host && mi->done, PLSLAM_EINVAL);
    std::lock_guard<std::mutex> lk(mi->ctx->mu);
    DeviceGuard dg_(mi->ctx->device);
    const DownloadItem items[] = {{host->pt_ev, mi->d.pt_ev, (size_t)mi->n_ev[0] * 16}, {host->pt_dir, mi->d.pt_dir, (size_t)mi->n_ev[0] * 48},
                                  {host->ls_ev, mi->d.ls_ev, (size_t)mi->n_ev[1] * 16}, {host->ls_dir, mi->d.ls_dir, (size_t)mi->n_ev[1] * 48},
                                  {host->pt_obs_src, mi->d.pt_obs_src, (size_t)mi->lists.k[0].dst_obs * 4},
                                  {host->ls_obs_src, mi->d.ls_obs_src, (size_t)mi->lists.k[1].dst_obs * 4}};
    return download_items(items, mi->ctx->stream);
}

}  // extern "C"
