// lc_fuse.hip -- MapHandler::loopClosureFuseLandmarks (src/mapHandler.cpp:4412-4687) over the device-resident CSR image of the map
// (plslam_map_index), OUT OF PLACE: the source image is read, every array of the destination is written.  The semantics, the
// deviations and the level rule are in include/plslam_hip.h; the sequential definition is tests/lc_fuse_ref.py.  Per landmark kind:
//   K68 a lane per source landmark (its list length, the state the events mutate) and per tuple: what the tuple can be from the
//       SOURCE image alone (entry flag, NULL slots, index ranges, NULL features: none of these changes during the call), the
//       features it would write
//   K69 the resolve: ONE workgroup.  An event's outcome depends only on (alive, length) of the landmarks it names as the earlier
//       events that name them left it.  Rounds: every pending event posts its number to its landmarks with an atomic min; the
//       event that is the minimum on all of its landmarks has no pending predecessor: it becomes final, records its offset o(e)
//       inside its target's list and its width, and updates the state.  The round an event becomes final in is its level, so the
//       rounds are capped at PLSLAM_LC_FUSE_MAX_LEVEL and what is left pending then refuses the call through the status word every
//       later kernel tests.  Then one pass in event order: the new landmarks' ranks, the (event, pair) offsets of K72, the last
//       writer per feature (atomic max, as K66), the counts.  Workgroup barriers only; no loop on device state without a cap.
//   K70 the new obs_ptr: a look-back scan of the final lengths (0 for a dead landmark, 2 for a new one) over n + n_new landmarks;
//       valid / inlier / X copied, the new rows computed
//   K71 the observations: a lane per SOURCE observation scatters it to its place, a lane per (tuple, side) writes what the event
//       made and its direction (zeros where it made none).  The place of entry k of landmark x: while x was fused away by event e into a, k += o(e) and x = a -- at most
//       MAX_LEVEL steps, since the killers along the chain have rising levels; then obs_ptr[x] + k.  So the list of any landmark at
//       the time of any event is a contiguous range of the destination.
//   K72 feat_idx (copy; the last acted event that names a feature wins), the anchors, and the graph: a lane per (event, pair)
//       reads the DESTINATION obs_kf ranges, int32 atomic adds into the zeroed dense delta (exact in any order)
//   K73 the counts and graph_delta to the page-locked block; kf_valid, x_kf_w and feat_ptr copied
// Atomics count and select; none decides an order.  Every output is an integer, a flag, a verbatim copy of a double or a
// fixed-order fp64 expression of correctly rounded operations.  Every index read from the image or a tuple is range-checked
// before it is used as an address.
// The host decisions -- the validation, the growth bounds, the layout of the handle's buffer, the packing of the staged block --
// are lc_fuse_plan.hpp (no HIP in it; tests/cpp/test_lc_fuse_pack.cpp); the commit the fusion shares with the insert is
// map_image.hpp's.
#include <climits>
#include <cstring>

#include "common.hpp"
#include "lc_fuse_plan.hpp"
#include "lookback_dev.hpp"
#include "map_image_dev.hpp"
#include "map_lists_plan.hpp"
#include "se3_dev.hpp"

namespace plslam {
namespace {

constexpr int LF_RES_NT = 1024;         // the resolve's one workgroup; a lane owns the events e = lane (mod LF_RES_NT): at most 64
constexpr unsigned LF_MAX_GRID = 4096;  // K72 / K73 stride over their items
constexpr int LF_MAX_LEVEL = PLSLAM_LC_FUSE_MAX_LEVEL;
static_assert(PLSLAM_LC_FUSE_MAX_TUPLES <= 64 * LF_RES_NT, "a resolve lane keeps its pending events in one 64-bit mask");
// the call counters (device words, mirrored in the page-locked block): eight per kind, then the status word
enum { W_A = 0, W_B, W_C, W_D, W_SKIP, W_OBS, W_PAIRS, W_KIND = 8, W_STATUS = 16, W_WORDS = LC_FUSE_COUNTER_WORDS };
// what a tuple can be from the source image alone
enum { SC_OFF = 0, SC_A, SC_B, SC_C, SC_D, SC_SELF, SC_NONE };

struct CallD {                          // one kind's tables and scratch (device), carved from the handle's buffer
    int32_t lines, n_map_kf, n_lc, m, c_cap;                     // c_cap: the host's bound on the new landmarks
    const uint8_t* kf_valid;
    const int32_t *lc, *tup, *eptr;
    const double *T, *P0, *o0, *P1, *o1;
    int32_t *cur_len, *killer, *head, *sc, *fw0, *fw1, *ev, *ev_off, *pair_off, *new_ev, *feat_win, *obs_src, *cnt, *status;
    double* ev_dir;
};

__device__ __forceinline__ int32_t ld(const int32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void st(int32_t* p, int32_t v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// the direction of a feature in its camera frame: P / |P|, lines (sP + eP) / |sP + eP| (:4560-4561)
__device__ __forceinline__ void cam_dir(int lines, const double* __restrict__ P, double* o)
{
    double v[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) v[a] = lines ? P[a] + P[3 + a] : P[a];
    over_norm3(v, o);
}
// ... in the world frame: (T P) / |.|, lines the midpoint 0.5 (s + e) of the transformed ends (:4608-4611)
__device__ __forceinline__ void world_dir(int lines, const double* __restrict__ T, const double* __restrict__ P, double* o)
{
    double s[3], e[3];
    xform(T, P, s);
    if (lines) {
        xform(T, P + 3, e);
#pragma unroll
        for (int a = 0; a < 3; ++a) s[a] = 0.5 * (s[a] + e[a]);
    }
    over_norm3(s, o);
}
// the entry of tuple t: the last one whose offset is at or below t (empty entries share an offset with their successor)
__device__ __forceinline__ int32_t entry_of(const CallD& C, int32_t t) { return segment_of(C.eptr, C.n_lc, t); }
// the place in the destination of entry `off` of landmark x's list (K71's chain)
__device__ __forceinline__ int64_t place(const MapKindSrc& S, const MapKindDst& D, const CallD& C, int32_t x, int64_t off)
{
    for (int it = 0; it <= LF_MAX_LEVEL && x >= 0 && x < S.n; ++it) {
        const int32_t e = C.killer[x];
        if (e < 0 || e >= C.m) break;
        off += C.ev_off[e];
        x = C.ev[6 * (size_t)e + 1];
    }
    return x >= 0 && x < D.cap ? (int64_t)D.obs_ptr[x] + off : -1;
}

// K68: the state and the static classification.  A lane per source landmark, then per tuple.
__global__ void __launch_bounds__(MAP_TILE)
k_lf_classify(MapKindSrc S, CallD C)
{
    const int64_t i = (int64_t)blockIdx.x * MAP_TILE + threadIdx.x;
    if (i < S.n) {
        C.cur_len[i] = old_len(S, (int32_t)i);
        return;
    }
    const int64_t tt = i - S.n;
    if (tt >= C.m) return;
    const int32_t t = (int32_t)tt, ent = entry_of(C, t);
    const int32_t kp = C.lc[3 * ent], kc = C.lc[3 * ent + 1], flag = C.lc[3 * ent + 2];
    const int32_t a = C.tup[4 * (size_t)t], l0 = C.tup[4 * (size_t)t + 1], b = C.tup[4 * (size_t)t + 2], l1 = C.tup[4 * (size_t)t + 3];
    int32_t sc = SC_OFF, fw0 = -1, fw1 = -1;
    if (flag == 1) {                                             // (the host checked this entry's slots: in range, distinct)
        sc = SC_NONE;
        bool skip = !C.kf_valid[kp] || !C.kf_valid[kc];
        skip = skip || (a != -1 && (a < 0 || a >= S.n)) || (b != -1 && (b < 0 || b >= S.n));
        if (!skip) {
            const bool need0 = a == -1, need1 = !(a == -1 && b != -1);
            int32_t p0, np, c0, nc;
            slot_features(S, kp, p0, np);
            slot_features(S, kc, c0, nc);
            skip = (need0 && (l0 < 0 || l0 >= np)) || (need1 && (l1 < 0 || l1 >= nc));
            if (!skip) {
                const bool f0 = need0 && S.feat_idx[p0 + l0] != PLSLAM_FEAT_NULL, f1 = need1 && S.feat_idx[c0 + l1] != PLSLAM_FEAT_NULL;
                if (a == -1 && b != -1) {
                    if (f0) { sc = SC_A; fw0 = p0 + l0; }
                } else if (a != -1 && b == -1) {
                    if (f1) { sc = SC_B; fw1 = c0 + l1; }
                } else if (a == -1) {
                    if (f0 && f1) { sc = SC_C; fw0 = p0 + l0; fw1 = c0 + l1; }
                } else if (f1) {
                    sc = a == b ? SC_SELF : SC_D;
                    fw1 = c0 + l1;
                }
            }
        }
        if (skip) atomicAdd(C.cnt + W_SKIP, 1);
    }
    C.sc[t] = sc; C.fw0[t] = fw0; C.fw1[t] = fw1;
}

// K69: the resolve.  One workgroup of LF_RES_NT lanes; lane l owns the events e = l + 1024 k, bit k of its pending mask.
__global__ void __launch_bounds__(LF_RES_NT)
k_lf_resolve(MapKindSrc S, CallD C)
{
    __shared__ uint32_t s_c[LF_RES_NT];
    __shared__ unsigned long long s_p[LF_RES_NT];
    __shared__ int32_t s_cnt[W_KIND];
    const int tid = (int)threadIdx.x;
    const int32_t m = C.m, n = S.n;
    if (tid < W_KIND) s_cnt[tid] = 0;
    // the records' defaults, and which events name a landmark at all
    unsigned long long pend = 0;
    for (int k = 0; k < 64; ++k) {
        const int32_t e = tid + k * LF_RES_NT;
        if (e >= m) break;
        const int32_t sc = C.sc[e], a = C.tup[4 * (size_t)e], b = C.tup[4 * (size_t)e + 2];
        int32_t* rec = C.ev + 6 * (size_t)e;
        st(rec + 0, sc == SC_C ? 3 : 0); st(rec + 1, -1); st(rec + 2, -1); st(rec + 3, -1); st(rec + 4, -1); st(rec + 5, sc == SC_C ? 2 : 0);
        st(C.ev_off + e, 0);
        if (sc != SC_OFF && ((a >= 0 && a < n) || (b >= 0 && b < n))) pend |= 1ull << k;
    }
    int left = 0;
    for (int round = 0; round <= LF_MAX_LEVEL; ++round) {
        left = __syncthreads_or(pend != 0);
        if (!left || round == LF_MAX_LEVEL) break;
        for (int k = 0; k < 64 && (pend >> k); ++k) {
            if (!((pend >> k) & 1)) continue;
            const int32_t e = tid + k * LF_RES_NT, a = C.tup[4 * (size_t)e], b = C.tup[4 * (size_t)e + 2];
            if (a >= 0 && a < n) atomicMin(C.head + a, e);
            if (b >= 0 && b < n) atomicMin(C.head + b, e);
        }
        __syncthreads();
        for (int k = 0; k < 64 && (pend >> k); ++k) {
            if (!((pend >> k) & 1)) continue;
            const int32_t e = tid + k * LF_RES_NT, a = C.tup[4 * (size_t)e], b = C.tup[4 * (size_t)e + 2];
            const bool na = a >= 0 && a < n, nb = b >= 0 && b < n;
            if ((na && ld(C.head + a) != e) || (nb && ld(C.head + b) != e)) continue;
            // no earlier event that names a or b is pending, and no other event touches them in this round
            const int32_t sc = C.sc[e];
            const bool va = na && S.valid[a] && ld(C.killer + a) < 0, vb = nb && S.valid[b] && ld(C.killer + b) < 0;
            int32_t code = 0, keep = -1, dead = -1, o = 0, w = 0;
            if (sc == SC_A && vb) { code = 1; keep = b; w = 1; }
            else if (sc == SC_B && va) { code = 2; keep = a; w = 1; }
            else if (sc == SC_SELF && va) atomicAdd(s_cnt + W_SKIP, 1);
            else if (sc == SC_D && va && vb) {
                w = ld(C.cur_len + b);
                if (w <= 0) { w = 0; atomicAdd(s_cnt + W_SKIP, 1); }
                else { code = 4; keep = a; dead = b; }
            }
            if (code) {
                o = ld(C.cur_len + keep);
                st(C.cur_len + keep, o + w);
                if (code == 4) { st(C.cur_len + b, 0); st(C.killer + b, e); }
                int32_t* rec = C.ev + 6 * (size_t)e;
                st(rec + 0, code); st(rec + 1, keep); st(rec + 2, dead); st(rec + 5, w);
                st(C.ev_off + e, o);
            }
            if (na) st(C.head + a, INT_MAX);
            if (nb) st(C.head + b, INT_MAX);
            pend &= ~(1ull << k);
        }
        __syncthreads();
    }
    if (left) {                                                  // an event of a level above LF_MAX_LEVEL: the call is refused
        if (tid == 0) atomicOr(C.status, 1);
        return;
    }
    // one pass in event order: lane l takes the events [l per, (l + 1) per)
    const int32_t per = (m + LF_RES_NT - 1) / LF_RES_NT, e0 = tid * per < m ? tid * per : m, e1 = e0 + per < m ? e0 + per : m;
    uint32_t nc = 0;
    unsigned long long np = 0;
    for (int32_t e = e0; e < e1; ++e) {
        const int32_t code = ld(C.ev + 6 * (size_t)e), o = ld(C.ev_off + e), w = ld(C.ev + 6 * (size_t)e + 5);
        nc += code == 3;
        np += code == 1 || code == 2 ? (unsigned long long)o + 1 : code == 3 ? 1ull : code == 4 ? (unsigned long long)o * w : 0ull;
    }
    s_c[tid] = nc;
    s_p[tid] = np;
    __syncthreads();
    for (int d = 1; d < LF_RES_NT; d <<= 1) {                    // an inclusive scan of the lanes' sums
        const uint32_t c = tid >= d ? s_c[tid - d] : 0u;
        const unsigned long long p = tid >= d ? s_p[tid - d] : 0ull;
        __syncthreads();
        s_c[tid] += c;
        s_p[tid] += p;
        __syncthreads();
    }
    const unsigned long long total = s_p[LF_RES_NT - 1];
    if (total >= (1ull << 30) || s_c[LF_RES_NT - 1] > (uint32_t)C.c_cap) {
        if (tid == 0) atomicOr(C.status, 1);
        return;
    }
    uint32_t rank = s_c[tid] - nc;
    unsigned long long poff = s_p[tid] - np;
    int32_t cnt[4] = {0, 0, 0, 0};
    for (int32_t e = e0; e < e1; ++e) {
        int32_t* rec = C.ev + 6 * (size_t)e;
        const int32_t code = ld(rec), o = ld(C.ev_off + e), w = ld(rec + 5);
        C.pair_off[e] = (int32_t)poff;
        if (!code) continue;
        ++cnt[code - 1];
        int32_t keep = ld(rec + 1);
        if (code == 3) {
            keep = n + (int32_t)rank;
            rec[1] = keep;
            rec[3] = C.lc[3 * entry_of(C, e)];
            C.cur_len[keep] = 2;
            C.new_ev[rank++] = e;
        }
        poff += code == 3 ? 1ull : code == 4 ? (unsigned long long)o * w : (unsigned long long)o + 1;
        const int32_t f0 = C.fw0[e], f1 = C.fw1[e];
        if (code != 2 && code != 4 && f0 >= 0) atomicMax(C.feat_win + f0, e + 1);
        if (code != 1 && f1 >= 0) atomicMax(C.feat_win + f1, e + 1);
    }
    for (int w = 0; w < 4; ++w)
        if (cnt[w]) atomicAdd(s_cnt + W_A + w, cnt[w]);
    __syncthreads();
    if (tid == 0) {
        for (int w = 0; w < 4; ++w) C.cnt[W_A + w] = s_cnt[W_A + w];
        atomicAdd(C.cnt + W_SKIP, s_cnt[W_SKIP]);
        C.cnt[W_PAIRS] = (int32_t)total;
        C.pair_off[m] = (int32_t)total;
    }
}

// K70: obs_ptr of the destination (an exclusive look-back scan of the final lengths over n + n_new landmarks) and the landmark
// rows: inlier / X copied, valid cleared where an event fused the landmark away; a new landmark is valid, an inlier and
// X = T_kp P0 (:4473, :4608-4609).
__global__ void __launch_bounds__(MAP_TILE)
k_lf_layout(MapKindSrc S, MapKindDst D, CallD C, uint32_t* __restrict__ part)
{
    __shared__ uint32_t s_o[MAP_NW], s_before;
    if (*C.status) return;
    const int tid = (int)threadIdx.x, b = (int)blockIdx.x;
    const int32_t i = b * MAP_TILE + tid;
    const int32_t n2 = S.n + C.cnt[W_C];
    const uint32_t c = i < n2 ? (uint32_t)C.cur_len[i] : 0u;
    const TileScan sc = lookback_offset<MAP_NW>(c, part, b, s_o, &s_before);
    if (i < n2) {
        D.obs_ptr[i] = (int32_t)sc.pos;
        if (i < S.n) {
            D.valid[i] = S.valid[i] && C.killer[i] < 0 ? S.valid[i] : 0;
            D.inlier[i] = S.inlier[i];
            for (int w = 0; w < S.dl; ++w) D.X[(size_t)S.dl * i + w] = S.X[(size_t)S.dl * i + w];
        } else {
            const int32_t e = C.new_ev[i - S.n];
            const double* T = C.T + 16 * (size_t)C.ev[6 * (size_t)e + 3];
            D.valid[i] = 1;
            D.inlier[i] = 1;
            xform(T, C.P0 + (size_t)S.dl * e, D.X + (size_t)S.dl * i);
            if (C.lines) xform(T, C.P0 + 6 * (size_t)e + 3, D.X + 6 * (size_t)i + 3);
        }
    }
    if (b == (int)gridDim.x - 1 && tid == 0) {
        D.obs_ptr[n2] = (int32_t)sc.upto;
        C.cnt[W_OBS] = (int32_t)sc.upto;
    }
}

// K71: obs_kf / obs_val / obs_src of the destination.  Lanes [0, n_obs): a source observation to its place; lanes n_obs + 2 t + w:
// the observation tuple t made on side w (A: w = 0, B: w = 1, C: both), and the position of the event's first observation.
__global__ void __launch_bounds__(MAP_TILE)
k_lf_obs(MapKindSrc S, MapKindDst D, CallD C)
{
    if (*C.status) return;
    const int64_t i = (int64_t)blockIdx.x * MAP_TILE + threadIdx.x;
    const int32_t total = C.cnt[W_OBS] < D.obs_cap ? C.cnt[W_OBS] : D.obs_cap;
    int64_t pos = -1;
    int32_t kf = -1, tag = 0;
    const double* val = nullptr;
    if (i < S.n_obs) {
        if (S.n <= 0) return;
        const int32_t j = (int32_t)i, x = segment_of(S.obs_ptr, S.n, j), k = j - S.obs_ptr[x];
        if (k < 0 || k >= old_len(S, x)) return;
        pos = place(S, D, C, x, k);
        kf = S.obs_kf[j];
        val = S.obs_val + (size_t)S.dv * j;
        tag = j;
    } else {
        const int64_t u = i - S.n_obs;
        if (u >= 2 * (int64_t)C.m) return;
        const int32_t t = (int32_t)(u >> 1), w = (int32_t)(u & 1);
        int32_t* rec = C.ev + 6 * (size_t)t;
        const int32_t code = rec[0], ent = entry_of(C, t);
        // the direction of the observation this side made: A / B in the camera frame, C in the world frame; zeros otherwise
        double dir[3] = {0.0, 0.0, 0.0};
        const double* Pw = (w ? C.P1 : C.P0) + (size_t)S.dl * t;
        if ((code == 1 && w == 0) || (code == 2 && w == 1)) cam_dir(C.lines, Pw, dir);
        else if (code == 3) world_dir(C.lines, C.T + 16 * (size_t)C.lc[3 * ent + w], Pw, dir);
#pragma unroll
        for (int a = 0; a < 3; ++a) C.ev_dir[6 * (size_t)t + 3 * w + a] = dir[a];
        if (!code) return;
        const int64_t first = code == 3 ? (int64_t)D.obs_ptr[rec[1]] : place(S, D, C, rec[1], C.ev_off[t]);
        if (w == 0) rec[4] = first >= 0 && first < total ? (int32_t)first : -1;
        if (code == 4 || (code == 1 && w == 1) || (code == 2 && w == 0)) return;
        pos = code == 3 ? first + w : first;
        kf = C.lc[3 * ent + w];
        val = (w ? C.o1 : C.o0) + (size_t)S.dv * t;
        tag = -1 - (2 * t + w);
    }
    if (pos < 0 || pos >= total) return;
    D.obs_kf[pos] = kf;
    C.obs_src[pos] = tag;
    for (int w = 0; w < S.dv; ++w) D.obs_val[(size_t)S.dv * pos + w] = val[w];
}

// K72: feat_idx, the anchors and the graph; the kernel strides over n_feat features, m events and the (event, pair) items.
// Pair q of event e -- A / B: entry q of the target's list at the time, [first - o, first], against the other keyframe; C: (kp,
// kc); D: entry q / w of a's first o entries against entry q % w of the w appended ones.
__global__ void __launch_bounds__(MAP_TILE)
k_lf_feat_graph(MapKindSrc S, MapKindDst D, CallD C, int32_t* __restrict__ graph)
{
    if (*C.status) return;
    const int32_t total = C.cnt[W_OBS] < D.obs_cap ? C.cnt[W_OBS] : D.obs_cap, nk = C.n_map_kf;
    const int64_t n_items = (int64_t)S.n_feat + C.m + C.cnt[W_PAIRS], stride = (int64_t)gridDim.x * MAP_TILE;
    for (int64_t it = (int64_t)blockIdx.x * MAP_TILE + threadIdx.x; it < n_items; it += stride) {
        if (it < S.n_feat) {
            int32_t v = S.feat_idx[it];
            const int32_t w = C.feat_win[it];
            if (w > 0 && w <= C.m) v = C.ev[6 * (size_t)(w - 1) + 1];
            D.feat_idx[it] = v;
            continue;
        }
        if (it < (int64_t)S.n_feat + C.m) {
            int32_t* rec = C.ev + 6 * (size_t)(it - S.n_feat);
            if (rec[0] == 4) rec[3] = rec[4] >= 0 && rec[4] < total ? D.obs_kf[rec[4]] : -1;
            continue;
        }
        const int32_t p = (int32_t)(it - S.n_feat - C.m), e = segment_of(C.pair_off, C.m, p), q = p - C.pair_off[e];
        const int32_t* rec = C.ev + 6 * (size_t)e;
        const int32_t code = rec[0], first = rec[4], o = C.ev_off[e], w = rec[5], ent = entry_of(C, e);
        const int32_t kp = C.lc[3 * ent], kc = C.lc[3 * ent + 1];
        int32_t gi = -1, gj = -1;
        if (code == 3) { gi = kp; gj = kc; }
        else if (first >= o && q >= 0) {
            const int64_t a0 = (int64_t)first - o;
            if (code == 4 && w > 0) {
                const int64_t pi = a0 + q / w, pj = (int64_t)first + q % w;
                if (pi < total && pj < total) { gi = D.obs_kf[pi]; gj = D.obs_kf[pj]; }
            } else if ((code == 1 || code == 2) && a0 + q < total) {
                gi = D.obs_kf[a0 + q];
                gj = code == 1 ? kc : kp;
            }
        }
        if (gi >= 0 && gi < nk && gj >= 0 && gj < nk) {
            atomicAdd(graph + (size_t)gi * nk + gj, 1);
            atomicAdd(graph + (size_t)gj * nk + gi, 1);
        } else atomicAdd(C.cnt + W_SKIP, 1);
    }
}

// one kind's tables and scratch: every slice of the plan's layout as the typed pointer the kernels take
CallD call_of(const LcFusePlan& P, int k, const uint8_t* kf_valid, char* d)
{
    const LcFuseKindPlan& K = P.k[k];
    const char* st_ = d + P.stage_off;
    int32_t* cnt = slice_at<int32_t>(d, P.d_cnt);
    CallD C{};
    C.lines = k; C.n_map_kf = P.nk; C.n_lc = P.n_lc; C.m = K.m; C.c_cap = K.cC;
    C.kf_valid = kf_valid;
    C.lc = slice_at<int32_t>(st_, P.o_lc); C.tup = slice_at<int32_t>(st_, K.o_tup); C.eptr = slice_at<int32_t>(st_, K.o_eptr);
    C.T = slice_at<double>(st_, P.o_T);
    C.P0 = slice_at<double>(st_, K.o_P0); C.o0 = slice_at<double>(st_, K.o_o0);
    C.P1 = slice_at<double>(st_, K.o_P1); C.o1 = slice_at<double>(st_, K.o_o1);
    C.cur_len = slice_at<int32_t>(d, K.d_len); C.killer = slice_at<int32_t>(d, K.d_killer); C.head = slice_at<int32_t>(d, K.d_head);
    C.sc = slice_at<int32_t>(d, K.d_sc); C.fw0 = slice_at<int32_t>(d, K.d_fw0); C.fw1 = slice_at<int32_t>(d, K.d_fw1);
    C.ev = slice_at<int32_t>(d, K.d_ev); C.ev_off = slice_at<int32_t>(d, K.d_off); C.pair_off = slice_at<int32_t>(d, K.d_pair);
    C.new_ev = slice_at<int32_t>(d, K.d_nev); C.feat_win = slice_at<int32_t>(d, K.d_win); C.obs_src = slice_at<int32_t>(d, K.d_osrc);
    C.cnt = cnt + W_KIND * k; C.status = cnt + W_STATUS; C.ev_dir = slice_at<double>(d, K.d_dir);
    return C;
}

struct KfCopy {                          // what K73 copies from the source image where the destination has its own array
    int32_t nk;
    const uint8_t* kf_valid; uint8_t* kf_valid_d;
    const double* x; double* x_d;
    const int32_t* fp[2]; int32_t* fp_d[2];
};

// what K73 copies: the keyframe arrays and feat_ptr, where the destination has an array of its own
KfCopy kf_copy_of(const plslam_map_index& src, const plslam_map_index& dst)
{
    const plslam_map_landmarks *S[2] = {&src.points, &src.lines}, *D[2] = {&dst.points, &dst.lines};
    KfCopy kc{};
    kc.nk = src.n_map_kf;
    kc.kf_valid = src.kf_valid; kc.kf_valid_d = dst.kf_valid != src.kf_valid ? (uint8_t*)dst.kf_valid : nullptr;
    kc.x = src.x_kf_w; kc.x_d = dst.x_kf_w != src.x_kf_w ? (double*)dst.x_kf_w : nullptr;
    for (int k = 0; k < 2; ++k) {
        kc.fp[k] = S[k]->feat_ptr;
        kc.fp_d[k] = S[k]->n_feat > 0 && D[k]->feat_ptr != S[k]->feat_ptr ? (int32_t*)D[k]->feat_ptr : nullptr;
    }
    return kc;
}

// K73: the call's last kernel: the counters and the graph to the page-locked block; kf_valid / x_kf_w / feat_ptr copied
__global__ void __launch_bounds__(MAP_TILE)
k_lf_publish(const int32_t* __restrict__ cnt, const int32_t* __restrict__ graph, KfCopy K, int32_t* __restrict__ pinned, int32_t with_graph)
{
    const int64_t g = (int64_t)blockIdx.x * MAP_TILE + threadIdx.x, stride = (int64_t)gridDim.x * MAP_TILE;
    const bool ok = cnt[W_STATUS] == 0;
    if (g < W_WORDS) pinned[g] = cnt[g];
    if (!ok) return;
    if (with_graph)
        for (int64_t i = g; i < (int64_t)K.nk * K.nk; i += stride) pinned[W_WORDS + i] = graph[i];
    for (int64_t i = g; i < K.nk; i += stride)
        if (K.kf_valid_d) K.kf_valid_d[i] = K.kf_valid[i];
    for (int64_t i = g; i < 6 * (int64_t)K.nk; i += stride)
        if (K.x_d) K.x_d[i] = K.x[i];
    for (int k = 0; k < 2; ++k)
        for (int64_t i = g; i <= K.nk; i += stride)
            if (K.fp_d[k]) K.fp_d[k][i] = K.fp[k][i];
}

}  // namespace
}  // namespace plslam

using namespace plslam;

struct plslam_lc_fuse {
    plslam_ctx* ctx = nullptr;
    DevBuf buf;
    HostBuf pin;                                 // W_WORDS counters, the graph where it was asked for, then the staged block
    bool done = false;
    plslam_lc_fuse_buffers d = {};
    int32_t m[2] = {0, 0}, n_obs[2] = {0, 0}, nk = 0;
    ListsRecords lists;                          // what plslam_lc_fuse_carry needs of the last run
};

const ListsRecords* plslam::lc_fuse_lists_records(plslam_lc_fuse* lf, plslam_ctx** ctx)
{
    if (!lf) return nullptr;
    *ctx = lf->ctx;
    return &lf->lists;
}

extern "C" {

int plslam_lc_fuse_create(plslam_ctx* ctx, plslam_lc_fuse** out)
{
    PLSLAM_REQUIRE(ctx && out, PLSLAM_EINVAL);
    *out = new plslam_lc_fuse();
    (*out)->ctx = ctx;
    return PLSLAM_OK;
}

void plslam_lc_fuse_destroy(plslam_lc_fuse* lf)
{
    if (!lf) return;
    release_handle_buffers(lf->ctx, lf->buf, lf->pin);
    delete lf;
}

int plslam_lc_fuse_run(plslam_lc_fuse* lf, const plslam_map_index* src, plslam_map_insert_dst* dst, int32_t n_lc,
                       const int32_t* lc_idx, const double* T_kf_w, const plslam_lc_fuse_kind* points,
                       const plslam_lc_fuse_kind* lines, int32_t* graph_delta, plslam_lc_fuse_counts* counts)
{
    // ---- validate everything (lc_fuse_plan.hpp), then commit once ----
    PLSLAM_REQUIRE(lf && counts, PLSLAM_EINVAL);
    LcFusePlan P;
    int rc = lc_fuse_plan(src, dst, n_lc, lc_idx, T_kf_w, points, lines, &P);
    if (rc) {
        set_last_error("plslam_lc_fuse_run: refused: %s", P.why);
        return rc;
    }
    const plslam_map_landmarks* S[2] = {&src->points, &src->lines};
    plslam_map_landmarks* Dk[2] = {&dst->map.points, &dst->map.lines};
    const int32_t cap[2] = {dst->pt_cap, dst->ls_cap}, obs_cap[2] = {dst->pt_obs_cap, dst->ls_obs_cap};
    const int32_t nk = P.nk;
    std::lock_guard<std::mutex> lk(lf->ctx->mu);
    DeviceGuard dg_(lf->ctx->device);
    hipStream_t s = lf->ctx->stream;
    lf->done = false;
    lf->lists.valid = false;
    if ((rc = lf->buf.reserve(P.total + 256))) return rc;
    const size_t res_bytes = P.res_bytes(graph_delta != nullptr);
    if ((rc = lf->pin.reserve(res_bytes + P.stage_bytes))) return rc;
    PLSLAM_REQUIRE(lf->pin.dev, PLSLAM_ENOTSUP);                 // the counters are written where the host reads them
    char* d = lf->buf.as<char>();
    char* staged = lf->pin.as<char>() + res_bytes;
    lc_fuse_pack(P, lc_idx, T_kf_w, staged);
    StreamSyncOnError guard(s);
    for (const FillRegion& f : P.fill) PLSLAM_HIP_CHECK(hipMemsetAsync(d + f.off, f.byte, f.bytes, s));
    PLSLAM_HIP_CHECK(hipMemcpyAsync(d + P.stage_off, staged, P.stage_bytes, hipMemcpyHostToDevice, s));
    int32_t* cnt = slice_at<int32_t>(d, P.d_cnt);
    int32_t* graph = slice_at<int32_t>(d, P.d_graph);
    MapKindSrc Sd[2];
    MapKindDst Dd[2];
    CallD C[2];
    for (int k = 0; k < 2; ++k) {
        Sd[k] = map_kind_src(*S[k], k);
        Dd[k] = map_kind_dst(*Dk[k], cap[k], obs_cap[k]);
        C[k] = call_of(P, k, src->kf_valid, d);
    }
    // both kinds are resolved before anything of the destination is written: a refusal leaves it untouched
    for (int k = 0; k < 2; ++k) hipLaunchKernelGGL(k_lf_classify, dim3(map_tiles((int64_t)S[k]->n + P.k[k].m)), dim3(MAP_TILE), 0, s, Sd[k], C[k]);
    for (int k = 0; k < 2; ++k) hipLaunchKernelGGL(k_lf_resolve, dim3(1), dim3(LF_RES_NT), 0, s, Sd[k], C[k]);
    for (int k = 0; k < 2; ++k) {
        hipLaunchKernelGGL(k_lf_layout, dim3(P.k[k].w_lm), dim3(MAP_TILE), 0, s, Sd[k], Dd[k], C[k], slice_at<uint32_t>(d, P.k[k].d_part));
        hipLaunchKernelGGL(k_lf_obs, dim3(map_tiles((int64_t)S[k]->n_obs + 2 * (int64_t)P.k[k].m)), dim3(MAP_TILE), 0, s, Sd[k], Dd[k], C[k]);
        const unsigned g = map_tiles((int64_t)S[k]->n_feat + S[k]->n_obs + 4 * (int64_t)P.k[k].m);
        hipLaunchKernelGGL(k_lf_feat_graph, dim3(g < LF_MAX_GRID ? g : LF_MAX_GRID), dim3(MAP_TILE), 0, s, Sd[k], Dd[k], C[k], graph);
    }
    const KfCopy kc = kf_copy_of(*src, dst->map);
    const unsigned gp = map_tiles(graph_delta ? (int64_t)nk * nk : nk + 1);
    hipLaunchKernelGGL(k_lf_publish, dim3(gp < 256u ? gp : 256u), dim3(MAP_TILE), 0, s, (const int32_t*)cnt, (const int32_t*)graph, kc,
                       (int32_t*)lf->pin.dev, graph_delta ? 1 : 0);
    PLSLAM_HIP_CHECK(hipGetLastError());
    PLSLAM_HIP_CHECK(hipStreamSynchronize(s));
    guard.dismiss();
    const int32_t* r = lf->pin.as<int32_t>();
    if (r[W_STATUS]) {
        set_last_error("plslam_lc_fuse_run: refused: an event's level is above PLSLAM_LC_FUSE_MAX_LEVEL (or its pairs beyond 2^30)");
        return PLSLAM_ERANGE;
    }
    if (graph_delta) memcpy(graph_delta, r + W_WORDS, (size_t)nk * nk * 4);
    plslam_lc_fuse_kind_counts* out[2] = {&counts->points, &counts->lines};
    MapCommitKind done[2];
    for (int k = 0; k < 2; ++k) {
        const int32_t* w = r + W_KIND * k;
        *out[k] = plslam_lc_fuse_kind_counts{w[W_A], w[W_B], w[W_C], w[W_D], w[W_C], w[W_D], w[W_SKIP]};
        lf->m[k] = P.k[k].m;
        lf->n_obs[k] = w[W_OBS] < obs_cap[k] ? w[W_OBS] : obs_cap[k];
        done[k] = MapCommitKind{w[W_C], lf->n_obs[k], P.k[k].m, {P.k[k].m, P.k[k].m}, C[k].ev, C[k].ev_dir, C[k].obs_src};
    }
    map_commit(*src, dst->map, done, 0, 1, lf->d, lf->lists);
    lf->nk = nk;
    lf->d.graph_delta = graph;
    lf->d.stream = (void*)s;
    lf->done = true;
    return PLSLAM_OK;
}

int plslam_lc_fuse_device_buffers(plslam_lc_fuse* lf, plslam_lc_fuse_buffers* out)
{
    PLSLAM_REQUIRE(lf && out && lf->done, PLSLAM_EINVAL);
    *out = lf->d;
    return PLSLAM_OK;
}

int plslam_lc_fuse_download(plslam_lc_fuse* lf, const plslam_lc_fuse_buffers* host)
{
    PLSLAM_REQUIRE(lf && host && lf->done, PLSLAM_EINVAL);
    std::lock_guard<std::mutex> lk(lf->ctx->mu);
    DeviceGuard dg_(lf->ctx->device);
    const DownloadItem items[] = {{host->pt_ev, lf->d.pt_ev, (size_t)lf->m[0] * 24}, {host->pt_dir, lf->d.pt_dir, (size_t)lf->m[0] * 48},
                                  {host->ls_ev, lf->d.ls_ev, (size_t)lf->m[1] * 24}, {host->ls_dir, lf->d.ls_dir, (size_t)lf->m[1] * 48},
                                  {host->pt_obs_src, lf->d.pt_obs_src, (size_t)lf->n_obs[0] * 4},
                                  {host->ls_obs_src, lf->d.ls_obs_src, (size_t)lf->n_obs[1] * 4},
                                  {host->graph_delta, lf->d.graph_delta, (size_t)lf->nk * lf->nk * 4}};
    return download_items(items, lf->ctx->stream);
}

}  // extern "C"
