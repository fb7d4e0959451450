// lba_plan_dev.hip -- the LBA plan built ON THE DEVICE from device columns (plslam_lba_plan_create_dev): what
// plslam_local_map_gather leaves on the device goes into the plan without crossing PCIe, and the plan keeps no host copy of any
// list.  The lists are those of the host builders (lba_lists.hpp: build_csr, pose_max_chunks, build_schur_pairs), entry for entry:
//   K74 k_lbp_validate      a lane per observation: the range checks of plslam_lba_plan_create (a status word; what is stored is
//                           made safe, so no later kernel follows a bad index), the slot rewrite, the stored columns, the keys of
//                           the keyframe list
//   K75 k_dist_hist / K76 k_dist_scan / K77 k_dist_scatter / K78 k_dist_ptr
//                           the stable distribution (distribute_dev.hpp; the kernels and dist_enqueue: distribute.hip), used three
//                           times for the plan -- points by lm_loc, lines by lm_loc, the keyframe list by kf_loc -- and once for
//                           the Schur pairs by 2 block + kind
//   K79 k_lbp_pair_count    a lane per position of the landmark lists: the pairs (o1, .) it starts; their sum in 64 bits
//   K80 k_lbp_publish       max_chunks reduced from kf_ptr; status and counts to the page-locked block the host reads
//   K81 k_lbp_pair_emit     enumeration offsets (the look-back of lookback_dev.hpp over K79's counts), then key and pair of every
//                           (o1, o2) in build_schur_pairs' enumeration order
//   K82 k_lbp_pair_layout   per-(block, kind) counts -> blk_ptr (line pairs at a SCH_CHUNK boundary), schur_chunks, the padded total
//   K83 k_lbp_pair_place    a lane per slot of the padded pair list: the pair the distribution put there, or the null pair
// One synchronisation for the plan, one for the Schur lists (the sizes the host carves the buffers from).
#include <cstring>
#include <new>

#include "distribute_dev.hpp"
#include "lba_plan.hpp"
#include "lookback_dev.hpp"

using namespace plslam;

namespace plslam {
namespace {

constexpr int LBP_NT = 256;
// the page-locked words the builders' last kernels write
enum { W_STATUS = 0, W_NKFI, W_MAX_CHUNKS, W_PAIRS_LO, W_PAIRS_HI, W_PADDED, W_SCHUR_CHUNKS, W_WORDS = 8 };
// the device words (aux): the status, then the 64-bit pair total at an 8-byte boundary
enum { D_STATUS = 0, D_PAIRS = 2, D_WORDS = 64 };

unsigned wgs(int64_t n, int per) { return (unsigned)((n + per - 1) / per); }

struct LbpValidateArgs {
    const int32_t *pt_lm, *pt_slot, *pt_kf, *ls_lm, *ls_slot, *ls_kf;     // the caller's columns
    const double *uv, *lobs;
    int32_t *o_pt_lm, *o_pt_slot, *o_pt_kf, *o_ls_lm, *o_ls_slot, *o_ls_kf;   // the plan's
    double *o_uv, *o_lobs;
    int32_t *kf_key, *status;
    int32_t np, nl, npt, nls, nkf, n_slots, first_slot;
};

__global__ void __launch_bounds__(LBP_NT)
k_lbp_validate(const LbpValidateArgs A)
{
    const int64_t t = (int64_t)blockIdx.x * LBP_NT + threadIdx.x;
    if (t >= (int64_t)A.np + A.nl) return;
    const bool lines = t >= A.np;
    const int32_t o = (int32_t)(lines ? t - A.np : t);
    int32_t lm = g_(lines ? A.ls_lm : A.pt_lm)[o], slot = g_(lines ? A.ls_slot : A.pt_slot)[o], kf = g_(lines ? A.ls_kf : A.pt_kf)[o];
    const int32_t nlm = lines ? A.nls : A.npt;
    if (lm < 0 || lm >= nlm || kf < -1 || kf >= A.nkf || slot < 0 || slot >= A.n_slots) {
        atomicOr(A.status, 1);
        lm = 0; kf = -1; slot = 0;                          // (in range: the host has refused observations without landmarks or slots)
    }
    // slot first_slot + k holds the current estimate of local keyframe k: what the POINT rows read (:1600-1601); line rows and
    // keyframes that are not optimised keep the given slot (:1680)
    if (!lines && kf >= 0 && A.first_slot >= 0) slot = A.first_slot + kf;
    g_(lines ? A.o_ls_lm : A.o_pt_lm)[o] = lm;
    g_(lines ? A.o_ls_slot : A.o_pt_slot)[o] = slot;
    g_(lines ? A.o_ls_kf : A.o_pt_kf)[o] = kf;
    g_(A.kf_key)[t] = kf;                                   // the keyframe list: points first, then lines with ids np + o
    if (!lines) {
#pragma unroll
        for (int w = 0; w < 2; ++w) g_(A.o_uv)[2 * (size_t)o + w] = g_(A.uv)[2 * (size_t)o + w];
    } else {
#pragma unroll
        for (int w = 0; w < 3; ++w) g_(A.o_lobs)[3 * (size_t)o + w] = g_(A.lobs)[3 * (size_t)o + w];
    }
}

// the lists as the pair kernels read them
struct LbpLists {
    const int32_t *pt_ptr, *pt_ids, *pt_lm, *pt_kf, *ls_ptr, *ls_ids, *ls_lm, *ls_kf;
    int32_t np, nl, nkf;
};

// K79: position i1 of a landmark's list starts the pairs (o1, o2) with kf(o1) >= 0 and kf(o2) >= kf(o1), o2 over the WHOLE list of
// the landmark (build_schur_pairs' loops); cnt[t]: points' positions, then lines'
__global__ void __launch_bounds__(LBP_NT)
k_lbp_pair_count(const LbpLists L, int32_t* __restrict__ cnt, unsigned long long* __restrict__ total)
{
    const int64_t t = (int64_t)blockIdx.x * LBP_NT + threadIdx.x;
    int32_t c = 0;
    if (t < (int64_t)L.np + L.nl) {
        const bool lines = t >= L.np;
        const int32_t i1 = (int32_t)(lines ? t - L.np : t);
        const int32_t* __restrict__ ptr = lines ? L.ls_ptr : L.pt_ptr;
        const int32_t* __restrict__ ids = lines ? L.ls_ids : L.pt_ids;
        const int32_t* __restrict__ kf = lines ? L.ls_kf : L.pt_kf;
        const int32_t nobs = lines ? L.nl : L.np;
        const int32_t o1 = g_(ids)[i1], k1 = (uint32_t)o1 < (uint32_t)nobs ? g_(kf)[o1] : -1;    // (ids are item numbers: in range)
        if (k1 >= 0) {
            const int32_t j = g_(lines ? L.ls_lm : L.pt_lm)[o1];                                   // (validated by K74)
            const int32_t e = g_(ptr)[j + 1] < nobs ? g_(ptr)[j + 1] : nobs;
            for (int32_t i2 = g_(ptr)[j] > 0 ? g_(ptr)[j] : 0; i2 < e; ++i2) {
                const int32_t o2 = g_(ids)[i2];
                c += (uint32_t)o2 < (uint32_t)nobs && g_(kf)[o2] >= k1 ? 1 : 0;
            }
        }
        cnt[t] = c;
    }
    unsigned long long sum = (unsigned long long)c;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) sum += (unsigned long long)__shfl_xor((long long)sum, o);
    if ((threadIdx.x & 63) == 0 && sum) atomicAdd(total, sum);
}

// K80: the plan's counts to the host.  One workgroup, the plan build's last kernel.
__global__ void __launch_bounds__(LBP_NT)
k_lbp_publish(const int32_t* __restrict__ kf_ptr, int32_t nkf, const int32_t* __restrict__ words, int32_t* __restrict__ pinned)
{
    __shared__ int32_t red[LBP_NT];
    int32_t m = 0;
    for (int32_t k = (int32_t)threadIdx.x; k < nkf; k += LBP_NT) {
        const int32_t ch = (kf_ptr[k + 1] - kf_ptr[k] + POSE_CHUNK - 1) / POSE_CHUNK;
        m = ch > m ? ch : m;
    }
    red[threadIdx.x] = m;
    __syncthreads();
    for (int s = LBP_NT / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] = red[threadIdx.x] > red[threadIdx.x + s] ? red[threadIdx.x] : red[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        pinned[W_STATUS] = words[D_STATUS];
        pinned[W_NKFI] = kf_ptr[nkf];
        pinned[W_MAX_CHUNKS] = red[0];
        pinned[W_PAIRS_LO] = words[D_PAIRS];
        pinned[W_PAIRS_HI] = words[D_PAIRS + 1];
    }
}

__device__ __forceinline__ int32_t schur_block_of(int32_t k1, int32_t k2, int32_t nkf) { return k1 * nkf - k1 * (k1 - 1) / 2 + (k2 - k1); }

// K81: the enumeration offset of every position (the exclusive sum of K79's counts: a look-back chain over tiles of LBP_NT
// positions), then the position's pairs in list order: key 2 block + kind, and the pair itself.  n_enum: the arrays' length.
__global__ void __launch_bounds__(LBP_NT)
k_lbp_pair_emit(const LbpLists L, const int32_t* __restrict__ cnt, uint32_t* __restrict__ part, int32_t n_enum,
                int32_t* __restrict__ key, SchurPair* __restrict__ pair)
{
    __shared__ uint32_t s_w[LBP_NT / 64], s_before;
    const int tid = (int)threadIdx.x, b = (int)blockIdx.x;
    const int64_t t = (int64_t)b * LBP_NT + tid;
    const bool in = t < (int64_t)L.np + L.nl;
    const uint32_t c = in ? (uint32_t)cnt[t] : 0u;
    uint32_t pos = lookback_offset<LBP_NT / 64>(c, part, b, s_w, &s_before).pos;
    if (!in || c == 0) return;
    const bool lines = t >= L.np;
    const int32_t i1 = (int32_t)(lines ? t - L.np : t);
    const int32_t* __restrict__ ptr = lines ? L.ls_ptr : L.pt_ptr;
    const int32_t* __restrict__ ids = lines ? L.ls_ids : L.pt_ids;
    const int32_t* __restrict__ kf = lines ? L.ls_kf : L.pt_kf;
    const int32_t nobs = lines ? L.nl : L.np;
    const int32_t o1 = g_(ids)[i1], k1 = g_(kf)[o1];        // (c > 0: K79 found o1 in range and its keyframe optimised)
    const int32_t j = g_(lines ? L.ls_lm : L.pt_lm)[o1];
    const int32_t e = g_(ptr)[j + 1] < nobs ? g_(ptr)[j + 1] : nobs;
    for (int32_t i2 = g_(ptr)[j] > 0 ? g_(ptr)[j] : 0; i2 < e; ++i2) {
        const int32_t o2 = g_(ids)[i2];
        if ((uint32_t)o2 >= (uint32_t)nobs) continue;
        const int32_t k2 = g_(kf)[o2];
        if (k2 < k1) continue;                              // (k2 < 0 included)
        if (pos < (uint32_t)n_enum) {
            key[pos] = 2 * schur_block_of(k1, k2, L.nkf) + (lines ? 1 : 0);
            pair[pos] = SchurPair{o1, o2, j, lines ? 1 : 0};
        }
        ++pos;
    }
}

// K82: ptr2[2 B] / ptr2[2 B + 1] / ptr2[2 B + 2]: where block B's point pairs and line pairs lie in the distributed list.  A block's
// line pairs start at a SCH_CHUNK boundary behind its point pairs (lba_lists.hpp: pt_room); blk_ptr: the exclusive sum of the
// blocks' room.  One workgroup; the Schur lists' last kernel before the host carves the buffers.
__global__ void __launch_bounds__(LBP_NT)
k_lbp_pair_layout(const int32_t* __restrict__ ptr2, int32_t nblk, int32_t* __restrict__ blk_ptr, int32_t* __restrict__ pinned)
{
    __shared__ uint32_t s_w[LBP_NT / 64];
    __shared__ int32_t s_max[LBP_NT];
    const int tid = (int)threadIdx.x, lane = tid & 63, wv = tid >> 6;
    int32_t carry = 0, mx = 0;
    for (int32_t base = 0; base < nblk; base += LBP_NT) {
        const int32_t B = base + tid;
        int32_t room = 0;
        if (B < nblk) {
            const int32_t npp = ptr2[2 * B + 1] - ptr2[2 * B], nlp = ptr2[2 * B + 2] - ptr2[2 * B + 1];
            room = (nlp ? (npp + SCH_CHUNK - 1) / SCH_CHUNK * SCH_CHUNK : npp) + nlp;
            const int32_t ch = (room + SCH_CHUNK - 1) / SCH_CHUNK;
            mx = ch > mx ? ch : mx;
        }
        const uint32_t incl = wave_inclusive_sum((uint32_t)room);
        if (lane == 63) s_w[wv] = incl;
        __syncthreads();
        uint32_t before, all;
        waves_before_and_all<LBP_NT / 64>(s_w, wv, before, all);
        if (B < nblk) blk_ptr[B] = carry + (int32_t)(before + incl - (uint32_t)room);
        carry += (int32_t)all;
        __syncthreads();
    }
    s_max[tid] = mx;
    __syncthreads();
    for (int s = LBP_NT / 2; s > 0; s >>= 1) {
        if (tid < s) s_max[tid] = s_max[tid] > s_max[tid + s] ? s_max[tid] : s_max[tid + s];
        __syncthreads();
    }
    if (tid == 0) {
        blk_ptr[nblk] = carry;
        pinned[W_PADDED] = carry;
        pinned[W_SCHUR_CHUNKS] = s_max[0];
    }
}

// K83: slot s of the padded list belongs to the block whose room holds it: a point pair, a null pair {0, 0, 0, 2} between the point
// pairs and the chunk boundary, or a line pair
__global__ void __launch_bounds__(LBP_NT)
k_lbp_pair_place(const int32_t* __restrict__ blk_ptr, int32_t nblk, const int32_t* __restrict__ ptr2, const int32_t* __restrict__ ids,
                 const SchurPair* __restrict__ src, int32_t n_enum, int32_t n_padded, SchurPair* __restrict__ pairs)
{
    const int64_t s = (int64_t)blockIdx.x * LBP_NT + threadIdx.x;
    if (s >= n_padded) return;
    const int32_t B = segment_of(blk_ptr, nblk, (int32_t)s);
    const int32_t r = (int32_t)s - blk_ptr[B];
    const int32_t npp = ptr2[2 * B + 1] - ptr2[2 * B], nlp = ptr2[2 * B + 2] - ptr2[2 * B + 1];
    const int32_t room = nlp ? (npp + SCH_CHUNK - 1) / SCH_CHUNK * SCH_CHUNK : npp;
    SchurPair q{0, 0, 0, 2};
    int32_t at = -1;
    if (r < npp) at = ptr2[2 * B] + r;
    else if (r >= room && r - room < nlp) at = ptr2[2 * B + 1] + (r - room);
    if (at >= 0 && at < n_enum) {
        const int32_t e = ids[at];
        if (e >= 0 && e < n_enum) q = src[e];
    }
    pairs[s] = q;
}

LbpLists lbp_lists(const plslam_lba_plan* P)
{
    const LbaStatView& S = P->st;
    return LbpLists{S.pt_ptr, S.pt_ids, S.pt_lm, S.pt_kf, S.ls_ptr, S.ls_ids, S.ls_lm, S.ls_kf, P->np, P->nl, P->nkf};
}

// the plan build's scratch (aux): the device words, the keyframe list's keys, the distribution's buffers for every observation,
// and -- kept for the Schur lists -- the pair counts
struct PlanScratch { int32_t *words, *kf_key, *pair_cnt; DistScratch dist; size_t bytes; };
PlanScratch plan_scratch(char* base, size_t nobs)
{
    ArrCarver c{base};
    PlanScratch w{};
    w.words = c.take<int32_t>(D_WORDS * 4);
    w.kf_key = c.take<int32_t>(nobs * 4);
    w.dist.key_a = c.take<int32_t>(nobs * 4); w.dist.key_b = c.take<int32_t>(nobs * 4); w.dist.id_tmp = c.take<int32_t>(nobs * 4);
    w.dist.table = c.take<uint32_t>((size_t)DIST_RADIX * (size_t)dist_tiles((int64_t)nobs) * 4);
    w.pair_cnt = c.take<int32_t>(nobs * 4);
    w.bytes = c.size();
    return w;
}

struct SchurScratch { uint32_t* part; SchurPair* pair; int32_t *key, *ids, *ptr2, *blk_ptr; DistScratch dist; size_t part_bytes, bytes; };
SchurScratch schur_scratch(char* base, size_t nobs, size_t n_enum, size_t nblk)
{
    ArrCarver c{base};
    SchurScratch w{};
    w.part_bytes = (size_t)wgs((int64_t)nobs, LBP_NT) * 4;
    w.part = c.take<uint32_t>(w.part_bytes);
    w.pair = c.take<SchurPair>(n_enum * sizeof(SchurPair));
    w.key = c.take<int32_t>(n_enum * 4); w.ids = c.take<int32_t>(n_enum * 4);
    w.dist.key_a = c.take<int32_t>(n_enum * 4); w.dist.key_b = c.take<int32_t>(n_enum * 4); w.dist.id_tmp = c.take<int32_t>(n_enum * 4);
    w.dist.table = c.take<uint32_t>((size_t)DIST_RADIX * (size_t)dist_tiles((int64_t)n_enum) * 4);
    w.ptr2 = c.take<int32_t>((2 * nblk + 1) * 4);
    w.blk_ptr = c.take<int32_t>((nblk + 1) * 4);
    w.bytes = c.size();
    return w;
}

}  // namespace

int lba_schur_prepare_dev(plslam_lba_plan* P)
{
    hipStream_t s = P->ctx->stream;
    const int64_t nblk = (int64_t)P->nkf * (P->nkf + 1) / 2, n_enum = P->n_pairs_enum;
    // (the pair list with its padding stays below 2^30 entries: the look-back's sums, and the keys 2 block + kind, are 32-bit words)
    PLSLAM_REQUIRE(n_enum + (int64_t)SCH_CHUNK * nblk < ((int64_t)1 << 30) && 2 * nblk + 1 < ((int64_t)1 << 30), PLSLAM_ERANGE);
    const size_t nobs = (size_t)P->np + (size_t)P->nl;
    int rc = P->aux_schur.reserve(schur_scratch(nullptr, nobs, (size_t)n_enum, (size_t)nblk).bytes + 256);
    if (rc) return rc;
    const SchurScratch w = schur_scratch(P->aux_schur.as<char>(), nobs, (size_t)n_enum, (size_t)nblk);
    int32_t* pinned = static_cast<int32_t*>(P->pin_cnt.dev);
    const LbpLists L = lbp_lists(P);
    if (n_enum > 0) {
        PLSLAM_HIP_CHECK(hipMemsetAsync(w.part, 0, w.part_bytes, s));
        hipLaunchKernelGGL(k_lbp_pair_emit, dim3(wgs((int64_t)nobs, LBP_NT)), dim3(LBP_NT), 0, s, L, (const int32_t*)P->d_pair_cnt, w.part,
                           (int32_t)n_enum, w.key, w.pair);
    }
    dist_enqueue(s, w.key, (int32_t)n_enum, (int32_t)(2 * nblk), w.ids, w.ptr2, w.dist);
    hipLaunchKernelGGL(k_lbp_pair_layout, dim3(1), dim3(LBP_NT), 0, s, (const int32_t*)w.ptr2, (int32_t)nblk, w.blk_ptr, pinned);
    PLSLAM_HIP_CHECK(hipGetLastError());
    PLSLAM_HIP_CHECK(hipStreamSynchronize(s));              // the Schur lists' one synchronisation: the sizes the buffers are carved from
    const int32_t* h = P->pin_cnt.as<int32_t>();
    const int32_t n_padded = h[W_PADDED];
    PLSLAM_REQUIRE(n_padded >= 0 && (int64_t)n_padded <= n_enum + (int64_t)SCH_CHUNK * nblk, PLSLAM_EHIP);
    P->nblk = (int32_t)nblk;
    P->schur_chunks = h[W_SCHUR_CHUNKS];
    if ((rc = lba_schur_reserve(P, (size_t)n_padded))) return rc;
    const LbaSchurView& V = P->sc;
    PLSLAM_HIP_CHECK(hipMemcpyAsync(V.blk_ptr, w.blk_ptr, V.blk_ptr.bytes, hipMemcpyDeviceToDevice, s));
    if (n_padded > 0)
        hipLaunchKernelGGL(k_lbp_pair_place, dim3(wgs(n_padded, LBP_NT)), dim3(LBP_NT), 0, s, (const int32_t*)w.blk_ptr, (int32_t)nblk,
                           (const int32_t*)w.ptr2, (const int32_t*)w.ids, (const SchurPair*)w.pair, (int32_t)n_enum, n_padded, V.pairs.p);
    PLSLAM_HIP_CHECK(hipGetLastError());
    // (the scratch stays with the plan: the placement reads it behind this call, on the stream every later call of the plan uses)
    P->schur_ready = true;
    return PLSLAM_OK;
}

}  // namespace plslam

extern "C" int plslam_lba_plan_create_dev(plslam_ctx* ctx, const plslam_cam* K, double homog_th, int32_t n_pose_slots, int32_t nkf,
                                          int32_t npt, int32_t nls, const int32_t* d_pt_lm_loc, const int32_t* d_pt_pose_slot,
                                          const int32_t* d_pt_kf_loc, const double* d_pt_obs_uv, int32_t n_pt_obs,
                                          const int32_t* d_ls_lm_loc, const int32_t* d_ls_pose_slot, const int32_t* d_ls_kf_loc,
                                          const double* d_ls_l_obs, int32_t n_ls_obs, const double* d_Xw, const double* d_Lw,
                                          int32_t first_estimate_slot, plslam_lba_plan** out)
{
    PLSLAM_REQUIRE(ctx && K && out && n_pose_slots >= 0 && nkf >= 0 && npt >= 0 && nls >= 0, PLSLAM_EINVAL);
    PLSLAM_REQUIRE(n_pt_obs >= 0 && n_ls_obs >= 0, PLSLAM_EINVAL);
    *out = nullptr;
    PLSLAM_REQUIRE(n_pt_obs == 0 || (d_pt_lm_loc && d_pt_pose_slot && d_pt_kf_loc && d_pt_obs_uv), PLSLAM_EINVAL);
    PLSLAM_REQUIRE(n_ls_obs == 0 || (d_ls_lm_loc && d_ls_pose_slot && d_ls_kf_loc && d_ls_l_obs), PLSLAM_EINVAL);
    // (an observation without a landmark or a slot to name is out of range whatever it holds: refused before anything is launched)
    PLSLAM_REQUIRE((n_pt_obs == 0 || (npt > 0 && n_pose_slots > 0)) && (n_ls_obs == 0 || (nls > 0 && n_pose_slots > 0)), PLSLAM_EINVAL);
    PLSLAM_REQUIRE(first_estimate_slot >= -1 && (first_estimate_slot < 0 || (int64_t)first_estimate_slot + nkf <= n_pose_slots), PLSLAM_EINVAL);
    PLSLAM_REQUIRE((int64_t)n_pt_obs + n_ls_obs < ((int64_t)1 << 30), PLSLAM_ERANGE);
    plslam_lba_plan* P = new (std::nothrow) plslam_lba_plan();
    PLSLAM_REQUIRE(P != nullptr, PLSLAM_ENOMEM);
    P->ctx = ctx; P->cam = *K; P->th = homog_th; P->n_slots = n_pose_slots; P->nkf = nkf; P->npt = npt; P->nls = nls;
    P->np = n_pt_obs; P->nl = n_ls_obs;
    P->dev_lists = true;
    const size_t nobs = (size_t)n_pt_obs + (size_t)n_ls_obs;
    P->n_kfi = 0; P->n_kfi_cap = (int32_t)nobs;             // (the keyframe list's length is the device's to say)
    std::lock_guard<std::mutex> lk(ctx->mu);
    DeviceGuard dg_(ctx->device);
    hipStream_t s = ctx->stream;
    auto fail = [P, s](int rc) { (void)hipStreamSynchronize(s); P->release(); delete P; return rc; };
    LbaPlanBytes need = lba_plan_carve(P);
    int rc;
    if ((rc = P->stat.reserve(need.stat + 256)) || (rc = P->dyn.reserve(need.dyn + 256)) ||
        (rc = P->aux.reserve(plan_scratch(nullptr, nobs).bytes + 256)) || (rc = P->pin_cnt.reserve(W_WORDS * 4)))
        return fail(rc);
    if (!P->pin_cnt.dev) return fail(PLSLAM_ENOTSUP);        // the counts are written where the host reads them
    lba_plan_carve(P);
    const PlanScratch w = plan_scratch(P->aux.as<char>(), nobs);
    P->d_pair_cnt = w.pair_cnt;
    const LbaStatView& S = P->st;
    auto build = [&]() -> int {
        PLSLAM_HIP_CHECK(hipMemsetAsync(w.words, 0, D_WORDS * 4, s));
        if (d_Xw && npt) PLSLAM_HIP_CHECK(hipMemcpyAsync(P->x.Xw, d_Xw, P->x.Xw.bytes, hipMemcpyDeviceToDevice, s));
        if (d_Lw && nls) PLSLAM_HIP_CHECK(hipMemcpyAsync(P->x.Lw, d_Lw, P->x.Lw.bytes, hipMemcpyDeviceToDevice, s));
        if (nobs) {
            const LbpValidateArgs A{d_pt_lm_loc, d_pt_pose_slot, d_pt_kf_loc, d_ls_lm_loc, d_ls_pose_slot, d_ls_kf_loc, d_pt_obs_uv, d_ls_l_obs,
                                    S.pt_lm, S.pt_slot, S.pt_kf, S.ls_lm, S.ls_slot, S.ls_kf, S.uv, S.lobs, w.kf_key, w.words + D_STATUS,
                                    n_pt_obs, n_ls_obs, npt, nls, nkf, n_pose_slots, first_estimate_slot};
            hipLaunchKernelGGL(k_lbp_validate, dim3(wgs((int64_t)nobs, LBP_NT)), dim3(LBP_NT), 0, s, A);
        }
        dist_enqueue(s, S.pt_lm, n_pt_obs, npt, S.pt_ids, S.pt_ptr, w.dist);
        dist_enqueue(s, S.ls_lm, n_ls_obs, nls, S.ls_ids, S.ls_ptr, w.dist);
        dist_enqueue(s, w.kf_key, (int32_t)nobs, nkf, S.kf_ids, S.kf_ptr, w.dist);
        if (nobs)
            hipLaunchKernelGGL(k_lbp_pair_count, dim3(wgs((int64_t)nobs, LBP_NT)), dim3(LBP_NT), 0, s, lbp_lists(P), w.pair_cnt,
                               reinterpret_cast<unsigned long long*>(w.words + D_PAIRS));
        hipLaunchKernelGGL(k_lbp_publish, dim3(1), dim3(LBP_NT), 0, s, (const int32_t*)S.kf_ptr, nkf, (const int32_t*)w.words,
                           static_cast<int32_t*>(P->pin_cnt.dev));
        PLSLAM_HIP_CHECK(hipGetLastError());
        PLSLAM_HIP_CHECK(hipStreamSynchronize(s));          // the plan's one synchronisation
        return PLSLAM_OK;
    };
    if ((rc = build())) return fail(rc);
    const int32_t* h = P->pin_cnt.as<int32_t>();
    if (h[W_STATUS] != 0) {
        set_last_error("plslam_lba_plan_create_dev: an lm_loc, kf_loc or pose_slot is out of range");
        return fail(PLSLAM_EINVAL);
    }
    if (h[W_NKFI] < 0 || (size_t)h[W_NKFI] > nobs || h[W_MAX_CHUNKS] < 0) return fail(PLSLAM_EHIP);
    P->n_kfi = h[W_NKFI];
    P->max_chunks = h[W_MAX_CHUNKS];
    P->n_pairs_enum = (int64_t)(((uint64_t)(uint32_t)h[W_PAIRS_HI] << 32) | (uint32_t)h[W_PAIRS_LO]);
    need = lba_plan_carve(P);                               // (the same layout of stat and dyn; out now has the chunk partials' room)
    P->dyn_bytes = need.dyn;
    if ((rc = P->rows.reserve(need.rows + 256)) || (rc = P->out.reserve(need.out + 256)) || (rc = P->pin_in.reserve(need.dyn + 256)) ||
        (rc = P->pin_out.reserve(P->n_unknowns() * 8 + 256)))
        return fail(rc);
    lba_plan_carve(P);
    P->lm_resident = (npt == 0 || d_Xw) && (nls == 0 || d_Lw);
    *out = P;
    return PLSLAM_OK;
}

extern "C" int plslam_lba_plan_list_sizes(plslam_lba_plan* P, int prepare_schur, plslam_lba_list_sizes* out)
{
    PLSLAM_REQUIRE(P && out, PLSLAM_EINVAL);
    plslam_ctx* ctx = P->ctx;
    std::lock_guard<std::mutex> lk(ctx->mu);
    DeviceGuard dg_(ctx->device);
    if (prepare_schur) {
        int rc = lba_schur_prepare(P);
        if (rc) { (void)hipStreamSynchronize(ctx->stream); return rc; }
    }
    out->nkf = P->nkf; out->npt = P->npt; out->nls = P->nls; out->n_pt_obs = P->np; out->n_ls_obs = P->nl;
    out->n_kf_ids = P->n_kfi; out->max_chunks = P->max_chunks;
    out->schur_ready = P->schur_ready ? 1 : 0;
    out->nblk = P->schur_ready ? P->nblk : 0;
    out->n_pairs = P->schur_ready ? (int32_t)(P->sc.pairs.bytes / sizeof(SchurPair)) : 0;
    out->schur_chunks = P->schur_ready ? P->schur_chunks : 0;
    return PLSLAM_OK;
}

extern "C" int plslam_lba_plan_lists(plslam_lba_plan* P, const plslam_lba_lists* host)
{
    PLSLAM_REQUIRE(P && host, PLSLAM_EINVAL);
    plslam_ctx* ctx = P->ctx;
    std::lock_guard<std::mutex> lk(ctx->mu);
    DeviceGuard dg_(ctx->device);
    PLSLAM_REQUIRE(P->schur_ready || (!host->blk_ptr && !host->pairs), PLSLAM_EINVAL);
    const LbaStatView& S = P->st;
    const DownloadItem items[] = {
        {host->pt_ptr, S.pt_ptr, S.pt_ptr.bytes}, {host->pt_ids, S.pt_ids, S.pt_ids.bytes}, {host->ls_ptr, S.ls_ptr, S.ls_ptr.bytes},
        {host->ls_ids, S.ls_ids, S.ls_ids.bytes}, {host->kf_ptr, S.kf_ptr, S.kf_ptr.bytes}, {host->kf_ids, S.kf_ids, S.kf_ids.bytes},
        {host->pt_lm_loc, S.pt_lm, S.pt_lm.bytes}, {host->pt_pose_slot, S.pt_slot, S.pt_slot.bytes}, {host->pt_kf_loc, S.pt_kf, S.pt_kf.bytes},
        {host->pt_obs_uv, S.uv, S.uv.bytes}, {host->ls_lm_loc, S.ls_lm, S.ls_lm.bytes}, {host->ls_pose_slot, S.ls_slot, S.ls_slot.bytes},
        {host->ls_kf_loc, S.ls_kf, S.ls_kf.bytes}, {host->ls_l_obs, S.lobs, S.lobs.bytes},
        {host->blk_ptr, P->sc.blk_ptr, P->schur_ready ? P->sc.blk_ptr.bytes : 0}, {host->pairs, P->sc.pairs, P->schur_ready ? P->sc.pairs.bytes : 0}};
    return download_items(items, ctx->stream);
}
