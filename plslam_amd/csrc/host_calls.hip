// host_calls.hip -- the host-pointer convenience entry points: stage the caller's arrays in the context's buffers, launch
// kernels that live elsewhere, download.  Beside them the _dev row entry points that only check and launch, and the pinned
// allocator a caller stages with.
#include <string.h>

#include <algorithm>
#include <new>

#include "map2kf_dev.hpp"   // the gates and the visibility pre-filter
#include "match_kernels.hpp"   // plslam_knn2_hamming256: the scans and the key unpack
#include "match_plan.hpp"

using namespace plslam;

extern "C" {

// ---- host-pointer matching -------------------------------------------------------------------
int plslam_match_batched(plslam_ctx* ctx, const uint8_t* d1, const int32_t* off1,
                         const uint8_t* d2, const int32_t* off2, int32_t B, float nnr, int mutual,
                         int32_t* matches_12, int32_t* n_matches)
{
    PLSLAM_REQUIRE(ctx != nullptr && B >= 0, PLSLAM_EINVAL);
    if (B == 0) return PLSLAM_OK;
    PLSLAM_REQUIRE(off1 && off2, PLSLAM_EINVAL);
    PLSLAM_REQUIRE(off1[0] == 0 && off2[0] == 0, PLSLAM_EINVAL);
    for (int32_t b = 0; b < B; ++b)
        PLSLAM_REQUIRE(off1[b + 1] >= off1[b] && off2[b + 1] >= off2[b], PLSLAM_EINVAL);
    const int64_t r1 = off1[B], r2 = off2[B];
    PLSLAM_REQUIRE(r1 == 0 || (d1 && matches_12), PLSLAM_EINVAL);
    PLSLAM_REQUIRE(r2 == 0 || d2, PLSLAM_EINVAL);

    std::lock_guard<std::mutex> lk(ctx->mu);
    DeviceGuard g(ctx->device);
    int r;
    if ((r = ctx->in_a.reserve((size_t)r1 * 32 + 16))) return r;
    if ((r = ctx->in_b.reserve((size_t)r2 * 32 + 16))) return r;
    if ((r = ctx->out_a.reserve((size_t)r1 * 4 + 16))) return r;
    if ((r = ctx->out_b.reserve((size_t)B * 4))) return r;
    // Latency path (one StVO::match of the SLAM loop, a frame's handful of problems): stage through the
    // context's pinned buffers -- the CPU copies ~100 kB in a few microseconds and every hipMemcpyAsync
    // becomes a plain DMA enqueue instead of the runtime's pageable-memory path.
    const size_t in1 = (size_t)r1 * 32, in2 = (size_t)r2 * 32, out1 = (size_t)r1 * 4, out2 = (size_t)B * 4;
    const bool pinned = in1 + in2 <= (size_t(1) << 20);
    const size_t in2_off = align256(in1), out2_off = align256(out1);
    const uint8_t *dev1 = ctx->in_a.as<uint8_t>(), *dev2 = ctx->in_b.as<uint8_t>();
    int32_t* tab_dev = ctx->out_a.as<int32_t>();      // where the kernels write the table
    bool table_in_place = false;
    if (pinned) {
        // ONE page-locked image [d1 | d2] -> ONE upload; the table is written by the finalize kernel straight into
        // page-locked memory (the counts are then the number of entries >= 0: no download at all)
        if ((r = ctx->pin_in.reserve(in2_off + in2 + 256))) return r;
        if ((r = ctx->pin_out.reserve(out2_off + out2 + 256))) return r;
        if ((r = ctx->in_a.reserve(in2_off + in2 + 256))) return r;
        if (in1) memcpy(ctx->pin_in.as<char>(), d1, in1);
        if (in2) memcpy(ctx->pin_in.as<char>() + in2_off, d2, in2);
        dev1 = ctx->in_a.as<uint8_t>();
        dev2 = ctx->in_a.as<uint8_t>() + in2_off;
        if (r1 + r2) PLSLAM_HIP_CHECK(hipMemcpyAsync(ctx->in_a.p, ctx->pin_in.p, in2_off + in2, hipMemcpyHostToDevice, ctx->stream));
        if (void* m = mapped_device_pointer(ctx->pin_out.p)) {
            tab_dev = static_cast<int32_t*>(m);
            table_in_place = true;
        }
    } else {
        if (r1) PLSLAM_HIP_CHECK(hipMemcpyAsync(ctx->in_a.p, d1, in1, hipMemcpyHostToDevice, ctx->stream));
        if (r2) PLSLAM_HIP_CHECK(hipMemcpyAsync(ctx->in_b.p, d2, in2, hipMemcpyHostToDevice, ctx->stream));
    }

    std::vector<plslam_match_problem> probs((size_t)B);
    for (int32_t b = 0; b < B; ++b) {
        plslam_match_problem& p = probs[b];
        p.d1 = dev1 + (size_t)off1[b] * 32;
        p.d2 = dev2 + (size_t)off2[b] * 32;
        p.n1 = off1[b + 1] - off1[b];
        p.n2 = off2[b + 1] - off2[b];
        p.nnr = nnr;
        p.mutual = mutual ? 1 : 0;
        p.matches_12 = tab_dev + off1[b];
        p.n_matches = ctx->out_b.as<int32_t>() + b;
    }
    // the context keeps ONE plan object for the host-pointer path: its device buffers only grow, so
    // a call in the SLAM loop does no hipMalloc/hipFree
    if (!ctx->host_plan) ctx->host_plan = new (std::nothrow) plslam_match_plan();
    PLSLAM_REQUIRE(ctx->host_plan != nullptr, PLSLAM_ENOMEM);
    plslam_match_plan& P = *ctx->host_plan;
    P.pin_tables = true;
    r = plan_build(ctx, probs.data(), B, &P);
    if (!r) r = plan_run(&P, ctx->stream, ctx->stream);
    if (!r) {
        hipError_t e = hipSuccess;
        void* dst1 = pinned ? ctx->pin_out.p : (void*)matches_12;
        void* dst2 = pinned ? (void*)(ctx->pin_out.as<char>() + out2_off) : (void*)n_matches;
        if (r1 && !table_in_place) e = hipMemcpyAsync(dst1, ctx->out_a.p, out1, hipMemcpyDeviceToHost, ctx->stream);
        if (e == hipSuccess && n_matches && !table_in_place)
            e = hipMemcpyAsync(dst2, ctx->out_b.p, out2, hipMemcpyDeviceToHost, ctx->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
        if (e == hipSuccess && pinned) {
            if (r1) memcpy(matches_12, dst1, out1);
            if (n_matches && !table_in_place) memcpy(n_matches, dst2, out2);
            if (n_matches && table_in_place)          // StVO::match on a fresh vector: the count IS the number of entries
                for (int32_t b = 0; b < B; ++b) {
                    int32_t n = 0;
                    for (int32_t i = off1[b]; i < off1[b + 1]; ++i) n += matches_12[i] >= 0;
                    n_matches[b] = n;
                }
        }
        if (e != hipSuccess) {
            set_last_error("%s:%d: D2H of match tables -> %s", __FILE__, __LINE__, hipGetErrorString(e));
            r = PLSLAM_EHIP;
        }
    } else {
        (void)hipStreamSynchronize(ctx->stream);
    }
    return r;
}

int plslam_match(plslam_ctx* ctx, const uint8_t* d1, int32_t n1, const uint8_t* d2, int32_t n2,
                 float nnr, int mutual, int32_t* matches_12, int32_t* n_matches)
{
    PLSLAM_REQUIRE(n1 >= 0 && n2 >= 0, PLSLAM_EINVAL);
    const int32_t off1[2] = {0, n1}, off2[2] = {0, n2};
    int32_t n = 0;
    const int r = plslam_match_batched(ctx, d1, off1, d2, off2, 1, nnr, mutual, matches_12, &n);
    if (!r && n_matches) *n_matches = n;
    return r;
}

int plslam_match_prior(plslam_ctx* ctx, const uint8_t* d1, int32_t n1, const uint8_t* d2, int32_t n2,
                       float nnr, int mutual, int32_t* matches_12, int32_t* n_matches)
{
    PLSLAM_REQUIRE(ctx != nullptr && n1 >= 0 && n2 >= 0, PLSLAM_EINVAL);
    if (n_matches) *n_matches = 0;
    if (n1 == 0) return PLSLAM_OK;
    PLSLAM_REQUIRE(d1 && matches_12 && (n2 == 0 || d2), PLSLAM_EINVAL);
    std::lock_guard<std::mutex> lk(ctx->mu);
    DeviceGuard g(ctx->device);
    hipStream_t s = ctx->stream;
    int r;
    if ((r = ctx->in_a.reserve((size_t)n1 * 32 + 16))) return r;
    if ((r = ctx->in_b.reserve((size_t)n2 * 32 + 16))) return r;
    if ((r = ctx->out_a.reserve((size_t)n1 * 4 + 16))) return r;
    if ((r = ctx->out_b.reserve(16))) return r;
    StreamSyncOnError guard(s);
    PLSLAM_HIP_CHECK(hipMemcpyAsync(ctx->in_a.p, d1, (size_t)n1 * 32, hipMemcpyHostToDevice, s));
    if (n2) PLSLAM_HIP_CHECK(hipMemcpyAsync(ctx->in_b.p, d2, (size_t)n2 * 32, hipMemcpyHostToDevice, s));
    PLSLAM_HIP_CHECK(hipMemcpyAsync(ctx->out_a.p, matches_12, (size_t)n1 * 4, hipMemcpyHostToDevice, s));
    plslam_match_problem p{};
    p.d1 = ctx->in_a.as<uint8_t>(); p.d2 = ctx->in_b.as<uint8_t>(); p.n1 = n1; p.n2 = n2; p.nnr = nnr;
    p.mutual = mutual ? 1 : 0; p.matches_12 = ctx->out_a.as<int32_t>(); p.n_matches = ctx->out_b.as<int32_t>();
    p.keep_prior = 1;
    if ((r = plslam::match_problems_on_ctx_stream(ctx, &p, 1))) return r;
    int32_t n = 0;
    PLSLAM_HIP_CHECK(hipMemcpyAsync(matches_12, ctx->out_a.p, (size_t)n1 * 4, hipMemcpyDeviceToHost, s));
    PLSLAM_HIP_CHECK(hipMemcpyAsync(&n, ctx->out_b.p, 4, hipMemcpyDeviceToHost, s));
    PLSLAM_HIP_CHECK(hipStreamSynchronize(s));
    guard.dismiss();
    if (n_matches) *n_matches = n;
    return PLSLAM_OK;
}

int plslam_knn2_hamming256(plslam_ctx* ctx, const uint8_t* q, int32_t nq, const uint8_t* t,
                           int32_t nt, int32_t* idx, int32_t* dist)
{
    PLSLAM_REQUIRE(ctx != nullptr && nq >= 0 && nt >= 0, PLSLAM_EINVAL);
    if (nq == 0) return PLSLAM_OK;
    PLSLAM_REQUIRE(q && idx && dist && (nt == 0 || t), PLSLAM_EINVAL);
    PLSLAM_REQUIRE(nt <= PLSLAM_MAX_TRAIN_ROWS, PLSLAM_ERANGE);
    std::lock_guard<std::mutex> lk(ctx->mu);
    DeviceGuard g(ctx->device);
    int r;
    hipStream_t s = ctx->stream;
    StreamSyncOnError sg(s);
    const bool small = (nq + 63) / 64 < ctx->prop.multiProcessorCount * 4;
    // large query sets (or a forced variant): the directed form of the matrix-core scan; otherwise the popcount kernels
    const bool mfma = nt > 0 && (ctx->scan_variant == PLSLAM_SCAN_MFMA || (ctx->scan_variant == PLSLAM_SCAN_AUTO && !small));
    const int variant = ctx->scan_variant == PLSLAM_SCAN_WAVE_PER_QUERY || (ctx->scan_variant == PLSLAM_SCAN_AUTO && small)
                            ? PLSLAM_SCAN_WAVE_PER_QUERY : PLSLAM_SCAN_LANE_PER_QUERY;
    const int bt = variant == PLSLAM_SCAN_WAVE_PER_QUERY ? 256 : (ctx->scan_block ? ctx->scan_block : 256);
    const int rpb = mfma ? 256 : scan_rows_per_block(variant, bt);
    std::vector<BlockDesc> blocks;
    for (int32_t r0 = 0; r0 < nq; r0 += rpb) blocks.push_back({0, r0});
    if (mfma || variant == PLSLAM_SCAN_LANE_PER_QUERY) {   // these kernels read the XCD-striped layout (8 rows of L)
        const size_t n = blocks.size(), L = (n + 7) / 8;
        std::vector<BlockDesc> striped(8 * L, BlockDesc{-1, 0});
        for (size_t i = 0; i < n; ++i) striped[(i & 7) * L + (i >> 3)] = blocks[i];
        blocks.swap(striped);
    }
    // one image [q | t | scan descriptor | block table] -- page-locked and uploaded with ONE copy when it is small --, the
    // (idx, dist) pairs written by the unpack kernel straight into page-locked memory when the device can address it
    const size_t qb = (size_t)nq * 32, tb = (size_t)nt * 32, bb = blocks.size() * sizeof(BlockDesc);
    Carver c;
    const size_t oQ = c.take(qb), oT = c.take(tb + 16), oD = c.take(std::max(sizeof(SymDesc), sizeof(ScanDesc))), oB = c.take(bb);
    const size_t ob = align256((size_t)nq * 8);
    if ((r = ctx->in_a.reserve(c.off))) return r;
    if ((r = ctx->misc_a.reserve((size_t)nq * 8))) return r;                 // keys
    if ((r = ctx->out_a.reserve(2 * ob))) return r;                          // idx | dist
    if ((r = ctx->pin_out.reserve(2 * ob))) return r;
    char* d = ctx->in_a.as<char>();
    SymDesc y{};
    y.a = (const uint8_t*)(d + oQ); y.b = (const uint8_t*)(d + oT); y.keys12 = ctx->misc_a.as<uint32_t>();
    y.n1 = nq; y.n2 = nt;
    y.flags = 1;                                   // knnMatch returns the second neighbour's index
    const ScanDesc sd{(const uint8_t*)(d + oQ), (const uint8_t*)(d + oT), ctx->misc_a.as<uint32_t>(), nq, nt};
    const void* desc = mfma ? (const void*)&y : (const void*)&sd;
    const size_t desc_bytes = mfma ? sizeof(y) : sizeof(sd);
    if (c.off <= (size_t(1) << 20)) {
        if ((r = ctx->pin_in.reserve(c.off))) return r;
        char* h = ctx->pin_in.as<char>();
        memcpy(h + oQ, q, qb);
        if (tb) memcpy(h + oT, t, tb);
        memcpy(h + oD, desc, desc_bytes);
        memcpy(h + oB, blocks.data(), bb);
        PLSLAM_HIP_CHECK(hipMemcpyAsync(d, h, c.off, hipMemcpyHostToDevice, s));
    } else {
        PLSLAM_HIP_CHECK(hipMemcpyAsync(d + oQ, q, qb, hipMemcpyHostToDevice, s));
        if (tb) PLSLAM_HIP_CHECK(hipMemcpyAsync(d + oT, t, tb, hipMemcpyHostToDevice, s));
        PLSLAM_HIP_CHECK(hipMemcpyAsync(d + oD, desc, desc_bytes, hipMemcpyHostToDevice, s));
        PLSLAM_HIP_CHECK(hipMemcpyAsync(d + oB, blocks.data(), bb, hipMemcpyHostToDevice, s));
    }
    if (mfma)
        r = launch_scan_mfma_form(ctx->mfma_form, (const SymDesc*)(d + oD), (const BlockDesc*)(d + oB), (int)blocks.size(), nullptr,
                                  0, nt > 2048, true, s);
    else
        r = launch_scan(ctx, variant, bt, (const ScanDesc*)(d + oD), (const BlockDesc*)(d + oB), (int)blocks.size(), nullptr, 0, s);
    if (r) return r;
    char* ho = ctx->pin_out.as<char>();
    char* out_dev = static_cast<char*>(mapped_device_pointer(ho));
    const bool in_place = out_dev != nullptr;
    if (!in_place) out_dev = ctx->out_a.as<char>();
    if ((r = launch_unpack_keys(ctx->misc_a.as<uint32_t>(), nq * 2, (int32_t*)out_dev, (int32_t*)(out_dev + ob), s))) return r;
    if (!in_place) PLSLAM_HIP_CHECK(hipMemcpyAsync(ho, out_dev, 2 * ob, hipMemcpyDeviceToHost, s));
    PLSLAM_HIP_CHECK(hipStreamSynchronize(s));
    sg.dismiss();
    memcpy(idx, ho, (size_t)nq * 8);
    memcpy(dist, ho + ob, (size_t)nq * 8);
    return PLSLAM_OK;
}

// ---- LBA rows --------------------------------------------------------------------------------
int plslam_lba_point_rows_dev_n(plslam_ctx* ctx, const plslam_cam* K, double homog_th,
                                const double* T_kf_w, int32_t n_pose_slots, const double* Xw, const double* obs_uv,
                                const int32_t* lm_loc, const int32_t* kf_slot, int32_t nobs,
                                double* J_pose, double* J_lm, double* r, double* w, void* stream)
{
    PLSLAM_REQUIRE(ctx && K && nobs >= 0 && n_pose_slots >= 0, PLSLAM_EINVAL);
    if (nobs == 0) return PLSLAM_OK;
    PLSLAM_REQUIRE(T_kf_w && Xw && obs_uv && lm_loc && kf_slot && J_pose && J_lm && r && w, PLSLAM_EINVAL);
    DeviceGuard g(ctx->device);
    return launch_point_rows(*K, homog_th, T_kf_w, Xw, obs_uv, lm_loc, kf_slot, nobs, J_pose, J_lm, r, w,
                             stream ? static_cast<hipStream_t>(stream) : ctx->stream, n_pose_slots);
}

int plslam_lba_point_rows_dev(plslam_ctx* ctx, const plslam_cam* K, double homog_th,
                              const double* T_kf_w, const double* Xw, const double* obs_uv,
                              const int32_t* lm_loc, const int32_t* kf_slot, int32_t nobs,
                              double* J_pose, double* J_lm, double* r, double* w, void* stream)
{
    return plslam_lba_point_rows_dev_n(ctx, K, homog_th, T_kf_w, 0, Xw, obs_uv, lm_loc, kf_slot, nobs, J_pose, J_lm, r, w, stream);
}

int plslam_lba_line_rows_dev_n(plslam_ctx* ctx, const plslam_cam* K, double homog_th,
                               int compat_iter_pass, const double* T_kf_w, int32_t n_pose_slots, const double* Lw,
                               const double* l_obs, const int32_t* lm_loc, const int32_t* kf_slot,
                               int32_t nobs, double* J_pose, double* J_lm, double* r, double* w,
                               void* stream)
{
    PLSLAM_REQUIRE(ctx && K && nobs >= 0 && n_pose_slots >= 0, PLSLAM_EINVAL);
    if (nobs == 0) return PLSLAM_OK;
    PLSLAM_REQUIRE(T_kf_w && Lw && l_obs && lm_loc && kf_slot && J_pose && J_lm && r && w, PLSLAM_EINVAL);
    DeviceGuard g(ctx->device);
    return launch_line_rows(*K, homog_th, compat_iter_pass ? 1 : 0, T_kf_w, Lw, l_obs, lm_loc, kf_slot,
                            nobs, J_pose, J_lm, r, w,
                            stream ? static_cast<hipStream_t>(stream) : ctx->stream, n_pose_slots);
}

int plslam_lba_line_rows_dev(plslam_ctx* ctx, const plslam_cam* K, double homog_th,
                             int compat_iter_pass, const double* T_kf_w, const double* Lw,
                             const double* l_obs, const int32_t* lm_loc, const int32_t* kf_slot,
                             int32_t nobs, double* J_pose, double* J_lm, double* r, double* w,
                             void* stream)
{
    return plslam_lba_line_rows_dev_n(ctx, K, homog_th, compat_iter_pass, T_kf_w, 0, Lw, l_obs, lm_loc, kf_slot, nobs, J_pose, J_lm, r, w,
                                      stream);
}


static int lba_rows_host(plslam_ctx* ctx, const plslam_cam* K, double th, int lines, int compat,
                         const double* T, int32_t nkf, const double* LM, int64_t n_lm_doubles,
                         const double* obs, int obs_stride, const int32_t* lm_loc,
                         const int32_t* kf_slot, int32_t nobs, double* Jp, double* Jl, double* r,
                         double* w)
{
    PLSLAM_REQUIRE(ctx && K && nobs >= 0 && nkf >= 0 && n_lm_doubles >= 0, PLSLAM_EINVAL);
    if (nobs == 0) return PLSLAM_OK;
    PLSLAM_REQUIRE(T && LM && obs && lm_loc && kf_slot && Jp && Jl && r && w, PLSLAM_EINVAL);
    const int lmw = lines ? 6 : 3;
    const int lm_stride = lines ? (compat ? 3 : 6) : 3;
    for (int32_t o = 0; o < nobs; ++o) {  // index validation: the kernel trusts its inputs
        PLSLAM_REQUIRE(kf_slot[o] >= 0 && kf_slot[o] < nkf, PLSLAM_EINVAL);
        PLSLAM_REQUIRE(lm_loc[o] >= 0 && (int64_t)lm_loc[o] * lm_stride + 3 <= n_lm_doubles, PLSLAM_EINVAL);
        PLSLAM_REQUIRE(!lines || compat || (int64_t)lm_loc[o] * 6 + 6 <= n_lm_doubles, PLSLAM_EINVAL);
    }
    std::lock_guard<std::mutex> lk(ctx->mu);
    DeviceGuard g(ctx->device);
    Carver ci, co;
    const size_t oT = ci.take((size_t)nkf * 128), oL = ci.take((size_t)n_lm_doubles * 8),
                 oO = ci.take((size_t)nobs * obs_stride * 8), oLm = ci.take((size_t)nobs * 4),
                 oKf = ci.take((size_t)nobs * 4);
    const size_t oJp = co.take((size_t)nobs * 48), oJl = co.take((size_t)nobs * lmw * 8),
                 oR = co.take((size_t)nobs * 8), oW = co.take((size_t)nobs * 8);
    int rc;
    if ((rc = ctx->in_a.reserve(ci.off))) return rc;
    if ((rc = ctx->out_a.reserve(co.off))) return rc;
    char* di = ctx->in_a.as<char>();
    char* dout = ctx->out_a.as<char>();
    hipStream_t s = ctx->stream;
    PLSLAM_HIP_CHECK(hipMemcpyAsync(di + oT, T, (size_t)nkf * 128, hipMemcpyHostToDevice, s));
    PLSLAM_HIP_CHECK(hipMemcpyAsync(di + oL, LM, (size_t)n_lm_doubles * 8, hipMemcpyHostToDevice, s));
    PLSLAM_HIP_CHECK(hipMemcpyAsync(di + oO, obs, (size_t)nobs * obs_stride * 8, hipMemcpyHostToDevice, s));
    PLSLAM_HIP_CHECK(hipMemcpyAsync(di + oLm, lm_loc, (size_t)nobs * 4, hipMemcpyHostToDevice, s));
    PLSLAM_HIP_CHECK(hipMemcpyAsync(di + oKf, kf_slot, (size_t)nobs * 4, hipMemcpyHostToDevice, s));
    if (!lines)
        rc = launch_point_rows(*K, th, (double*)(di + oT), (double*)(di + oL), (double*)(di + oO),
                               (int32_t*)(di + oLm), (int32_t*)(di + oKf), nobs, (double*)(dout + oJp),
                               (double*)(dout + oJl), (double*)(dout + oR), (double*)(dout + oW), s, nkf);
    else
        rc = launch_line_rows(*K, th, compat, (double*)(di + oT), (double*)(di + oL), (double*)(di + oO),
                              (int32_t*)(di + oLm), (int32_t*)(di + oKf), nobs, (double*)(dout + oJp),
                              (double*)(dout + oJl), (double*)(dout + oR), (double*)(dout + oW), s, nkf);
    if (rc) return rc;
    PLSLAM_HIP_CHECK(hipMemcpyAsync(Jp, dout + oJp, (size_t)nobs * 48, hipMemcpyDeviceToHost, s));
    PLSLAM_HIP_CHECK(hipMemcpyAsync(Jl, dout + oJl, (size_t)nobs * lmw * 8, hipMemcpyDeviceToHost, s));
    PLSLAM_HIP_CHECK(hipMemcpyAsync(r, dout + oR, (size_t)nobs * 8, hipMemcpyDeviceToHost, s));
    PLSLAM_HIP_CHECK(hipMemcpyAsync(w, dout + oW, (size_t)nobs * 8, hipMemcpyDeviceToHost, s));
    PLSLAM_HIP_CHECK(hipStreamSynchronize(s));
    return PLSLAM_OK;
}

int plslam_lba_point_rows(plslam_ctx* ctx, const plslam_cam* K, double homog_th,
                          const double* T_kf_w, int32_t nkf, const double* Xw, int32_t npt,
                          const double* obs_uv, const int32_t* lm_loc, const int32_t* kf_slot,
                          int32_t nobs, double* J_pose, double* J_lm, double* r, double* w)
{
    return lba_rows_host(ctx, K, homog_th, 0, 0, T_kf_w, nkf, Xw, (int64_t)npt * 3, obs_uv, 2, lm_loc,
                         kf_slot, nobs, J_pose, J_lm, r, w);
}

int plslam_lba_line_rows(plslam_ctx* ctx, const plslam_cam* K, double homog_th,
                         int compat_iter_pass, const double* T_kf_w, int32_t nkf, const double* Lw,
                         int32_t n_lw, const double* l_obs, const int32_t* lm_loc,
                         const int32_t* kf_slot, int32_t nobs, double* J_pose, double* J_lm,
                         double* r, double* w)
{
    return lba_rows_host(ctx, K, homog_th, 1, compat_iter_pass ? 1 : 0, T_kf_w, nkf, Lw, n_lw, l_obs, 3,
                         lm_loc, kf_slot, nobs, J_pose, J_lm, r, w);
}

// ---- gates -----------------------------------------------------------------------------------
static int gate_host(plslam_ctx* ctx, const plslam_cam* K, const double* Twf, int lines,
                     const double* LM, const int32_t* m12, int32_t nq, const double* feat, int32_t nt,
                     double th, uint8_t* mask, int32_t* n_inliers)
{
    PLSLAM_REQUIRE(ctx && K && Twf && nq >= 0 && nt >= 0, PLSLAM_EINVAL);
    if (n_inliers) *n_inliers = 0;
    if (nq == 0) return PLSLAM_OK;
    PLSLAM_REQUIRE(LM && m12 && mask && (nt == 0 || feat), PLSLAM_EINVAL);
    for (int32_t i = 0; i < nq; ++i) PLSLAM_REQUIRE(m12[i] < nt, PLSLAM_EINVAL);
    const int lw = lines ? 6 : 3, fw = lines ? 3 : 2;
    std::lock_guard<std::mutex> lk(ctx->mu);
    DeviceGuard g(ctx->device);
    Carver c;
    const size_t oL = c.take((size_t)nq * lw * 8), oM = c.take((size_t)nq * 4),
                 oF = c.take((size_t)nt * fw * 8 + 16), oMask = c.take((size_t)nq), oCnt = c.take(4);
    int rc;
    if ((rc = ctx->in_a.reserve(c.off))) return rc;
    char* d = ctx->in_a.as<char>();
    hipStream_t s = ctx->stream;
    PLSLAM_HIP_CHECK(hipMemcpyAsync(d + oL, LM, (size_t)nq * lw * 8, hipMemcpyHostToDevice, s));
    PLSLAM_HIP_CHECK(hipMemcpyAsync(d + oM, m12, (size_t)nq * 4, hipMemcpyHostToDevice, s));
    if (nt) PLSLAM_HIP_CHECK(hipMemcpyAsync(d + oF, feat, (size_t)nt * fw * 8, hipMemcpyHostToDevice, s));
    rc = lines ? launch_line_gate(*K, Twf, (double*)(d + oL), (int32_t*)(d + oM), nq, (double*)(d + oF), th,
                                  (uint8_t*)(d + oMask), (int32_t*)(d + oCnt), s)
               : launch_point_gate(*K, Twf, (double*)(d + oL), (int32_t*)(d + oM), nq, (double*)(d + oF), th,
                                   (uint8_t*)(d + oMask), (int32_t*)(d + oCnt), s);
    if (rc) return rc;
    PLSLAM_HIP_CHECK(hipMemcpyAsync(mask, d + oMask, (size_t)nq, hipMemcpyDeviceToHost, s));
    int32_t cnt = 0;
    PLSLAM_HIP_CHECK(hipMemcpyAsync(&cnt, d + oCnt, 4, hipMemcpyDeviceToHost, s));
    PLSLAM_HIP_CHECK(hipStreamSynchronize(s));
    if (n_inliers) *n_inliers = cnt;
    return PLSLAM_OK;
}

int plslam_map2kf_point_gate(plslam_ctx* ctx, const plslam_cam* K, const double* Twf,
                             const double* Xw, const int32_t* matches_12, int32_t nq,
                             const double* pl, int32_t nt, double max_epip, uint8_t* mask,
                             int32_t* n_inliers)
{
    return gate_host(ctx, K, Twf, 0, Xw, matches_12, nq, pl, nt, max_epip, mask, n_inliers);
}

int plslam_map2kf_line_gate(plslam_ctx* ctx, const plslam_cam* K, const double* Twf,
                            const double* Lw, const int32_t* matches_12, int32_t nq,
                            const double* le, int32_t nt, double max_epip, uint8_t* mask,
                            int32_t* n_inliers)
{
    return gate_host(ctx, K, Twf, 1, Lw, matches_12, nq, le, nt, max_epip, mask, n_inliers);
}

static int visible_host(plslam_ctx* ctx, const plslam_cam* K, const double* Twf, const double* X,
                        int32_t n, int lines, uint8_t* vis)
{
    PLSLAM_REQUIRE(ctx && K && Twf && n >= 0, PLSLAM_EINVAL);
    if (n == 0) return PLSLAM_OK;
    PLSLAM_REQUIRE(X && vis, PLSLAM_EINVAL);
    const int lw = lines ? 6 : 3;
    std::lock_guard<std::mutex> lk(ctx->mu);
    DeviceGuard g(ctx->device);
    Carver c;
    const size_t oX = c.take((size_t)n * lw * 8), oV = c.take((size_t)n);
    int rc;
    if ((rc = ctx->in_a.reserve(c.off))) return rc;
    char* d = ctx->in_a.as<char>();
    hipStream_t s = ctx->stream;
    PLSLAM_HIP_CHECK(hipMemcpyAsync(d + oX, X, (size_t)n * lw * 8, hipMemcpyHostToDevice, s));
    if ((rc = launch_visible(*K, Twf, (double*)(d + oX), n, lines, (uint8_t*)(d + oV), s))) return rc;
    PLSLAM_HIP_CHECK(hipMemcpyAsync(vis, d + oV, (size_t)n, hipMemcpyDeviceToHost, s));
    PLSLAM_HIP_CHECK(hipStreamSynchronize(s));
    return PLSLAM_OK;
}

int plslam_map_point_visible(plslam_ctx* ctx, const plslam_cam* K, const double* Twf,
                             const double* Xw, int32_t n, uint8_t* vis)
{
    return visible_host(ctx, K, Twf, Xw, n, 0, vis);
}

int plslam_map_line_visible(plslam_ctx* ctx, const plslam_cam* K, const double* Twf,
                            const double* Lw, int32_t n, uint8_t* vis)
{
    return visible_host(ctx, K, Twf, Lw, n, 1, vis);
}

// ---- representative descriptors ---------------------------------------------------------------
int plslam_median_desc_batched_dev(plslam_ctx* ctx, const uint8_t* desc_lists, const int32_t* offsets,
                                   int32_t n_lm, int32_t total, int32_t* med_idx, uint8_t* med_desc,
                                   void* stream)
{
    PLSLAM_REQUIRE(ctx && n_lm >= 0 && total >= 0, PLSLAM_EINVAL);
    if (n_lm == 0) return PLSLAM_OK;
    PLSLAM_REQUIRE(offsets && med_idx && (total == 0 || desc_lists), PLSLAM_EINVAL);
    PLSLAM_REQUIRE(((uintptr_t)desc_lists & 3) == 0 && ((uintptr_t)med_desc & 3) == 0, PLSLAM_EINVAL);
    DeviceGuard g(ctx->device);
    return launch_median_desc(desc_lists, offsets, n_lm, total, med_idx, med_desc,
                              stream ? static_cast<hipStream_t>(stream) : ctx->stream);
}

int plslam_median_desc_batched(plslam_ctx* ctx, const uint8_t* desc_lists, const int32_t* offsets,
                               int32_t n_lm, int32_t* med_idx, uint8_t* med_desc)
{
    PLSLAM_REQUIRE(ctx && n_lm >= 0, PLSLAM_EINVAL);
    if (n_lm == 0) return PLSLAM_OK;
    PLSLAM_REQUIRE(offsets && med_idx && offsets[0] == 0, PLSLAM_EINVAL);
    for (int32_t l = 0; l < n_lm; ++l) {
        const int64_t n = (int64_t)offsets[l + 1] - offsets[l];
        PLSLAM_REQUIRE(n >= 0 && n < (1 << 23), PLSLAM_EINVAL);
    }
    const int32_t total = offsets[n_lm];
    PLSLAM_REQUIRE(total == 0 || desc_lists, PLSLAM_EINVAL);
    std::lock_guard<std::mutex> lk(ctx->mu);
    DeviceGuard g(ctx->device);
    Carver c;
    const size_t oD = c.take((size_t)total * 32), oO = c.take((size_t)(n_lm + 1) * 4),
                 oI = c.take((size_t)n_lm * 4), oM = c.take((size_t)n_lm * 32);
    int rc;
    if ((rc = ctx->in_a.reserve(c.off))) return rc;
    char* d = ctx->in_a.as<char>();
    hipStream_t s = ctx->stream;
    if (total) PLSLAM_HIP_CHECK(hipMemcpyAsync(d + oD, desc_lists, (size_t)total * 32, hipMemcpyHostToDevice, s));
    PLSLAM_HIP_CHECK(hipMemcpyAsync(d + oO, offsets, (size_t)(n_lm + 1) * 4, hipMemcpyHostToDevice, s));
    if ((rc = launch_median_desc((const uint8_t*)(d + oD), (const int32_t*)(d + oO), n_lm, total,
                                 (int32_t*)(d + oI), med_desc ? (uint8_t*)(d + oM) : nullptr, s)))
        return rc;
    PLSLAM_HIP_CHECK(hipMemcpyAsync(med_idx, d + oI, (size_t)n_lm * 4, hipMemcpyDeviceToHost, s));
    if (med_desc) PLSLAM_HIP_CHECK(hipMemcpyAsync(med_desc, d + oM, (size_t)n_lm * 32, hipMemcpyDeviceToHost, s));
    PLSLAM_HIP_CHECK(hipStreamSynchronize(s));
    return PLSLAM_OK;
}

// ---- LBD binarisation ------------------------------------------------------------------------
int plslam_lbd_binarise_dev(plslam_ctx* ctx, const float* lbd_f32, int32_t n, uint8_t* desc_u8,
                            void* stream)
{
    PLSLAM_REQUIRE(ctx && n >= 0, PLSLAM_EINVAL);
    if (n == 0) return PLSLAM_OK;
    PLSLAM_REQUIRE(lbd_f32 && desc_u8, PLSLAM_EINVAL);
    PLSLAM_REQUIRE(((uintptr_t)lbd_f32 & 15) == 0 && ((uintptr_t)desc_u8 & 15) == 0, PLSLAM_EINVAL);
    DeviceGuard g(ctx->device);
    return launch_lbd_binarise(lbd_f32, n, desc_u8,
                               stream ? static_cast<hipStream_t>(stream) : ctx->stream);
}

int plslam_lbd_binarise(plslam_ctx* ctx, const float* lbd_f32, int32_t n, uint8_t* desc_u8)
{
    PLSLAM_REQUIRE(ctx && n >= 0, PLSLAM_EINVAL);
    if (n == 0) return PLSLAM_OK;
    PLSLAM_REQUIRE(lbd_f32 && desc_u8, PLSLAM_EINVAL);
    std::lock_guard<std::mutex> lk(ctx->mu);
    DeviceGuard g(ctx->device);
    Carver c;
    const size_t oF = c.take((size_t)n * PLSLAM_LBD_FLOATS * 4), oC = c.take((size_t)n * 32);
    int rc;
    if ((rc = ctx->in_a.reserve(c.off))) return rc;
    char* d = ctx->in_a.as<char>();
    hipStream_t s = ctx->stream;
    PLSLAM_HIP_CHECK(hipMemcpyAsync(d + oF, lbd_f32, (size_t)n * PLSLAM_LBD_FLOATS * 4,
                                    hipMemcpyHostToDevice, s));
    if ((rc = launch_lbd_binarise((const float*)(d + oF), n, (uint8_t*)(d + oC), s))) return rc;
    PLSLAM_HIP_CHECK(hipMemcpyAsync(desc_u8, d + oC, (size_t)n * 32, hipMemcpyDeviceToHost, s));
    PLSLAM_HIP_CHECK(hipStreamSynchronize(s));
    return PLSLAM_OK;
}

void* plslam_pinned_alloc(size_t bytes)
{
    void* p = nullptr;
    return hipHostMalloc(&p, bytes ? bytes : 1, hipHostMallocDefault) == hipSuccess ? p : nullptr;
}

void plslam_pinned_free(void* p)
{
    if (p) (void)hipHostFree(p);
}

}  // extern "C"
