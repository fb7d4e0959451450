// track.hip -- K108-K110: from the match tables and stereo gates of a batch of stereo pairs to the packed prev -> curr
// correspondences computeRelativePoseRobustGN runs on (K54, loop_closure.hip), without the host in between
// (include/plslam_track.h states the semantics per pair).  fp64, no FMA contraction, operations in the order written.
//
//   K108  count   one workgroup of 256 lanes per (pair, kind) counts the kind's correspondences: counts[kind * B + b]
//   K109  scan    ONE workgroup turns the 2 B counts into the two offset arrays (B + 1 entries each): lane t sums
//                 track_scan_chunk(B) consecutive pairs, adds the sums of the lanes below it, and writes its pairs' offsets
//   K110  write   one workgroup per (pair, kind) evaluates the predicate again and writes rows [off[b], off[b + 1]): the
//                 ballot prefix per 256-row chunk of gather_kind (loop_closure.hip), back-projecting on the fly
//   K110f         the same device functions for ONE frame, indexed by left row (plslam_stereo_backproject_dev)
//
// Three launches: no workgroup waits for another, and every row's place is a function of the tables alone.  K110 writes
// nothing at or past off[b + 1]: were a table changed between K108 and K110, rows would be dropped, never written outside the
// pair's range.
//
// The host half: track_plan.hpp decides everything that needs no device (checks, capacities, the buffer table, the launch
// shapes); what is left here allocates, copies, launches and hands the rows to K54.
#include <new>

#include "common.hpp"

#include "lc_plan.hpp"      // lc_check_params
#include "track_plan.hpp"

struct plslam_track_batch {
    plslam_ctx* ctx = nullptr;
    plslam_lc_params p{};
    int32_t B = 0;
    plslam::TrackCaps caps;
    plslam::TrackLayout L;
    plslam::DevBuf buf;         // every array of the object (track_plan.hpp: TrackBuf)
    template <class T> T* at(int which) const { return reinterpret_cast<T*>(buf.as<char>() + L.off[which]); }
};

namespace plslam {
namespace {

struct TrackCam { double fx, cx, cy, b; };

// one kind of one pair, as the three kernels read it
struct TrackKind {
    const int32_t* m;
    const int32_t* st_prev;
    const double* disp;
    const float* f_prev;
    const int32_t* st_curr;
    const float* f_curr;
    int32_t n_prev, n_curr;
};

// where K110 writes (the bases of the whole batch)
struct TrackOut {
    const int32_t* pt_off;
    const int32_t* ls_off;
    int32_t* pt_rows;
    int32_t* ls_rows;
    double* P;
    double* pl;
    double* sPeP;
    double* le;
};

constexpr int PAIR_WORDS = (int)(sizeof(plslam_track_pair) / 8);
static_assert(sizeof(plslam_track_pair) % 8 == 0, "K108 / K110 copy their record in 8-byte words");

// record b into LDS (every lane returns behind the barrier), then the kind's view of it
__device__ __forceinline__ TrackKind load_kind(plslam_track_pair& pr, const plslam_track_pair* pairs, int b, int kind)
{
    const int tid = threadIdx.x;
    if (tid < PAIR_WORDS) reinterpret_cast<uint64_t*>(&pr)[tid] = g_(reinterpret_cast<const uint64_t*>(pairs))[(size_t)b * PAIR_WORDS + tid];
    __syncthreads();
    if (kind) return TrackKind{pr.m_ls, pr.st_ls_prev, pr.disp_ls_prev, pr.seg_prev, pr.st_ls_curr, pr.seg_curr, pr.n_ls_prev, pr.n_ls_curr};
    return TrackKind{pr.m_pt, pr.st_pt_prev, pr.disp_pt_prev, pr.kp_prev, pr.st_pt_curr, pr.kp_curr, pr.n_pt_prev, pr.n_pt_curr};
}

// the correspondence of prev row i1: i2, or -1 (no array is read where it has no rows: a kind without rows has null arrays)
__device__ __forceinline__ int32_t track_match(const TrackKind& k, int32_t i1)
{
    if (i1 >= k.n_prev) return -1;
    const int32_t i2 = g_(k.m)[i1];
    if (i2 < 0 || i2 >= k.n_curr) return -1;
    if (g_(k.st_prev)[i1] < 0) return -1;
    if (g_(k.st_curr)[i2] < 0) return -1;
    return i2;
}

// PinholeStereoCamera::backProjection as include/plslam_track.h states it
__device__ __forceinline__ void track_backproject(const TrackCam& c, double u, double v, double d, double X[3])
{
    const double bd = c.b / d;
    X[0] = bd * (u - c.cx);
    X[1] = bd * (v - c.cy);
    X[2] = bd * c.fx;
}

// the normalised line through (sx, sy, 1) and (ex, ey, 1)
__device__ __forceinline__ void track_line(double sx, double sy, double ex, double ey, double le[3])
{
    const double l0 = sy - ey, l1 = ex - sx, l2 = sx * ey - sy * ex;
    const double n = sqrt(l0 * l0 + l1 * l1);
    le[0] = l0 / n;
    le[1] = l1 / n;
    le[2] = l2 / n;
}

// P (3) and pl (2) of a point: the left key point f[i1] with its disparity, observed at g[i2]
__device__ __forceinline__ void track_point_row(const TrackCam& c, const float* f, int32_t i1, double d, const float* g, int32_t i2,
                                                double* P, double* pl)
{
    double X[3];
    track_backproject(c, (double)g_(f)[2 * (size_t)i1], (double)g_(f)[2 * (size_t)i1 + 1], d, X);
    g_(P)[0] = X[0]; g_(P)[1] = X[1]; g_(P)[2] = X[2];
    g_(pl)[0] = (double)g_(g)[2 * (size_t)i2];
    g_(pl)[1] = (double)g_(g)[2 * (size_t)i2 + 1];
}

// sPeP (6) and le (3) of a line: the left segment f[i1] with its two disparities, observed as the segment g[i2]
__device__ __forceinline__ void track_line_row(const TrackCam& c, const float* f, int32_t i1, double ds, double de, const float* g,
                                               int32_t i2, double* sPeP, double* le)
{
    double S[3], E[3], l[3];
    track_backproject(c, (double)g_(f)[4 * (size_t)i1], (double)g_(f)[4 * (size_t)i1 + 1], ds, S);
    track_backproject(c, (double)g_(f)[4 * (size_t)i1 + 2], (double)g_(f)[4 * (size_t)i1 + 3], de, E);
    track_line((double)g_(g)[4 * (size_t)i2], (double)g_(g)[4 * (size_t)i2 + 1], (double)g_(g)[4 * (size_t)i2 + 2],
               (double)g_(g)[4 * (size_t)i2 + 3], l);
#pragma unroll
    for (int q = 0; q < 3; ++q) { g_(sPeP)[q] = S[q]; g_(sPeP)[3 + q] = E[q]; g_(le)[q] = l[q]; }
}

// K108
__global__ void __launch_bounds__(TRACK_THREADS) k_track_count(const plslam_track_pair* pairs, int32_t B, int32_t* counts)
{
    __shared__ plslam_track_pair pr;
    __shared__ int32_t wsum[TRACK_THREADS / 64];
    const int tid = threadIdx.x, b = blockIdx.x, kind = blockIdx.y;
    const TrackKind k = load_kind(pr, pairs, b, kind);
    int32_t n = 0;                                                  // the wave's count, the same in all its lanes
    for (int32_t base = 0; base < k.n_prev; base += TRACK_THREADS) n += __popcll(__ballot(track_match(k, base + tid) >= 0));
    if ((tid & 63) == 0) wsum[tid >> 6] = n;
    __syncthreads();
    if (tid == 0) g_(counts)[(size_t)kind * B + b] = wsum[0] + wsum[1] + wsum[2] + wsum[3];
}

// K109
__global__ void __launch_bounds__(TRACK_THREADS) k_track_scan(const int32_t* counts, int32_t B, int32_t chunk, int32_t* pt_off,
                                                              int32_t* ls_off)
{
    __shared__ int32_t part[TRACK_THREADS];
    const int tid = threadIdx.x;
    const int32_t b0 = tid * chunk < B ? tid * chunk : B, b1 = b0 + chunk < B ? b0 + chunk : B;
    for (int kind = 0; kind < 2; ++kind) {
        const int32_t* c = counts + (size_t)kind * B;
        int32_t* off = kind ? ls_off : pt_off;
        int32_t s = 0;
        for (int32_t b = b0; b < b1; ++b) s += g_(c)[b];
        part[tid] = s;
        __syncthreads();
        int32_t at = 0;
        for (int t = 0; t < tid; ++t) at += part[t];
        for (int32_t b = b0; b < b1; ++b) {
            g_(off)[b] = at;
            at += g_(c)[b];
        }
        if (tid == TRACK_THREADS - 1) g_(off)[B] = at;              // (the last lane's `at` ends as the total: b1 = B there)
        __syncthreads();
    }
}

// K110
__global__ void __launch_bounds__(TRACK_THREADS) k_track_write(const plslam_track_pair* pairs, TrackCam cam, TrackOut o)
{
    __shared__ plslam_track_pair pr;
    __shared__ int32_t wsum[TRACK_THREADS / 64];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, b = blockIdx.x, kind = blockIdx.y;
    const TrackKind k = load_kind(pr, pairs, b, kind);
    const int32_t* off = kind ? o.ls_off : o.pt_off;
    const int32_t row1 = g_(off)[b + 1];
    int32_t total = g_(off)[b];
    for (int32_t base = 0; base < k.n_prev; base += TRACK_THREADS) {
        const int32_t i1 = base + tid, i2 = track_match(k, i1);
        const bool f = i2 >= 0;
        const uint64_t bal = __ballot(f);
        const int below = __popcll(bal & ((uint64_t(1) << lane) - 1));
        if (lane == 0) wsum[wv] = __popcll(bal);
        __syncthreads();
        int32_t at = total;
        for (int w = 0; w < wv; ++w) at += wsum[w];
        total += wsum[0] + wsum[1] + wsum[2] + wsum[3];
        const int32_t r = at + below;
        if (f && r < row1) {
            int32_t* rows = kind ? o.ls_rows : o.pt_rows;
            g_(rows)[2 * (size_t)r] = i1;
            g_(rows)[2 * (size_t)r + 1] = i2;
            if (kind)
                track_line_row(cam, k.f_prev, i1, g_(k.disp)[2 * (size_t)i1], g_(k.disp)[2 * (size_t)i1 + 1], k.f_curr, i2,
                               o.sPeP + 6 * (size_t)r, o.le + 3 * (size_t)r);
            else
                track_point_row(cam, k.f_prev, i1, g_(k.disp)[i1], k.f_curr, i2, o.P + 3 * (size_t)r, o.pl + 2 * (size_t)r);
        }
        __syncthreads();
    }
}

// K110f: one lane per left row of one frame
__global__ void __launch_bounds__(TRACK_THREADS) k_stereo_backproject(TrackCam cam, const int32_t* st, const double* disp,
                                                                      const float* f, int32_t n, int32_t lines, double* a, double* o)
{
    const int32_t i = (int32_t)(blockIdx.x * TRACK_THREADS + threadIdx.x);
    if (i >= n) return;
    const int wa = lines ? 6 : 3, wo = lines ? 3 : 2;
    if (g_(st)[i] < 0) {
        for (int q = 0; q < wa; ++q) g_(a)[wa * (size_t)i + q] = 0.0;
        for (int q = 0; q < wo; ++q) g_(o)[wo * (size_t)i + q] = 0.0;
    } else if (lines) {
        track_line_row(cam, f, i, g_(disp)[2 * (size_t)i], g_(disp)[2 * (size_t)i + 1], f, i, a + 6 * (size_t)i, o + 3 * (size_t)i);
    } else {
        track_point_row(cam, f, i, g_(disp)[i], f, i, a + 3 * (size_t)i, o + 2 * (size_t)i);
    }
}

TrackCam track_cam(const plslam_cam& c) { return TrackCam{c.fx, c.cx, c.cy, c.b}; }

}  // namespace
}  // namespace plslam

extern "C" {

int plslam_track_batch_create(plslam_ctx* ctx, const plslam_lc_params* params, const plslam_track_pair* pairs, int32_t B,
                              plslam_track_batch** out)
{
    using namespace plslam;
    int rc;
    if (out) *out = nullptr;
    TrackCaps caps;
    if ((rc = track_check(ctx, params, pairs, B, out, caps)) || (rc = lc_check_params(params))) return rc;
    plslam_track_batch* bt = new (std::nothrow) plslam_track_batch();
    PLSLAM_REQUIRE(bt != nullptr, PLSLAM_ENOMEM);
    bt->ctx = ctx;
    bt->p = *params;
    bt->B = B;
    bt->caps = caps;
    bt->L = track_layout(B, caps);
    if (B > 0) {
        std::lock_guard<std::mutex> lk(ctx->mu);
        DeviceGuard guard(ctx->device);
        // the records go up from the caller's array: the copy is waited for, the array may go when this returns
        rc = bt->buf.reserve(bt->L.bytes);
        if (rc == PLSLAM_OK && hipMemcpy(bt->at<char>(TB_PAIRS), pairs, bt->L.bytes_of[TB_PAIRS], hipMemcpyHostToDevice) != hipSuccess) {
            set_last_error("%s:%d: the upload of the pair records failed", __FILE__, __LINE__);
            rc = PLSLAM_EHIP;
        }
        if (rc != PLSLAM_OK) bt->buf.release();
    }
    if (rc != PLSLAM_OK) {
        delete bt;
        return rc;
    }
    *out = bt;
    return PLSLAM_OK;
}

int plslam_track_batch_run(plslam_track_batch* batch, void* stream)
{
    using namespace plslam;
    PLSLAM_REQUIRE(batch != nullptr, PLSLAM_EINVAL);
    const TrackLaunches T = track_launches(batch->B);
    if (T.n == 0) return PLSLAM_OK;
    plslam_ctx* ctx = batch->ctx;
    std::lock_guard<std::mutex> lk(ctx->mu);
    DeviceGuard guard(ctx->device);
    hipStream_t s = stream ? static_cast<hipStream_t>(stream) : ctx->stream;
    const plslam_track_pair* pairs = batch->at<plslam_track_pair>(TB_PAIRS);
    int32_t* counts = batch->at<int32_t>(TB_COUNTS);
    TrackOut o{batch->at<int32_t>(TB_PT_OFF), batch->at<int32_t>(TB_LS_OFF), batch->at<int32_t>(TB_PT_ROWS), batch->at<int32_t>(TB_LS_ROWS),
               batch->at<double>(TB_P), batch->at<double>(TB_PL), batch->at<double>(TB_SPEP), batch->at<double>(TB_LE)};
    hipLaunchKernelGGL(k_track_count, dim3(T.count.gx, T.count.gy), dim3(T.count.threads), 0, s, pairs, batch->B, counts);
    hipLaunchKernelGGL(k_track_scan, dim3(T.scan.gx, T.scan.gy), dim3(T.scan.threads), 0, s, counts, batch->B,
                       track_scan_chunk(batch->B), batch->at<int32_t>(TB_PT_OFF), batch->at<int32_t>(TB_LS_OFF));
    hipLaunchKernelGGL(k_track_write, dim3(T.write.gx, T.write.gy), dim3(T.write.threads), 0, s, pairs, track_cam(batch->p.cam), o);
    PLSLAM_HIP_CHECK(hipGetLastError());
    // K54 on the context's stream, fenced against `s` on both sides: behind the rows, in front of what `s` is given next
    return lc_relpose_batched_unlocked(ctx, &batch->p, o.P, o.pl, o.pt_off, o.sPeP, o.le, o.ls_off, batch->B,
                                       batch->at<plslam_lc_result>(TB_RESULTS), batch->at<uint8_t>(TB_PT_INL),
                                       batch->at<uint8_t>(TB_LS_INL), s);
}

int plslam_track_batch_device_buffers(plslam_track_batch* batch, plslam_track_buffers* out)
{
    using namespace plslam;
    PLSLAM_REQUIRE(batch && out, PLSLAM_EINVAL);
    *out = track_buffers(batch->L, batch->buf.as<char>(), batch->B, batch->caps);
    return PLSLAM_OK;
}

int plslam_track_batch_download(plslam_track_batch* batch, int32_t* pt_off, int32_t* ls_off, int32_t* pt_rows, int32_t* ls_rows,
                                double* P, double* pl_obs, double* sPeP, double* le_obs, uint8_t* pt_inlier, uint8_t* ls_inlier,
                                plslam_lc_result* results)
{
    using namespace plslam;
    PLSLAM_REQUIRE(batch != nullptr, PLSLAM_EINVAL);
    if (batch->B == 0) return PLSLAM_OK;
    plslam_ctx* ctx = batch->ctx;
    std::lock_guard<std::mutex> lk(ctx->mu);
    DeviceGuard guard(ctx->device);
    const TrackLayout& L = batch->L;
    void* const dst[TB_COUNT] = {nullptr, nullptr, pt_off, ls_off, pt_rows, ls_rows, P, pl_obs, sPeP, le_obs, pt_inlier, ls_inlier, results};
    DownloadItem items[TB_COUNT];
    for (int i = 0; i < TB_COUNT; ++i) items[i] = DownloadItem{dst[i], batch->at<char>(i), L.bytes_of[i]};
    return download_items(items, ctx->stream);
}

void plslam_track_batch_destroy(plslam_track_batch* batch)
{
    using namespace plslam;
    if (!batch) return;
    {
        std::lock_guard<std::mutex> lk(batch->ctx->mu);
        DeviceGuard guard(batch->ctx->device);
        (void)hipStreamSynchronize(batch->ctx->stream);
        batch->buf.release();
    }
    delete batch;
}

int plslam_stereo_backproject_dev(plslam_ctx* ctx, const plslam_cam* cam, const int32_t* stereo_12, const double* disp,
                                  const float* f_l, int32_t n_l, int32_t lines, double* P_or_sPeP, double* pl_or_le, void* stream)
{
    using namespace plslam;
    PLSLAM_REQUIRE(ctx && cam && n_l >= 0, PLSLAM_EINVAL);
    PLSLAM_REQUIRE(n_l == 0 || (stereo_12 && disp && f_l && P_or_sPeP && pl_or_le), PLSLAM_EINVAL);
    if (n_l == 0) return PLSLAM_OK;
    std::lock_guard<std::mutex> lk(ctx->mu);
    DeviceGuard guard(ctx->device);
    hipStream_t s = stream ? static_cast<hipStream_t>(stream) : ctx->stream;
    hipLaunchKernelGGL(k_stereo_backproject, dim3((unsigned)((n_l + TRACK_THREADS - 1) / TRACK_THREADS)), dim3(TRACK_THREADS), 0, s,
                       track_cam(*cam), stereo_12, disp, f_l, n_l, lines ? 1 : 0, P_or_sPeP, pl_or_le);
    PLSLAM_HIP_CHECK(hipGetLastError());
    return PLSLAM_OK;
}

}  // extern "C"
