// lc_correct.hip -- the map correction behind the loop-closure pose graph (MapHandler::loopClosureOptimizationCovGraphG2O,
// src/mapHandler.cpp:4306-4355 / :4364-4397): the rigid re-anchoring of every landmark by the T_corr of the keyframes that
// anchor it.  It shares nothing with the graph (pgo.hip) but T_corr and the corrected flags.
//   K50 k_lc_count             a lane per anchor entry: its slot, a count per landmark that a corrected slot lists
//   K51 k_lc_scan              one workgroup: the counts' exclusive prefix sum
//   K52 k_lc_fill              a lane per anchor entry: its place in its landmark's list
//   K53 k_lc_apply<DL>         a lane per landmark: its anchors' T_corr in anchor order applied to X, med_obs_dir and every
//                              dir_list entry
// No floating-point atomics: the integer atomics only place list entries, whose order K53 restores.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "common.hpp"
#include "se3_dev.hpp"

namespace plslam {
namespace {

// ---- K50-K53: the map correction ---------------------------------------------------------------------------------------------
// K50: a lane per anchor entry: its slot (binary search of the CSR), a count per landmark that a corrected slot lists
__global__ void __launch_bounds__(256)
k_lc_count(const int32_t* __restrict__ aptr, int32_t nslot, const int32_t* __restrict__ aidx, int32_t na, int32_t nlm,
           const uint8_t* __restrict__ corrected, int32_t* __restrict__ eslot, int32_t* __restrict__ cnt)
{
    const int a = blockIdx.x * 256 + threadIdx.x;
    if (a >= na) return;
    int lo = 0, hi = nslot;                       // the last slot s with aptr[s] <= a
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (aptr[mid] <= a) lo = mid; else hi = mid;
    }
    const int j = aidx[a];
    const bool use = j >= 0 && j < nlm && corrected[lo];
    eslot[a] = use ? lo : -1;
    if (use) atomic_add_global(cnt + j, 1);
}
// K51: one workgroup: exclusive prefix sum of the counts -> ptr (n + 1); the fill cursors start at 0
__global__ void __launch_bounds__(1024)
k_lc_scan(int32_t* __restrict__ cnt, int32_t n, int32_t* __restrict__ ptr)
{
    __shared__ int32_t part[1024];
    const int t = threadIdx.x;
    const int per = (n + 1023) / 1024, a0 = min(n, t * per), a1 = min(n, a0 + per);
    int s = 0;
    for (int i = a0; i < a1; ++i) s += cnt[i];
    part[t] = s;
    __syncthreads();
    for (int h = 1; h < 1024; h <<= 1) {
        const int v = t >= h ? part[t - h] : 0;
        __syncthreads();
        part[t] += v;
        __syncthreads();
    }
    int run = t ? part[t - 1] : 0;
    for (int i = a0; i < a1; ++i) { ptr[i] = run; run += cnt[i]; cnt[i] = 0; }
    if (t == 1023) ptr[n] = part[1023];
}
// K52: a lane per anchor entry: its place in its landmark's list (the order inside a list is restored by K53)
__global__ void __launch_bounds__(256)
k_lc_fill(const int32_t* __restrict__ aidx, const int32_t* __restrict__ eslot, int32_t na, const int32_t* __restrict__ ptr,
          int32_t* __restrict__ cur, int32_t* __restrict__ list)
{
    const int a = blockIdx.x * 256 + threadIdx.x;
    if (a >= na || eslot[a] < 0) return;
    const int j = aidx[a];
    list[ptr[j] + atomic_add_global(cur + j, 1)] = a;
}
// K53: a lane per landmark: its anchor entries in CSR order (slot order), each applying that slot's T_corr
template <int DL>
__global__ void __launch_bounds__(256)
k_lc_apply(const int32_t* __restrict__ ptr, int32_t* __restrict__ list, const int32_t* __restrict__ eslot,
           const uint8_t* __restrict__ valid, int32_t n, const double* __restrict__ T_corr, double* __restrict__ X,
           double* __restrict__ med, const int32_t* __restrict__ dptr, double* __restrict__ dirs)
{
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= n || !valid[j]) return;
    const int p0 = ptr[j], p1 = ptr[j + 1];
    if (p1 == p0) return;
    for (int a = p0 + 1; a < p1; ++a) {           // insertion sort: the entries of one landmark are few
        const int v = list[a];
        int b = a - 1;
        while (b >= p0 && list[b] > v) { list[b + 1] = list[b]; --b; }
        list[b + 1] = v;
    }
    const int d0 = dptr[j], d1 = dptr[j + 1];
    for (int a = p0; a < p1; ++a) {
        const double* C = T_corr + 16 * (size_t)eslot[list[a]];
        double c[12];
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int q = 0; q < 4; ++q) c[4 * i + q] = C[4 * i + q];
        double p[3];
#pragma unroll
        for (int h = 0; h < DL / 3; ++h) {
#pragma unroll
            for (int q = 0; q < 3; ++q) p[q] = X[(size_t)DL * j + 3 * h + q];
            xform(c, p, p);
#pragma unroll
            for (int q = 0; q < 3; ++q) X[(size_t)DL * j + 3 * h + q] = p[q];
        }
#pragma unroll
        for (int q = 0; q < 3; ++q) p[q] = med[3 * (size_t)j + q];
        xform(c, p, p);
#pragma unroll
        for (int q = 0; q < 3; ++q) med[3 * (size_t)j + q] = p[q];
        for (int d = d0; d < d1; ++d) {
#pragma unroll
            for (int q = 0; q < 3; ++q) p[q] = dirs[3 * (size_t)d + q];
            xform(c, p, p);
#pragma unroll
            for (int q = 0; q < 3; ++q) dirs[3 * (size_t)d + q] = p[q];
        }
    }
}

// the map correction of one kind on stream s; scratch: 2 n + 1 + 2 n_anchor int32
int lc_correct_enqueue(int32_t n_map, const double* T_corr, const uint8_t* corrected, const plslam_lc_landmarks* L, int dl,
                       int32_t* scratch, hipStream_t s)
{
    if (!L || L->n == 0 || L->n_anchor == 0) return PLSLAM_OK;
    int32_t* cnt = scratch;
    int32_t* ptr = cnt + L->n;
    int32_t* eslot = ptr + L->n + 1;
    int32_t* list = eslot + L->n_anchor;
    PLSLAM_HIP_CHECK(hipMemsetAsync(cnt, 0, (size_t)L->n * 4, s));
    const unsigned ga = (unsigned)((L->n_anchor + 255) / 256), gl = (unsigned)((L->n + 255) / 256);
    hipLaunchKernelGGL(k_lc_count, dim3(ga), dim3(256), 0, s, L->anchor_ptr, n_map, L->anchor_idx, L->n_anchor, L->n, corrected,
                       eslot, cnt);
    hipLaunchKernelGGL(k_lc_scan, dim3(1), dim3(1024), 0, s, cnt, L->n, ptr);
    hipLaunchKernelGGL(k_lc_fill, dim3(ga), dim3(256), 0, s, L->anchor_idx, (const int32_t*)eslot, L->n_anchor,
                       (const int32_t*)ptr, cnt, list);
    if (dl == 3)
        hipLaunchKernelGGL(k_lc_apply<3>, dim3(gl), dim3(256), 0, s, (const int32_t*)ptr, list, (const int32_t*)eslot, L->valid,
                           L->n, T_corr, L->X, L->med_dir, L->dir_ptr, L->dirs);
    else
        hipLaunchKernelGGL(k_lc_apply<6>, dim3(gl), dim3(256), 0, s, (const int32_t*)ptr, list, (const int32_t*)eslot, L->valid,
                           L->n, T_corr, L->X, L->med_dir, L->dir_ptr, L->dirs);
    PLSLAM_HIP_CHECK(hipGetLastError());
    return PLSLAM_OK;
}

bool lm_ok(const plslam_lc_landmarks* L)
{
    return !L || L->n == 0 ||
           (L->n > 0 && L->n_anchor >= 0 && L->n_dir >= 0 && L->anchor_ptr && (L->n_anchor == 0 || L->anchor_idx) && L->valid &&
            L->X && L->med_dir && L->dir_ptr && (L->n_dir == 0 || L->dirs));
}

size_t scratch_ints(const plslam_lc_landmarks* L) { return L ? 2 * (size_t)L->n + 1 + 2 * (size_t)L->n_anchor : 0; }

// the device image of one kind's host arrays (plslam_lc_correct_map): carved once, uploaded from and downloaded into L
struct LcKindView {
    Arr<int32_t> anchor_ptr, anchor_idx;
    Arr<uint8_t> valid;
    Arr<double> X, med_dir;
    Arr<int32_t> dir_ptr;
    Arr<double> dirs;
};
void carve_lc_kind(ArrCarver& c, int32_t n_map_kf, const plslam_lc_landmarks& L, int dl, LcKindView& v)
{
    const size_t n = (size_t)L.n;
    v.anchor_ptr = c.take<int32_t>(((size_t)n_map_kf + 1) * 4);
    v.anchor_idx = c.take<int32_t>((size_t)L.n_anchor * 4, 4);
    v.valid = c.take<uint8_t>(n, 8);
    v.X = c.take<double>(n * dl * 8);
    v.med_dir = c.take<double>(n * 24);
    v.dir_ptr = c.take<int32_t>((n + 1) * 4);
    v.dirs = c.take<double>((size_t)L.n_dir * 24, 8);
}
struct LcImageView {
    Arr<double> T_corr;
    Arr<uint8_t> corrected;
    LcKindView k[2];
};
size_t carve_lc_image(LcImageView& v, int32_t n_map_kf, const plslam_lc_landmarks* const kinds[2], char* base)
{
    ArrCarver c{base};
    v.T_corr = c.take<double>((size_t)n_map_kf * 128);
    v.corrected = c.take<uint8_t>((size_t)n_map_kf, 8);
    for (int k = 0; k < 2; ++k)
        if (kinds[k] && kinds[k]->n) carve_lc_kind(c, n_map_kf, *kinds[k], k ? 6 : 3, v.k[k]);
    return c.size();
}

}  // namespace
}  // namespace plslam

using namespace plslam;

extern "C" {

int plslam_lc_correct_map_dev(plslam_ctx* ctx, int32_t n_map_kf, const double* T_corr, const uint8_t* corrected,
                              const plslam_lc_landmarks* points, const plslam_lc_landmarks* lines, void* stream)
{
    PLSLAM_REQUIRE(ctx && n_map_kf >= 1 && T_corr && corrected && lm_ok(points) && lm_ok(lines), PLSLAM_EINVAL);
    std::lock_guard<std::mutex> lk(ctx->mu);
    DeviceGuard dg_(ctx->device);
    hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
    const size_t need = std::max(scratch_ints(points), scratch_ints(lines)) * 4 + 256;
    // the scratch is the context's: whatever used it before on another stream is finished first
    PLSLAM_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    int rc = ctx->pgo_scratch.reserve(need);
    if (rc) return rc;
    StreamSyncOnError guard(s);
    int32_t* scr = ctx->pgo_scratch.as<int32_t>();
    if ((rc = lc_correct_enqueue(n_map_kf, T_corr, corrected, points, 3, scr, s))) return rc;
    if ((rc = lc_correct_enqueue(n_map_kf, T_corr, corrected, lines, 6, scr, s))) return rc;
    // the scratch is reused by the next call: the correction is finished when this returns
    PLSLAM_HIP_CHECK(hipStreamSynchronize(s));
    guard.dismiss();
    return PLSLAM_OK;
}

int plslam_lc_correct_map(plslam_ctx* ctx, int32_t n_map_kf, const double* T_corr, const uint8_t* corrected,
                          const plslam_lc_landmarks* points, const plslam_lc_landmarks* lines)
{
    PLSLAM_REQUIRE(ctx && n_map_kf >= 1 && T_corr && corrected && lm_ok(points) && lm_ok(lines), PLSLAM_EINVAL);
    // host arrays -> one device image, the _dev form on the context's stream, the landmarks back
    const plslam_lc_landmarks* kinds[2] = {points, lines};
    LcImageView v;
    DevBuf buf;
    plslam_lc_landmarks dev[2] = {};
    {
        std::lock_guard<std::mutex> lk(ctx->mu);
        DeviceGuard dg_(ctx->device);
        hipStream_t s = ctx->stream;
        int rc = buf.reserve(carve_lc_image(v, n_map_kf, kinds, nullptr) + 256);
        if (rc) return rc;
        carve_lc_image(v, n_map_kf, kinds, buf.as<char>());
        StreamSyncOnError guard(s);
        const UploadItem head[] = {{v.T_corr, T_corr}, {v.corrected, corrected}};
        if ((rc = upload_items(head, s))) return rc;
        for (int k = 0; k < 2; ++k) {
            const plslam_lc_landmarks* L = kinds[k];
            if (!L || L->n == 0) continue;
            const LcKindView& K = v.k[k];
            const UploadItem ups[] = {{K.anchor_ptr, L->anchor_ptr}, {K.anchor_idx, L->anchor_idx}, {K.valid, L->valid}, {K.X, L->X},
                                      {K.med_dir, L->med_dir}, {K.dir_ptr, L->dir_ptr}, {K.dirs, L->dirs}};
            if ((rc = upload_items(ups, s))) return rc;
            dev[k] = *L;
            dev[k].anchor_ptr = K.anchor_ptr; dev[k].anchor_idx = K.anchor_idx; dev[k].valid = K.valid; dev[k].X = K.X;
            dev[k].med_dir = K.med_dir; dev[k].dir_ptr = K.dir_ptr; dev[k].dirs = K.dirs;
        }
        PLSLAM_HIP_CHECK(hipStreamSynchronize(s));
        guard.dismiss();
    }
    int rc = plslam_lc_correct_map_dev(ctx, n_map_kf, v.T_corr, v.corrected, points ? &dev[0] : nullptr, lines ? &dev[1] : nullptr,
                                       nullptr);
    std::lock_guard<std::mutex> lk(ctx->mu);
    DeviceGuard dg2_(ctx->device);
    hipStream_t s = ctx->stream;
    ReleaseAfterSync rel{buf, s};
    if (rc) return rc;
    for (int k = 0; k < 2; ++k) {
        const plslam_lc_landmarks* L = kinds[k];
        if (!L || L->n == 0) continue;
        const DownloadItem back[] = {{L->X, v.k[k].X, v.k[k].X.bytes}, {L->med_dir, v.k[k].med_dir, v.k[k].med_dir.bytes},
                                     {L->dirs, v.k[k].dirs, v.k[k].dirs.bytes}};
        for (const DownloadItem& it : back)
            if (it.bytes) PLSLAM_HIP_CHECK(hipMemcpyAsync(it.dst, it.src, it.bytes, hipMemcpyDeviceToHost, s));
    }
    PLSLAM_HIP_CHECK(hipStreamSynchronize(s));
    return PLSLAM_OK;
}

}  // extern "C"
