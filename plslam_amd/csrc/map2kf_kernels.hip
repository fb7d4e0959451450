// map2kf_kernels.hip -- the kernels of the map <-> keyframe and keyframe <-> keyframe drivers (map2kf.hip) and of the gate and
// visibility host calls (host_calls.hip): K5/K6 (the epipolar gates), the visibility pre-filter, the projection into grid cells,
// the one-synchronisation form's fused steps (k_visible_compact, k_prepare_rows), the row gather and the counters' publish.
// Their launchers are declared in map2kf_dev.hpp.
//
// fp64 elementwise work, one lane per landmark.  The translation unit is compiled with -ffp-contract=off and every expression
// keeps the reference's source order (src/mapHandler.cpp:605-613, :720-729) so that thresholded results (inlier masks) are
// reproducible bit for bit against the CPU restatement.
#include "lba_rows_dev.hpp"
#include "lookback_dev.hpp"
#include "map2kf_dev.hpp"
#include "map2kf_plan.hpp"  // VC_NT, visible_compact_part_words
#include "match_grid.hpp"   // GridDesc: k_visible_compact writes the row count into a descriptor
#include "publish_dev.hpp"

namespace plslam {

struct Pose12 { double m[12]; };  // rows 0..2 of the row-major 4x4

// The gates as the LAST kernel of a one-synchronisation driver call (map2kf.hip): the workgroup that finishes last copies the call's
// counters (device words, some of them this kernel's own atomic counts) into the page-locked block the host reads (publish_dev.hpp).
// pub.done = nullptr: nothing to publish, and no wave waits for its count; count = nullptr: nothing is counted.
__device__ __forceinline__ void gate_count_and_publish(int ok, int32_t* __restrict__ count, const Publish& pub)
{
    if (count) {
        if (pub.done) wave_count_and_wait(ok, count);
        else {
            const unsigned long long b = __ballot(ok);
            if ((threadIdx.x & 63) == 0 && b) atomicAdd(count, (int)__popcll(b));
        }
    }
    if (pub.done) publish_from_last_workgroup(pub);
}

// K5: point gate  (:601-613)
__global__ void __launch_bounds__(256)
k_point_gate(CamD K, Pose12 Twf, const double* __restrict__ Xw, const int32_t* __restrict__ m12,
             int32_t nq, const double* __restrict__ pl, double th, uint8_t* __restrict__ mask,
             int32_t* __restrict__ count, const int32_t* __restrict__ nq_dev, const int32_t* __restrict__ idx,
             const int32_t* __restrict__ ti, int32_t* __restrict__ map_to_kf, Publish pub)
{
    if (nq_dev) nq = *nq_dev;                  // (the row count lives on the device: the launch covers an upper bound)
    const int i = blockIdx.x * 256 + threadIdx.x;
    int ok = 0;
    if (i < nq) {
        const int i2 = m12[i];
        if (i2 >= 0) {
            double Pf[3], u, v;
            xform(Twf.m, Xw + 3 * (size_t)i, Pf);
            project(K, Pf, u, v);
            const double ex = u - pl[2 * (size_t)i2], ey = v - pl[2 * (size_t)i2 + 1];
            ok = sqrt(ex * ex + ey * ey) < th;
        }
        mask[i] = (uint8_t)ok;
        if (ok && map_to_kf) map_to_kf[idx[i]] = ti[i2];          // :614-619, the association (table pre-filled with -1)
    }
    gate_count_and_publish(ok, count, pub);
}

// K6: line gate  (:716-729), signed test on both endpoints
__global__ void __launch_bounds__(256)
k_line_gate(CamD K, Pose12 Twf, const double* __restrict__ Lw, const int32_t* __restrict__ m12,
            int32_t nq, const double* __restrict__ le, double th, uint8_t* __restrict__ mask,
            int32_t* __restrict__ count, const int32_t* __restrict__ nq_dev, const int32_t* __restrict__ idx,
            const int32_t* __restrict__ ti, int32_t* __restrict__ map_to_kf, Publish pub)
{
    if (nq_dev) nq = *nq_dev;
    const int i = blockIdx.x * 256 + threadIdx.x;
    int ok = 0;
    if (i < nq) {
        const int i2 = m12[i];
        if (i2 >= 0) {
            double sP[3], eP[3], su, sv, eu, ev;
            xform(Twf.m, Lw + 6 * (size_t)i, sP);
            project(K, sP, su, sv);
            xform(Twf.m, Lw + 6 * (size_t)i + 3, eP);
            project(K, eP, eu, ev);
            const double lx = le[3 * (size_t)i2], ly = le[3 * (size_t)i2 + 1], lz = le[3 * (size_t)i2 + 2];
            const double e0 = lx * su + ly * sv + lz;
            const double e1 = lx * eu + ly * ev + lz;
            ok = (e0 < th) && (e1 < th);
        }
        mask[i] = (uint8_t)ok;
        if (ok && map_to_kf) map_to_kf[idx[i]] = ti[i2];
    }
    gate_count_and_publish(ok, count, pub);
}

__device__ __forceinline__ int inside(const CamD& K, const double P[3])
{
    double u, v;
    project(K, P, u, v);
    return u > 0 && u < K.width && v > 0 && v < K.height && P[2] > 0.0;
}

// candidate pre-filter (:549-551, :650-655)
__global__ void __launch_bounds__(256)
k_visible(CamD K, Pose12 Twf, const double* __restrict__ X, int32_t n, int lines,
          uint8_t* __restrict__ vis, const uint8_t* __restrict__ cand)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const bool c = cand == nullptr || cand[i] != 0;      // (cand: the caller's candidate flags live on the device -- folded in)
    double P[3];
    if (!lines) {
        xform(Twf.m, X + 3 * (size_t)i, P);
        vis[i] = (uint8_t)(c && inside(K, P));
    } else {
        double E[3];
        xform(Twf.m, X + 6 * (size_t)i, P);
        xform(Twf.m, X + 6 * (size_t)i + 3, E);
        vis[i] = (uint8_t)(c && inside(K, P) && inside(K, E));
    }
}

static Pose12 pose12(const double* T16)
{
    Pose12 p;
    for (int i = 0; i < 12; ++i) p.m[i] = T16[i];
    return p;
}

int launch_point_gate(const plslam_cam& K, const double* Twf16, const double* Xw, const int32_t* m12,
                      int32_t nq, const double* pl, double th, uint8_t* mask, int32_t* count,
                      hipStream_t s)
{
    if (count) PLSLAM_HIP_CHECK(hipMemsetAsync(count, 0, sizeof(int32_t), s));
    if (nq <= 0) return PLSLAM_OK;
    hipLaunchKernelGGL(k_point_gate, dim3((nq + 255) / 256), dim3(256), 0, s, cam_d(K), pose12(Twf16),
                       Xw, m12, nq, pl, th, mask, count, (const int32_t*)nullptr, (const int32_t*)nullptr, (const int32_t*)nullptr,
                       (int32_t*)nullptr, Publish{nullptr, nullptr, nullptr, 0});
    PLSLAM_HIP_CHECK(hipGetLastError());
    return PLSLAM_OK;
}

int launch_line_gate(const plslam_cam& K, const double* Twf16, const double* Lw, const int32_t* m12,
                     int32_t nq, const double* le, double th, uint8_t* mask, int32_t* count,
                     hipStream_t s)
{
    if (count) PLSLAM_HIP_CHECK(hipMemsetAsync(count, 0, sizeof(int32_t), s));
    if (nq <= 0) return PLSLAM_OK;
    hipLaunchKernelGGL(k_line_gate, dim3((nq + 255) / 256), dim3(256), 0, s, cam_d(K), pose12(Twf16),
                       Lw, m12, nq, le, th, mask, count, (const int32_t*)nullptr, (const int32_t*)nullptr, (const int32_t*)nullptr,
                       (int32_t*)nullptr, Publish{nullptr, nullptr, nullptr, 0});
    PLSLAM_HIP_CHECK(hipGetLastError());
    return PLSLAM_OK;
}

int launch_visible(const plslam_cam& K, const double* Twf16, const double* X, int32_t n, int lines,
                   uint8_t* vis, hipStream_t s)
{
    if (n <= 0) return PLSLAM_OK;
    hipLaunchKernelGGL(k_visible, dim3((n + 255) / 256), dim3(256), 0, s, cam_d(K), pose12(Twf16), X, n,
                       lines, vis, (const uint8_t*)nullptr);
    PLSLAM_HIP_CHECK(hipGetLastError());
    return PLSLAM_OK;
}
// ... AND the candidate flags (device): what the drivers with a device-resident map read back
int launch_visible_cand(const plslam_cam& K, const double* Twf16, const double* X, const uint8_t* cand, int32_t n, int lines,
                        uint8_t* vis, hipStream_t s)
{
    if (n <= 0) return PLSLAM_OK;
    hipLaunchKernelGGL(k_visible, dim3((n + 255) / 256), dim3(256), 0, s, cam_d(K), pose12(Twf16), X, n,
                       lines, vis, cand);
    PLSLAM_HIP_CHECK(hipGetLastError());
    return PLSLAM_OK;
}

// pj_points / pj_lines of the fast_matching drivers (:553-555, :656-661): projection of the (already gathered)
// candidate landmarks in grid units, truncated toward zero as std::make_pair<int,int>(double, double) does; for
// lines also the unit direction matchGrid derives from the two INTEGER end points (zero vector -> NaN)
__global__ void __launch_bounds__(256)
k_project_cells(CamD K, Pose12 Twf, const double* __restrict__ X, int32_t n, int lines, double inv_w, double inv_h,
                int32_t* __restrict__ cells, double* __restrict__ dir1, const int32_t* __restrict__ n_dev)
{
    if (n_dev) n = *n_dev;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int nc = lines ? 2 : 1;
    int32_t c[4];
    // double -> int as the reference's x86 build does it (cvttsd2si): truncation; NaN / out of range -> INT_MIN
    auto cvtt = [](double v) -> int32_t { return (v > -2147483649.0 && v < 2147483648.0) ? (int32_t)v : INT32_MIN; };
    for (int e = 0; e < nc; ++e) {
        double P[3], u, v;
        xform(Twf.m, X + (size_t)i * 3 * nc + 3 * e, P);
        project(K, P, u, v);
        c[2 * e] = cvtt(u * inv_w);
        c[2 * e + 1] = cvtt(v * inv_h);
        cells[((size_t)i * nc + e) * 2] = c[2 * e];
        cells[((size_t)i * nc + e) * 2 + 1] = c[2 * e + 1];
    }
    if (lines) {
        const double vx = (double)c[2] - (double)c[0], vy = (double)c[3] - (double)c[1];
        const double magnitude = sqrt(vx * vx + vy * vy);
        dir1[2 * (size_t)i] = vx / magnitude;
        dir1[2 * (size_t)i + 1] = vy / magnitude;
    }
}

int launch_project_cells(const plslam_cam& K, const double* Twf16, const double* X, int32_t n, int lines, double inv_w,
                         double inv_h, int32_t* cells, double* dir1, hipStream_t s)
{
    if (n <= 0) return PLSLAM_OK;
    hipLaunchKernelGGL(k_project_cells, dim3((n + 255) / 256), dim3(256), 0, s, cam_d(K), pose12(Twf16), X, n, lines,
                       inv_w, inv_h, cells, dir1, (const int32_t*)nullptr);
    PLSLAM_HIP_CHECK(hipGetLastError());
    return PLSLAM_OK;
}

// The gates with the row count ON THE DEVICE (*n_dev <= n_max; the launch covers n_max rows): the drivers' one-synchronisation
// form builds its candidate list on the device and never learns its length before the results are back.  The gate's counter is
// NOT cleared here (the caller's image holds the zero); idx / ti / map_to_kf: the association of the rows that pass.
// publish_*: the call's counters (publish_n device words at publish_src) go to publish_dst -- page-locked, mapped -- from the last
// workgroup to finish; publish_done: a ZERO device word the workgroups count themselves into (nullptr: nothing is published)
int launch_gate_n(int lines, const plslam_cam& K, const double* Twf16, const double* LM, const int32_t* m12, const int32_t* n_dev,
                  int32_t n_max, const double* feat, double th, uint8_t* mask, int32_t* count, const int32_t* idx, const int32_t* ti,
                  int32_t* map_to_kf, hipStream_t s, int32_t* publish_done, const int32_t* publish_src, int32_t* publish_dst,
                  int32_t publish_n)
{
    if (n_max <= 0) {
        // (no gate workgroup will run: the counters still have to come down)
        PLSLAM_REQUIRE(!publish_done, PLSLAM_EINVAL);
        return PLSLAM_OK;
    }
    const Publish pub{publish_done, publish_src, publish_dst, publish_n};
    if (lines)
        hipLaunchKernelGGL(k_line_gate, dim3((n_max + 255) / 256), dim3(256), 0, s, cam_d(K), pose12(Twf16), LM, m12, n_max, feat,
                           th, mask, count, n_dev, idx, ti, map_to_kf, pub);
    else
        hipLaunchKernelGGL(k_point_gate, dim3((n_max + 255) / 256), dim3(256), 0, s, cam_d(K), pose12(Twf16), LM, m12, n_max, feat,
                           th, mask, count, n_dev, idx, ti, map_to_kf, pub);
    PLSLAM_HIP_CHECK(hipGetLastError());
    return PLSLAM_OK;
}


// ---- the map<->keyframe drivers' one-synchronisation form (map2kf.hip): its small kernels fused -- a launch of a
// microsecond's work costs 4-5 us on the timeline ------------------------------------------------------------------------------
// candidate pre-filter (:549-551, :650-655) x candidate flags -> the STABLE list of the landmarks that pass (ascending) + its
// length, the association table's -1 start, and the row count of the matchGrid problem that follows (its uploaded descriptor).
// A workgroup per 256 landmarks, all of them at once (a single workgroup evaluated 10 000 landmarks in 17 - 28 us: fp64 on one
// CU); a workgroup's survivors are counted by ballot and the list comes out ascending: a workgroup's first slot is the number of
// survivors in front of it, found by DECOUPLED LOOK-BACK (lookback_dev.hpp; round 6 -- rounds 3-5 summed ALL predecessors'
// counts, b words per workgroup b: fine at C3's 40 workgroups, 7.6 M polls at a 1 M-landmark map).  part: (n + 255) / 256 words,
// ZERO when the kernel starts (the drivers' upload image holds them).  VC_NT, the landmarks per workgroup: map2kf_plan.hpp.
__global__ void __launch_bounds__(VC_NT)
k_visible_compact(CamD K, Pose12 Twf, const double* __restrict__ X, const uint8_t* __restrict__ cand, int32_t n, int lines,
                  int32_t* __restrict__ idx, int32_t* __restrict__ n_out, int32_t* __restrict__ fill, GridDesc* __restrict__ desc,
                  uint32_t* __restrict__ part)
{
    constexpr int NW = VC_NT / 64;
    __shared__ uint32_t s_w[NW], s_before;
    const int tid = (int)threadIdx.x, b = (int)blockIdx.x;
    const int32_t i = b * VC_NT + tid;
    bool v = false;
    if (i < n) {                                            // (the landmark is read whether it is a candidate or not: one round trip)
        const uint8_t c = cand[i];
        double P[3], E[3];
        if (!lines) {
            xform(Twf.m, X + 3 * (size_t)i, P);
            v = c != 0 && inside(K, P) != 0;
        } else {
            xform(Twf.m, X + 6 * (size_t)i, P);
            xform(Twf.m, X + 6 * (size_t)i + 3, E);
            v = c != 0 && inside(K, P) && inside(K, E);
        }
        fill[i] = -1;
    }
    const TileScan sc = lookback_rank<NW>(v, part, b, s_w, &s_before);
    if (v) idx[sc.pos] = i;
    if (b == (int)gridDim.x - 1 && tid == 0) {
        *n_out = (int32_t)sc.upto;
        if (desc) desc->n1 = (int32_t)sc.upto;
    }
}

// Q matrix construction (:555, :567) + pj_points / pj_lines (k_project_cells): row a of Q = med_desc[idx[a]], of QL = LM[idx[a]],
// its window centre(s) from QL; a lane per listed landmark, *n_dev of them
__global__ void __launch_bounds__(256)
k_prepare_rows(CamD K, Pose12 Twf, const uint64_t* __restrict__ md, const double* __restrict__ lm, const int32_t* __restrict__ idx,
               const int32_t* __restrict__ n_dev, int lines, double inv_w, double inv_h, uint64_t* __restrict__ Q,
               double* __restrict__ QL, int32_t* __restrict__ cells, double* __restrict__ dir1)
{
    const int a = blockIdx.x * 256 + threadIdx.x;
    if (a >= *n_dev) return;
    const int64_t src = idx[a];
    const int nc = lines ? 2 : 1, lw = 3 * nc;
#pragma unroll
    for (int w = 0; w < 4; ++w) Q[(int64_t)a * 4 + w] = md[src * 4 + w];
    double X[6];
    for (int w = 0; w < lw; ++w) {
        X[w] = lm[src * lw + w];
        QL[(int64_t)a * lw + w] = X[w];
    }
    if (!cells) return;                                     // (the brute-force driver: no window centres)
    auto cvtt = [](double v) -> int32_t { return (v > -2147483649.0 && v < 2147483648.0) ? (int32_t)v : INT32_MIN; };
    int32_t c[4];
    for (int e = 0; e < nc; ++e) {
        double P[3], u, v;
        xform(Twf.m, X + 3 * e, P);
        project(K, P, u, v);
        c[2 * e] = cvtt(u * inv_w);
        c[2 * e + 1] = cvtt(v * inv_h);
        cells[((size_t)a * nc + e) * 2] = c[2 * e];
        cells[((size_t)a * nc + e) * 2 + 1] = c[2 * e + 1];
    }
    if (lines) {
        const double vx = (double)c[2] - (double)c[0], vy = (double)c[3] - (double)c[1];
        const double magnitude = sqrt(vx * vx + vy * vy);
        dir1[2 * (size_t)a] = vx / magnitude;
        dir1[2 * (size_t)a + 1] = vy / magnitude;
    }
}

// part: visible_compact_part_words(n) device words that must be ZERO when the kernel starts (its workgroups chain their counts
// through them; a stale word gives wrong offsets).  part_zeroed = true: the caller's upload image has just written the zeros
// on this stream (the drivers: no extra operation on their latency path); false: they are cleared here.
int launch_visible_compact(const plslam_cam& K, const double* Twf16, const double* X, const uint8_t* cand, int32_t n, int lines,
                           int32_t* idx, int32_t* n_out, int32_t* fill, GridDesc* desc, uint32_t* part, bool part_zeroed,
                           hipStream_t s)
{
    const unsigned nb = (unsigned)visible_compact_part_words(n);
    if (!part_zeroed) PLSLAM_HIP_CHECK(hipMemsetAsync(part, 0, sizeof(uint32_t) * nb, s));
    hipLaunchKernelGGL(k_visible_compact, dim3(nb), dim3(VC_NT), 0, s, cam_d(K), pose12(Twf16), X, cand, n, lines, idx, n_out, fill,
                       desc, part);
    PLSLAM_HIP_CHECK(hipGetLastError());
    return PLSLAM_OK;
}
int launch_prepare_rows(const plslam_cam& K, const double* Twf16, const void* md, const double* lm, const int32_t* idx,
                        const int32_t* n_dev, int32_t n_max, int lines, double inv_w, double inv_h, void* Q, double* QL, int32_t* cells,
                        double* dir1, hipStream_t s)
{
    if (n_max <= 0) return PLSLAM_OK;
    hipLaunchKernelGGL(k_prepare_rows, dim3((n_max + 255) / 256), dim3(256), 0, s, cam_d(K), pose12(Twf16),
                       static_cast<const uint64_t*>(md), lm, idx, n_dev, lines, inv_w, inv_h, static_cast<uint64_t*>(Q), QL, cells, dir1);
    PLSLAM_HIP_CHECK(hipGetLastError());
    return PLSLAM_OK;
}

// dst[i] = src[idx[i]] for rows of row_bytes (a multiple of 8) bytes: the step-by-step form's Q / T matrices
__global__ void __launch_bounds__(256)
k_gather_rows(const uint64_t* __restrict__ src, const int32_t* __restrict__ idx, int32_t n, int32_t words,
              uint64_t* __restrict__ dst)
{
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= (int64_t)n * words) return;
    const int32_t row = (int32_t)(t / words), w = (int32_t)(t % words);
    dst[t] = src[(int64_t)idx[row] * words + w];
}

int launch_gather_rows(const void* src, const int32_t* idx, int32_t n, int32_t row_bytes, void* dst,
                       hipStream_t s)
{
    if (n <= 0) return PLSLAM_OK;
    PLSLAM_REQUIRE(row_bytes % 8 == 0, PLSLAM_EINVAL);
    const int32_t words = row_bytes / 8;
    const int64_t total = (int64_t)n * words;
    hipLaunchKernelGGL(k_gather_rows, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s,
                       static_cast<const uint64_t*>(src), idx, n, words, static_cast<uint64_t*>(dst));
    PLSLAM_HIP_CHECK(hipGetLastError());
    return PLSLAM_OK;
}

// the drivers' counters, device -> the page-locked block the host reads (one lane per word): a LAUNCH behind the last kernel
// instead of a copy command -- on the timeline a small device-to-host copy starts ~13 us after the kernel in front of it, a kernel
// 2-3 us (profiles/r6_r_call_timeline_map2kf_points_fast.txt)
__global__ void k_publish_words(const int32_t* __restrict__ src, int32_t* __restrict__ dst, int n)
{
    if ((int)threadIdx.x < n) dst[threadIdx.x] = src[threadIdx.x];
}

int launch_publish_words(const int32_t* src, int32_t* dst, int n, hipStream_t s)
{
    hipLaunchKernelGGL(k_publish_words, dim3(1), dim3(64), 0, s, src, dst, n);
    PLSLAM_HIP_CHECK(hipGetLastError());
    return PLSLAM_OK;
}

}  // namespace plslam
