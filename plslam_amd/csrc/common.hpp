// common.hpp -- internal declarations shared by the HIP translation units of libplslam_hip.so.
// Nothing here is part of the ABI (see include/plslam_hip.h).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cstdio>
#include <mutex>
#include <vector>

#include "match_tables.hpp"   // ScanDesc, SymDesc, ProblemDesc, BlockDesc: the launch tables (no HIP header in there)
#include "plslam_hip.h"

namespace plslam {

void set_last_error(const char* fmt, ...);

#define PLSLAM_HIP_CHECK(expr)                                                              \
    do {                                                                                    \
        hipError_t e_ = (expr);                                                             \
        if (e_ != hipSuccess) {                                                             \
            ::plslam::set_last_error("%s:%d: %s -> %s", __FILE__, __LINE__, #expr,           \
                                     hipGetErrorString(e_));                                \
            return e_ == hipErrorOutOfMemory ? PLSLAM_ENOMEM : PLSLAM_EHIP;                 \
        }                                                                                   \
    } while (0)

#define PLSLAM_REQUIRE(cond, code)                                                          \
    do {                                                                                    \
        if (!(cond)) {                                                                      \
            ::plslam::set_last_error("%s:%d: requirement failed: %s", __FILE__, __LINE__,    \
                                     #cond);                                                \
            return (code);                                                                  \
        }                                                                                   \
    } while (0)

// grow-only device scratch buffer owned by a context
struct DevBuf {
    void* p = nullptr;
    size_t cap = 0;
    int reserve(size_t bytes);
    void release();
    template <class T> T* as() const { return static_cast<T*>(p); }
};
// pinned host memory (hipHostMalloc), grow-only: staging for the latency path of the host-pointer entry
// points -- copies from/to pinned memory are plain DMA enqueues, copies from pageable memory are not
struct HostBuf {
    void* p = nullptr;
    void* dev = nullptr;     // the device address of the block (mapped page-locked memory), nullptr if the device cannot address it
    size_t cap = 0;
    int reserve(size_t bytes);
    void release();
    template <class T> T* as() const { return static_cast<T*>(p); }
};

// ring of page-locked slots for small per-call host tables a kernel reads in place (lbd_float.hip: the line records)
struct LineRing {
    static constexpr int SLOTS = 4;
    HostBuf rec[SLOTS];
    hipEvent_t done[SLOTS] = {nullptr, nullptr, nullptr, nullptr};   // recorded behind the kernel that read the slot
    bool busy[SLOTS] = {false, false, false, false};
    int next = 0;
    void release()
    {
        for (int k = 0; k < SLOTS; ++k) {
            if (done[k]) (void)hipEventDestroy(done[k]);
            done[k] = nullptr;
            busy[k] = false;
            rec[k].release();
        }
    }
};

// the device address of page-locked, mapped host memory (hipHostMalloc / hipHostRegister), or nullptr
inline void* mapped_device_pointer(void* host)
{
    hipPointerAttribute_t at;
    if (!host || hipPointerGetAttributes(&at, host) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
    return at.type == hipMemoryTypeHost ? at.devicePointer : nullptr;
}

struct DeviceGuard {  // every entry point runs on the context's device
    int prev = -1;
    explicit DeviceGuard(int dev)
    {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        if (prev != dev) (void)hipSetDevice(dev);
        else prev = -1;
    }
    ~DeviceGuard()
    {
        if (prev >= 0) (void)hipSetDevice(prev);
    }
};

// Host-pointer entry points enqueue copies from stack / local objects and work on the context's shared scratch buffers:
// whatever way they return (PLSLAM_HIP_CHECK, `return rc`), nothing may still be in flight when the locals die and
// ctx->mu is released.  On the success path the stream is already idle and the extra synchronise costs a microsecond.
struct StreamSyncOnError {
    hipStream_t s;
    bool armed = true;
    explicit StreamSyncOnError(hipStream_t st) : s(st) {}
    void dismiss() { armed = false; }
    ~StreamSyncOnError()
    {
        if (armed) (void)hipStreamSynchronize(s);
    }
};

// a scratch buffer that lives for one call: whatever way the call returns, the stream is drained and the buffer freed
struct ReleaseAfterSync {
    DevBuf& b;
    hipStream_t s;
    ~ReleaseAfterSync()
    {
        (void)hipStreamSynchronize(s);
        b.release();
    }
};

// an array inside a carved buffer: where it starts and how many bytes of it are data (what an upload or a download copies;
// the slack the carving leaves behind it is not counted)
template <class T>
struct Arr {
    T* p = nullptr;
    size_t bytes = 0;
    operator T*() const { return p; }
};

// carves arrays out of the block at `base` in the order they are taken (Carver's alignment); base = nullptr: only the
// total is wanted (the buffer is reserved after its size is known, and carved again over its address)
struct ArrCarver {
    char* base;
    Carver c{};
    size_t size() const { return c.off; }
    template <class T> Arr<T> take(size_t bytes, size_t slack = 0) { return {reinterpret_cast<T*>(reinterpret_cast<uintptr_t>(base) + c.take(bytes + slack)), bytes}; }
};

// The upload of a plan's host-built lists into its carved arrays: each array's data bytes from the host vector behind it,
// enqueued on s (nothing is waited for).  The caller holds the context's lock and has selected its device.
struct UploadItem {
    void* dst;
    size_t bytes;
    const void* src;
    template <class T> UploadItem(const Arr<T>& a, const void* host) : dst(a.p), bytes(a.bytes), src(host) {}
};
template <size_t N> int upload_items(const UploadItem (&items)[N], hipStream_t s)
{
    for (const UploadItem& it : items)
        if (it.bytes) PLSLAM_HIP_CHECK(hipMemcpyAsync(it.dst, it.src, it.bytes, hipMemcpyHostToDevice, s));
    return PLSLAM_OK;
}

}  // namespace plslam

struct plslam_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    hipDeviceProp_t prop;
    int scan_variant = PLSLAM_SCAN_AUTO;
    int scan_block = 0;  // 0 = variant default
    int group_cap = 0;   // blocks of one problem kept together on one XCD; 0 = auto (match_planner.hpp, deal_to_xcds)
    int sym_rows = 0;    // rows of d1 per lane in the symmetric scan: 0 = auto, 1, 4
    int mfma_form = 0;   // matrix-core scan: 0 = auto (= 5), 1 = exact push per tile (K1e), 2 = grouped rows (K1f), 3 = directed pairs (K1g), 4 = grouped both ways (K1h), 5 = K1h with the M-tiles pipelined against each other (K1i)
    int col_split = 0;   // K1f, few large problems: 0 = auto (cut the columns into ranges when the plan cannot fill the chip), 1 = never, 2 = always
    int exact_second = 0; // K1h: 1 = the index of every second-best row key is exact (0: only where it is an output -- knnMatch)
    int graph = 1;             // plslam_match_plan_run as a replayed HIP graph: 0 = latency plans, 1 = never (default until measured), 2 = always
    int post_workgroups = 0;   // > 0: the stages behind a scan (merge of K1h's partials, finalize) run as at most this many workgroups walking their block tables
    int split_target = 0, split_min_tiles = 0;   // column split: workgroups per CU aimed at (0 = 3), tiles per column range at least (0 = 4)
    int split_post = 0;  // column-split K1f plans: 0 = auto (merge + ratio + mutual behind the scan in ONE kernel: two launches per run), 1 = never
    int post_xcd = 2;    // finalize: 0 = table order, 1 = an XCD takes contiguous entries of the block table (a problem's row blocks share one L2), 2 = the table dealt to the XCDs problem by problem (default)
    int zero_copy_kb = 64;  // (round 6) host-pointer calls of ONE small problem (plslam_match_grid): an upload image of at most this many KB is read by the kernel where it lies in page-locked host memory -- no H2D copy command in front of it -- when the dense one-workgroup kernel takes the problem (it reads every word once); negative: for every problem whose image fits; 0 = always copy
    int post_fuse = 0;   // K1h / K1i plans: merge + finalize + gates behind the scan as ONE kernel: 0 = auto (throughput plans), 1 = never, 2 = whenever eligible
    int fuse = 0;        // K1f: 0 = auto (one workgroup per problem incl. merge + finalize when the plan is large), 1 = never, 2 = always
    std::mutex mu;       // serialises the host-pointer entry points
    plslam::DevBuf in_a, in_b, out_a, out_b, misc_a, misc_b, misc_c;
    plslam::HostBuf pin_in, pin_out;                // pinned staging of small host-pointer calls
    plslam::HostBuf pin_misc;                       // host-built tables of the map-level drivers (map2kf.hip)
    plslam::LineRing lbd_ring;                      // line records of the last plslam_lbd_compute* calls
    struct plslam_match_plan* host_plan = nullptr;  // reused by the host-pointer match entry points
    struct plslam_match_plan* lc_plan = nullptr;    // the loop-closure check's two match problems (loop_closure.hip)
    plslam::DevBuf lc_in, lc_out, lc_tab;           // ... its keyframe image, its outputs, its match tables
    hipEvent_t lc_ev[2] = {nullptr, nullptr};       // ... its fences with a caller's stream (the _dev forms)
    plslam::DevBuf lc_args;                         // plslam_relpose_robust_gn_batched_dev: K54's argument table
    std::vector<char> lc_args_h;                    // ... and its host image (pageable: staged by the copy call itself)
    int lba_loop_peek = 1;                          // plslam_lba_plan_optimize_dev: 1 = the host looks at the mapped stop word between two passes and stops enqueuing, 0 = every pass is enqueued
    int pgo_solver = 0;                             // pgo plans created from now on: 0 = envelope L D L^T, 1 = the dense one (comparison)
    plslam::DevBuf pgo_scratch;                     // the map correction's per-landmark lists (lc_correct.hip)
    plslam::DevBuf lists_scratch;                   // the carries' chain words and touched-landmark lists (map_lists.hip)
    plslam::HostBuf lc_image_pin;                   // plslam_lc_correct_image: its counts, then its staged block (lc_correct_image.hip)
};

namespace plslam {

// The destroy of a handle that owns one device buffer and one page-locked block (plslam_local_map, plslam_map_insert,
// plslam_lc_fuse): nothing of the handle's may be in flight when its buffers go.
inline void release_handle_buffers(plslam_ctx* ctx, DevBuf& buf, HostBuf& pin)
{
    std::lock_guard<std::mutex> lk(ctx->mu);
    DeviceGuard dg_(ctx->device);
    (void)hipStreamSynchronize(ctx->stream);
    buf.release();
    pin.release();
}

// The download of a handle's device arrays: the ones the caller gave a host pointer for (dst != nullptr) and that hold something,
// copied on s and waited for.  The caller holds the context's lock and has selected its device.
struct DownloadItem { void* dst; const void* src; size_t bytes; };
template <size_t N> int download_items(const DownloadItem (&items)[N], hipStream_t s)
{
    StreamSyncOnError guard(s);
    for (const DownloadItem& it : items)
        if (it.dst && it.bytes) PLSLAM_HIP_CHECK(hipMemcpyAsync(it.dst, it.src, it.bytes, hipMemcpyDeviceToHost, s));
    PLSLAM_HIP_CHECK(hipStreamSynchronize(s));
    guard.dismiss();
    return PLSLAM_OK;
}

// Pointers read from launch tables are GENERIC to the compiler, and a generic access is a FLAT instruction (it counts on
// lgkmcnt as well as vmcnt, and cannot take a scalar base).  Kernels spell the address space out at the point of use:
// g_(p)[i] is a global_load / global_store.  (tests/test_abi.py: no flat_* instruction in any kernel's ISA.)
#if defined(__HIPCC__)
#define PLSLAM_AS1 __attribute__((address_space(1)))
#define g_(p) ((PLSLAM_AS1 __typeof__(*(p))*)(p))          /* keeps the pointee's typedef (alignment attributes included) */
typedef uint32_t gvec2_t __attribute__((ext_vector_type(2)));   // native vectors: HIP's uint2 / uint4 structs cannot be copied
typedef uint32_t gvec4_t __attribute__((ext_vector_type(4)));   // out of / into another address space
template <class T> __device__ __forceinline__ int atomic_add_global(T* p, int v)
{
    return __hip_atomic_fetch_add((PLSLAM_AS1 int*)p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
#endif

// --- composite keys of the Hamming scans and the windowed matcher (the scans' launch interface: match_kernels.hpp) --------
// key = (distance << 23) | trainIdx; 0xFFFFFFFF = "no neighbour"
constexpr uint32_t KEY_IDX_BITS = 23;
constexpr uint32_t KEY_IDX_MASK = (1u << KEY_IDX_BITS) - 1u;
constexpr uint32_t KEY_NONE = 0xFFFFFFFFu;

// --- LBA rows (lba.hip; the gates and the visibility kernels: map2kf_dev.hpp) ------------------
int launch_point_rows(const plslam_cam& K, double th, const double* T, const double* Xw,
                      const double* uv, const int32_t* lm, const int32_t* kf, int32_t nobs,
                      double* Jp, double* Jl, double* r, double* w, hipStream_t s, int32_t n_pose_slots = 0);
int launch_line_rows(const plslam_cam& K, double th, int compat, const double* T, const double* Lw,
                     const double* lobs, const int32_t* lm, const int32_t* kf, int32_t nobs,
                     double* Jp, double* Jl, double* r, double* w, hipStream_t s, int32_t n_pose_slots = 0);

// --- stereo gates (stereo_gates.hip) -------------------------------------------------------------
int launch_stereo_gates(const plslam_stereo_gate_problem* d_gates, const BlockDesc* d_blocks, int nblocks, hipStream_t s);
int check_stereo_gate_problem(const plslam_stereo_gate_problem& q);

// --- representative descriptor per landmark (median_desc.hip) ---------------------------------
// desc: total x 32 u8 (4-byte aligned), off: n_lm+1 CSR offsets (device), med_idx: n_lm, med_desc:
// n_lm x 32 or nullptr.  memset + 2 kernels on s.
int launch_median_desc(const uint8_t* desc, const int32_t* off, int32_t n_lm, int32_t total,
                       int32_t* med_idx, uint8_t* med_desc, hipStream_t s);

// --- K54 from inside the library (loop_closure.hip; the tracker, track.hip) --------------------
// plslam_relpose_robust_gn_batched_dev behind its checks and its lock: K54 on the context's stream, behind what `us` holds on
// entry and in front of what it is given next.  The caller holds ctx->mu and has selected the context's device.
int lc_relpose_batched_unlocked(plslam_ctx* ctx, const plslam_lc_params* params, const double* P, const double* pl_obs,
                                const int32_t* pt_off, const double* sPeP, const double* le_obs, const int32_t* ls_off, int32_t B,
                                plslam_lc_result* results, uint8_t* pt_inlier, uint8_t* ls_inlier, hipStream_t us);

// --- LBD float -> binary line descriptor (lbd.hip) ---------------------------------------------
// lbd: n x 72 f32, codes: n x 32 u8 (both 16-byte aligned)
int launch_lbd_binarise(const float* lbd, int32_t n, uint8_t* codes, hipStream_t s);

}  // namespace plslam
