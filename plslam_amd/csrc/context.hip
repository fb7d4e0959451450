// context.hip -- the context of libplslam_hip.so (see include/plslam_hip.h): the last-error text, the grow-only device and
// pinned buffers, plslam_ctx_create / destroy and the option table.  The one translation unit that
// sees PLSLAM_BUILD_LEGACY_SCANS: what the build carries is answered here (option "legacy_scans", launch_scan_mfma_form).
#include <stdarg.h>
#include <string.h>

#include <new>

#include "common.hpp"
#include "match_grid.hpp"   // g_grid_dense
#include "match_kernels.hpp"   // launch_scan_mfma_form and the scans it picks among
#include "match_plan.hpp"   // match_plan_release: the context owns two plans

namespace plslam {

static thread_local char g_err[512] = "";

void set_last_error(const char* fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

int DevBuf::reserve(size_t bytes)
{
    if (bytes <= cap) return PLSLAM_OK;
    if (p) {
        (void)hipFree(p);
        p = nullptr;
        cap = 0;
    }
    size_t want = bytes + (bytes >> 2);  // grow by 25 % to damp re-allocation
    want = align256(want);
    PLSLAM_HIP_CHECK(hipMalloc(&p, want));
    cap = want;
    return PLSLAM_OK;
}

void DevBuf::release()
{
    if (p) (void)hipFree(p);
    p = nullptr;
    cap = 0;
}

int HostBuf::reserve(size_t bytes)
{
    if (bytes <= cap) return PLSLAM_OK;
    if (p) {
        (void)hipHostFree(p);
        p = nullptr;
        dev = nullptr;
        cap = 0;
    }
    size_t want = bytes + (bytes >> 2);
    want = (want + 4095) & ~size_t(4095);
    PLSLAM_HIP_CHECK(hipHostMalloc(&p, want, hipHostMallocDefault));
    cap = want;
    dev = mapped_device_pointer(p);                // (asked once: hipPointerGetAttributes per call was 1-2 us of a 40 us call)
    return PLSLAM_OK;
}

void HostBuf::release()
{
    if (p) (void)hipHostFree(p);
    p = nullptr;
    dev = nullptr;
    cap = 0;
}

}  // namespace plslam

using namespace plslam;

// the matrix-core scan of `form`: the generations a legacy build carries beside K1i and K1f
int plslam::launch_scan_mfma_form(int form, const SymDesc* d_sym, const BlockDesc* d_blocks, int nblocks, int32_t* d_zero,
                                  int nzero, bool multi_window, bool directed, hipStream_t s, bool fused)
{
#if PLSLAM_BUILD_LEGACY_SCANS
    if (form == 3 && directed && !fused) return launch_scan_dir_mfma(d_sym, d_blocks, nblocks, d_zero, nzero, s);
    if (form == 4 && !fused) return launch_scan_sym_mfma_h(d_sym, d_blocks, nblocks, d_zero, nzero, directed, s);
#endif
    if (mfma_form_is_h(form) && !fused) return launch_scan_sym_mfma_i(d_sym, d_blocks, nblocks, d_zero, nzero, directed, s);
#if PLSLAM_BUILD_LEGACY_SCANS
    if (form == 1) return launch_scan_sym_mfma(d_sym, d_blocks, nblocks, d_zero, nzero, multi_window, directed, s);
#endif
    return launch_scan_sym_mfma_g(d_sym, d_blocks, nblocks, d_zero, nzero, multi_window, directed, fused, s);
}

extern "C" {

const char* plslam_strerror(int code)
{
    switch (code) {
        case PLSLAM_OK: return "ok";
        case PLSLAM_EINVAL: return "invalid argument";
        case PLSLAM_ENODEV: return "no usable gfx950 HIP device";
        case PLSLAM_EHIP: return "HIP runtime error";
        case PLSLAM_ENOMEM: return "out of memory";
        case PLSLAM_ERANGE: return "size beyond documented limit";
        case PLSLAM_ENOTSUP: return "optional component unavailable";
        default: return "unknown error";
    }
}

const char* plslam_last_error(void) { return g_err; }
int plslam_abi_version(void) { return PLSLAM_ABI_VERSION; }

int plslam_ctx_create(int device_ordinal, plslam_ctx** out)
{
    PLSLAM_REQUIRE(out != nullptr, PLSLAM_EINVAL);
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
        set_last_error("no HIP device visible (this library has no CPU fallback)");
        return PLSLAM_ENODEV;
    }
    PLSLAM_REQUIRE(device_ordinal >= 0 && device_ordinal < ndev, PLSLAM_ENODEV);
    plslam_ctx* c = new (std::nothrow) plslam_ctx();
    PLSLAM_REQUIRE(c != nullptr, PLSLAM_ENOMEM);
    c->device = device_ordinal;
    DeviceGuard g(device_ordinal);
    if (hipGetDeviceProperties(&c->prop, device_ordinal) != hipSuccess) {
        delete c;
        set_last_error("hipGetDeviceProperties failed");
        return PLSLAM_ENODEV;
    }
    if (strncmp(c->prop.gcnArchName, "gfx950", 6) != 0) {
        set_last_error("device %d is %s; this library carries gfx950 code only", device_ordinal,
                       c->prop.gcnArchName);
        delete c;
        return PLSLAM_ENODEV;
    }
    if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) {
        delete c;
        set_last_error("hipStreamCreate failed");
        return PLSLAM_EHIP;
    }
    *out = c;
    return PLSLAM_OK;
}

void plslam_ctx_destroy(plslam_ctx* ctx)
{
    if (!ctx) return;
    DeviceGuard g(ctx->device);
    (void)hipStreamSynchronize(ctx->stream);
    ctx->in_a.release(); ctx->in_b.release(); ctx->out_a.release(); ctx->out_b.release();
    ctx->misc_a.release(); ctx->misc_b.release(); ctx->misc_c.release();
    ctx->pin_in.release();
    ctx->pin_out.release();
    ctx->pin_misc.release();
    ctx->lbd_ring.release();
    match_plan_release(ctx->host_plan);
    match_plan_release(ctx->lc_plan);
    ctx->lc_in.release(); ctx->lc_out.release(); ctx->lc_tab.release(); ctx->lc_args.release();
    ctx->pgo_scratch.release();
    ctx->lists_scratch.release();
    ctx->lc_image_pin.release();
    for (hipEvent_t& e : ctx->lc_ev)
        if (e) (void)hipEventDestroy(e);
    (void)hipStreamDestroy(ctx->stream);
    delete ctx;
}

// every option of plslam_ctx_set_option / plslam_ctx_get_option (meanings: plslam_hip.h): a field of the context, or a
// process-wide variable; lo > hi: read-only
namespace {
int g_legacy_scans = PLSLAM_BUILD_LEGACY_SCANS;
struct OptionDesc { const char* name; int plslam_ctx::*member; int* global; int lo, hi; };
const OptionDesc kOptions[] = {
    {"scan_variant", &plslam_ctx::scan_variant, nullptr, PLSLAM_SCAN_AUTO, PLSLAM_SCAN_MFMA},
    {"scan_block", &plslam_ctx::scan_block, nullptr, 0, 1024},                // (0, 256, 512 or 1024)
    {"sym_rows", &plslam_ctx::sym_rows, nullptr, 0, 4},                       // (0, 1 or 4)
    {"group_cap", &plslam_ctx::group_cap, nullptr, 0, 64},
    {"mfma_form", &plslam_ctx::mfma_form, nullptr, 0, 5},                     // (a form the build lacks: PLSLAM_ENOTSUP)
    {"legacy_scans", nullptr, &g_legacy_scans, 0, -1},                        // a fact of the build
    {"fuse", &plslam_ctx::fuse, nullptr, 0, 2},
    {"post_fuse", &plslam_ctx::post_fuse, nullptr, 0, 2},
    {"exact_second", &plslam_ctx::exact_second, nullptr, 0, 1},
    {"col_split", &plslam_ctx::col_split, nullptr, 0, 2},
    {"graph", &plslam_ctx::graph, nullptr, 0, 2},
    {"grid_dense", nullptr, &plslam::g_grid_dense, 0, 1},                     // the lone small matchGrid problem on one dense workgroup
    {"zero_copy_kb", &plslam_ctx::zero_copy_kb, nullptr, -(1 << 20), 1 << 20},
    {"post_xcd", &plslam_ctx::post_xcd, nullptr, 0, 2},
    {"split_post", &plslam_ctx::split_post, nullptr, 0, 1},
    {"split_target", &plslam_ctx::split_target, nullptr, 0, 64},
    {"split_min_tiles", &plslam_ctx::split_min_tiles, nullptr, 0, 64},
    {"post_workgroups", &plslam_ctx::post_workgroups, nullptr, 0, INT32_MAX},
    {"lba_loop_peek", &plslam_ctx::lba_loop_peek, nullptr, 0, 1},
    {"pgo_solver", &plslam_ctx::pgo_solver, nullptr, 0, 1},                   // measurement tools only: 1 = the pose graph on the dense L D L^T
};
const OptionDesc* find_option(const char* key, bool to_write)
{
    for (const OptionDesc& o : kOptions)
        if (!strcmp(key, o.name) && (!to_write || o.lo <= o.hi)) return &o;
    set_last_error("unknown option '%s'", key);
    return nullptr;
}
}  // namespace

int plslam_ctx_set_option(plslam_ctx* ctx, const char* key, int value)
{
    PLSLAM_REQUIRE(ctx && key, PLSLAM_EINVAL);
    const OptionDesc* o = find_option(key, true);
    if (!o) return PLSLAM_EINVAL;
    PLSLAM_REQUIRE(value >= o->lo && value <= o->hi, PLSLAM_EINVAL);
    if (o->member == &plslam_ctx::scan_block) PLSLAM_REQUIRE(value == 0 || value == 256 || value == 512 || value == 1024, PLSLAM_EINVAL);
    if (o->member == &plslam_ctx::sym_rows) PLSLAM_REQUIRE(value == 0 || value == 1 || value == 4, PLSLAM_EINVAL);
    if (o->member == &plslam_ctx::mfma_form && !mfma_form_built(value)) {
        set_last_error("mfma_form 1 / 3 / 4 (K1e, K1g, K1h: earlier generations of the matrix-core scan) are not in this build: "
                       "PLSLAM_BUILD_LEGACY_SCANS=1 python -m plslam_amd.build");
        return PLSLAM_ENOTSUP;
    }
    (o->member ? ctx->*(o->member) : *o->global) = value;
    return PLSLAM_OK;
}

int plslam_ctx_get_option(plslam_ctx* ctx, const char* key, int* value)
{
    PLSLAM_REQUIRE(ctx && key && value, PLSLAM_EINVAL);
    const OptionDesc* o = find_option(key, false);
    if (!o) return PLSLAM_EINVAL;
    *value = o->member ? ctx->*(o->member) : *o->global;
    return PLSLAM_OK;
}

int plslam_ctx_device_info(plslam_ctx* ctx, int32_t* cu_count, int32_t* clock_khz,
                           int32_t* lds_bytes, char* name, int32_t name_len)
{
    PLSLAM_REQUIRE(ctx != nullptr, PLSLAM_EINVAL);
    if (cu_count) *cu_count = ctx->prop.multiProcessorCount;
    if (clock_khz) *clock_khz = ctx->prop.clockRate;
    if (lds_bytes) *lds_bytes = (int32_t)ctx->prop.sharedMemPerBlock;
    if (name && name_len > 0) {
        snprintf(name, (size_t)name_len, "%s (%s)", ctx->prop.name, ctx->prop.gcnArchName);
    }
    return PLSLAM_OK;
}

}  // extern "C"
