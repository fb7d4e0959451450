// match_grid_api.hip -- the host side of the windowed matcher (K14, StVO::matchGrid): the check of a problem and its descriptor,
// the launch of ONE problem along the path grid_route() picks (match_grid_layout.hpp), the plan of a batch of problems, and the
// C ABI (include/plslam_hip.h) -- plslam_match_grid stages one pinned image here.  The kernels and their launchers are in
// match_grid.hip, match_grid_listers.hip and match_grid_dense.hip.
#include <cstring>
#include <new>

#include "match_grid.hpp"

using namespace plslam;

struct plslam_grid_plan {
    plslam_ctx* ctx = nullptr;
    int32_t nprob = 0;
    int32_t n_mode[4] = {0, 0, 0, 0};  // the table holds the problems of launch group 3 first, then 2, 1, 0
    size_t lds_bytes[4] = {0, 0, 0, 0};   // largest LDS request of a problem of each group
    DevBuf table, scratch, status;
};

static size_t grid_prob_scratch(const plslam_grid_problem& q)
{
    return (grid_scratch_words(q.n1, q.n2, (int64_t)q.grid_cols * q.grid_rows, q.pair_capacity) + 63) & ~size_t(63);
}

// device_rows: d1 / d2 are the pointers the kernels will read (16-byte vector loads); host rows are staged into aligned
// device memory first and may sit anywhere
static int grid_check_problem(const plslam_grid_problem& q, bool device_rows = true)
{
    PLSLAM_REQUIRE(q.n1 >= 0 && q.n2 >= 0 && q.n_centres >= 1 && q.grid_cols >= 1 && q.grid_rows >= 1,
                   PLSLAM_EINVAL);
    PLSLAM_REQUIRE((int64_t)q.grid_cols * q.grid_rows < (int64_t(1) << 31) - 1, PLSLAM_ERANGE);
    PLSLAM_REQUIRE(q.n1 < PLSLAM_MAX_GRID_ROWS && q.n2 <= PLSLAM_MAX_TRAIN_ROWS, PLSLAM_ERANGE);
    PLSLAM_REQUIRE(q.window[0] >= 0 && q.window[1] >= 0 && q.window[2] >= 0 && q.window[3] >= 0,
                   PLSLAM_EINVAL);
    PLSLAM_REQUIRE(q.pair_capacity >= 0 && q.n_items >= 0, PLSLAM_EINVAL);
    PLSLAM_REQUIRE(q.cell_start != nullptr && (q.n_items == 0 || q.cell_items != nullptr), PLSLAM_EINVAL);
    PLSLAM_REQUIRE(q.n1 == 0 || (q.d1 && q.centres1 && q.matches_12), PLSLAM_EINVAL);
    PLSLAM_REQUIRE(q.n2 == 0 || q.d2, PLSLAM_EINVAL);
    PLSLAM_REQUIRE(!device_rows || (((uintptr_t)q.d1 & 15) == 0 && ((uintptr_t)q.d2 & 15) == 0), PLSLAM_EINVAL);
    PLSLAM_REQUIRE((q.dir1 == nullptr) == (q.dir2 == nullptr) || q.n1 == 0 || q.n2 == 0, PLSLAM_EINVAL);
    return PLSLAM_OK;
}

static void grid_fill_desc(const plslam_grid_problem& q, uint32_t* scratch, int32_t* status, GridDesc* d)
{
    d->d1 = q.d1; d->d2 = q.d2; d->centres = q.centres1;
    d->cell_start = q.cell_start; d->cell_items = q.cell_items;
    d->dir1 = q.dir1; d->dir2 = q.dir2;
    d->matches_12 = q.matches_12; d->n_matches = q.n_matches;
    d->scratch = scratch; d->status = status;
    d->sim_th = q.sim_th; d->nnr = q.nnr;
    d->n1 = q.n1; d->n2 = q.n2; d->n_centres = q.n_centres; d->cols = q.grid_cols; d->rows = q.grid_rows;
    d->mutual = q.mutual ? 1 : 0;
    for (int k = 0; k < 4; ++k) d->w[k] = q.window[k];
    d->pair_cap = q.pair_capacity;
    d->n_items = q.n_items;
}


namespace plslam {

int g_grid_dense = 1;               // ctx option "grid_dense": 0 = the small lone problem takes the general kernels as before
bool grid_dense_ok(int32_t n1, int32_t n2, int64_t ncell, int32_t n_items, bool dirs, int32_t n_centres)
{
    return g_grid_dense && grid_dense_fits(n1, n2, ncell, n_items, dirs, n_centres);
}

// aux = grid_aux_words(n2) device words the two launches of a large lone problem share -- [0] the candidate list's length --
// holding zero when the launches reach them: callers upload an image anyway and put them there (grid_aux_fill).
size_t grid_aux_words(int32_t) { return 4; }
void grid_aux_fill(void* host_image, int32_t n2) { memset(host_image, 0, grid_aux_words(n2) * 4); }

// One problem with DEVICE pointers, in two steps so that the descriptor can travel inside a larger upload of the caller:
// grid_prepare_one checks the problem and writes its GridDesc to h_desc_slot (host); grid_launch_single launches it once
// that descriptor is at d_desc on the device.
int grid_prepare_one(const plslam_grid_problem& q, uint32_t* scratch, int32_t* status, GridDesc* h_desc_slot)
{
    int rc;
    if ((rc = grid_check_problem(q))) return rc;
    grid_fill_desc(q, scratch, status, h_desc_slot);
    return PLSLAM_OK;
}

// ONE problem on `s`, along the path grid_route() picks.  aux: see above; without it (nullptr) the problem is one launch.
// n1_upper_bound: q.n1 is an upper bound, the row count is the device descriptor's, patched by the caller's kernels.
// h_desc: the host's copy of the descriptor (the kernels of a lone problem take it by value), or nullptr.
int grid_launch_single(const plslam_grid_problem& q, const GridDesc* d_desc, hipStream_t s, uint32_t* aux, bool n1_upper_bound,
                       const GridDesc* h_desc)
{
    GridShape sh{};
    sh.n1 = q.n1; sh.n2 = q.n2; sh.n_centres = q.n_centres; sh.cols = q.grid_cols; sh.rows = q.grid_rows;
    sh.n_items = q.n_items; sh.pair_capacity = q.pair_capacity;
    for (int k = 0; k < 4; ++k) sh.window[k] = q.window[k];
    sh.mutual = q.mutual;
    sh.dirs = q.dir1 != nullptr && q.dir2 != nullptr;
    const GridRoute r = grid_route(sh, g_grid_dense != 0, aux != nullptr, h_desc != nullptr, n1_upper_bound);
    const int64_t ncell = (int64_t)q.grid_cols * q.grid_rows;
    const int32_t* n1_dev = n1_upper_bound ? &d_desc->n1 : nullptr;
    int rc;
    switch (r.path) {
    case GRID_PATH_DENSE:
        return launch_match_grid_dense(*h_desc, s);
    case GRID_PATH_RECORDS:
        if ((rc = launch_grid_records(*h_desc, aux, n1_dev, r.workgroups, s))) return rc;
        return launch_match_grid_listed(d_desc, grid_group_lds_bytes(2, q.n1, q.n2, ncell, q.n_items, sh.dirs), s, aux, REC_SLOT, h_desc, n1_dev);
    case GRID_PATH_CANDIDATES:
        if ((rc = launch_grid_candidates(d_desc, aux, r.split, r.workgroups, s))) return rc;
        return launch_match_grid_listed(d_desc, grid_group_lds_bytes(2, q.n1, q.n2, ncell, q.n_items, sh.dirs), s, aux, 0, nullptr, nullptr);
    case GRID_PATH_SINGLE:
        break;
    }
    int32_t n_mode[4] = {0, 0, 0, 0};
    size_t lds_bytes[4] = {0, 0, 0, 0};
    n_mode[r.group] = 1;
    lds_bytes[r.group] = grid_group_lds_bytes(r.group, q.n1, q.n2, ncell, q.n_items, sh.dirs);
    return launch_match_grid(d_desc, n_mode, lds_bytes, s);
}

}  // namespace plslam

extern "C" {

int plslam_grid_plan_create(plslam_ctx* ctx, const plslam_grid_problem* probs, int32_t nprob,
                            plslam_grid_plan** out)
{
    PLSLAM_REQUIRE(ctx && out && nprob >= 0 && (nprob == 0 || probs), PLSLAM_EINVAL);
    *out = nullptr;
    int rc;
    size_t words = 0;
    for (int32_t b = 0; b < nprob; ++b) {
        if ((rc = grid_check_problem(probs[b]))) return rc;
        words += grid_prob_scratch(probs[b]);
    }
    DeviceGuard g(ctx->device);
    plslam_grid_plan* P = new (std::nothrow) plslam_grid_plan();
    PLSLAM_REQUIRE(P != nullptr, PLSLAM_ENOMEM);
    P->ctx = ctx;
    P->nprob = nprob;
    auto fail = [&](int code) { plslam_grid_plan_destroy(P); return code; };
    if ((rc = P->table.reserve(sizeof(GridDesc) * (size_t)(nprob ? nprob : 1)))) return fail(rc);
    if ((rc = P->scratch.reserve(words * 4 + 256))) return fail(rc);
    if ((rc = P->status.reserve(256))) return fail(rc);
    std::vector<GridDesc> tab((size_t)nprob);
    size_t off = 0;
    int32_t slot = 0;
    for (int mode = 3; mode >= 0; --mode)
        for (int32_t b = 0; b < nprob; ++b) {
            const int64_t ncell = (int64_t)probs[b].grid_cols * probs[b].grid_rows;
            const bool dirs = probs[b].dir1 != nullptr && probs[b].dir2 != nullptr;
            if (grid_group(probs[b].n1, probs[b].n2, ncell, probs[b].n_items, dirs) != mode) continue;
            const size_t lb = grid_group_lds_bytes(mode, probs[b].n1, probs[b].n2, ncell, probs[b].n_items, dirs);
            if (lb > P->lds_bytes[mode]) P->lds_bytes[mode] = lb;
            ++P->n_mode[mode];
            grid_fill_desc(probs[b], P->scratch.as<uint32_t>() + off, P->status.as<int32_t>(), &tab[slot++]);
            off += grid_prob_scratch(probs[b]);
        }
    if (hipMemset(P->status.p, 0, 256) != hipSuccess ||
        (nprob && hipMemcpy(P->table.p, tab.data(), sizeof(GridDesc) * (size_t)nprob, hipMemcpyHostToDevice) !=
                      hipSuccess)) {
        set_last_error("%s:%d: upload of the grid problem table failed", __FILE__, __LINE__);
        return fail(PLSLAM_EHIP);
    }
    *out = P;
    return PLSLAM_OK;
}

int plslam_grid_plan_run(plslam_grid_plan* plan, void* stream)
{
    PLSLAM_REQUIRE(plan != nullptr, PLSLAM_EINVAL);
    DeviceGuard g(plan->ctx->device);
    return launch_match_grid(plan->table.as<GridDesc>(), plan->n_mode, plan->lds_bytes,
                             stream ? static_cast<hipStream_t>(stream) : plan->ctx->stream);
}

int plslam_grid_plan_overflows(plslam_grid_plan* plan, void* stream, int32_t* n_overflows)
{
    PLSLAM_REQUIRE(plan && n_overflows, PLSLAM_EINVAL);
    DeviceGuard g(plan->ctx->device);
    hipStream_t s = stream ? static_cast<hipStream_t>(stream) : plan->ctx->stream;
    PLSLAM_HIP_CHECK(hipMemcpyAsync(n_overflows, plan->status.p, 4, hipMemcpyDeviceToHost, s));
    PLSLAM_HIP_CHECK(hipMemsetAsync(plan->status.p, 0, 4, s));
    PLSLAM_HIP_CHECK(hipStreamSynchronize(s));
    return PLSLAM_OK;
}

void plslam_grid_plan_destroy(plslam_grid_plan* plan)
{
    if (!plan) return;
    DeviceGuard g(plan->ctx->device);
    plan->table.release();
    plan->scratch.release();
    plan->status.release();
    delete plan;
}

int plslam_match_grid(plslam_ctx* ctx, const int32_t* centres1, int32_t n_centres, const uint8_t* d1,
                      int32_t n1, const int32_t* cell_start, const int32_t* cell_items, int32_t grid_cols,
                      int32_t grid_rows, const uint8_t* d2, int32_t n2, const double* dir1,
                      const double* dir2, double sim_th, const int32_t window[4], double nnr, int mutual,
                      int32_t* matches_12, int32_t* n_matches)
{
    PLSLAM_REQUIRE(ctx && window, PLSLAM_EINVAL);
    PLSLAM_REQUIRE(n1 >= 0, PLSLAM_EINVAL);
    if (n_matches) *n_matches = 0;
    if (n1 == 0) return PLSLAM_OK;
    plslam_grid_problem q{};
    q.d1 = d1; q.d2 = d2; q.centres1 = centres1; q.cell_start = cell_start; q.cell_items = cell_items;
    q.dir1 = dir1; q.dir2 = dir2;
    q.n1 = n1; q.n2 = n2; q.n_centres = n_centres; q.grid_cols = grid_cols; q.grid_rows = grid_rows;
    q.n_items = 0;   // validated and set below
    for (int k = 0; k < 4; ++k) q.window[k] = window[k];
    q.sim_th = sim_th; q.nnr = nnr; q.mutual = mutual;
    q.matches_12 = matches_12;
    int rc;
    if ((rc = grid_check_problem(q, false))) return rc;
    // the grid is host data here: validate the offsets and count the (row, candidate) pairs exactly.  The ENTRIES are
    // not validated: an entry outside [0, n2) is skipped by the kernel before any read, as upstream's loop skips it
    // (`if (i2 < 0 || i2 >= desc2.rows) continue;`) -- tests/test_gpu_match_grid.py::test_empty_and_out_of_range_inputs
    const int64_t ncell = (int64_t)grid_cols * grid_rows;
    PLSLAM_REQUIRE(cell_start[0] == 0, PLSLAM_EINVAL);
    for (int64_t c = 0; c < ncell; ++c) PLSLAM_REQUIRE(cell_start[c + 1] >= cell_start[c], PLSLAM_EINVAL);
    const int32_t n_items = cell_start[ncell];
    PLSLAM_REQUIRE(n_items == 0 || cell_items, PLSLAM_EINVAL);
    q.n_items = n_items;
    // capacity of the candidate store.  A bound from the grid alone (fullest cell x cells of a window, at most every item,
    // per window centre; rows in blocks of 1024) costs one pass over cell_start; only when that bound is large is the
    // exact figure worth a walk over every row's window.
    int64_t pairs = grid_store_capacity_bound(n1, n_centres, cell_start, grid_cols, grid_rows, window, mutual);
    if (pairs > (int64_t(1) << 21))
        pairs = grid_store_capacity_host(centres1, n1, n_centres, cell_start, grid_cols, grid_rows, window, mutual);
    PLSLAM_REQUIRE(pairs < (int64_t(1) << 31) - 1, PLSLAM_ERANGE);
    q.pair_capacity = (int32_t)pairs;

    std::lock_guard<std::mutex> lk(ctx->mu);
    DeviceGuard g(ctx->device);
    // ONE pinned staging block -> one H2D copy: [GridDesc | centres | cell_start | cell_items | d1 | d2 | dir1 | dir2]
    Carver ci;
    const bool dirs = dir1 && dir2 && n2 > 0;
    const size_t oT = ci.take(sizeof(GridDesc)), oX = ci.take(grid_aux_words(n2) * 4), oC = ci.take((size_t)n1 * n_centres * 8),
                 oS = ci.take((size_t)(ncell + 1) * 4), oI = ci.take((size_t)n_items * 4),
                 oA = ci.take((size_t)n1 * 32), oB = ci.take((size_t)n2 * 32),
                 oD1 = ci.take(dirs ? (size_t)n1 * 16 : 0), oD2 = ci.take(dirs ? (size_t)n2 * 16 : 0);
    Carver co;
    const size_t oM = co.take((size_t)n1 * 4), oN = co.take(8);   // n_matches, status
    if ((rc = ctx->pin_in.reserve(ci.off))) return rc;
    if ((rc = ctx->in_a.reserve(ci.off))) return rc;
    if ((rc = ctx->pin_out.reserve(co.off))) return rc;
    if ((rc = ctx->out_a.reserve(co.off))) return rc;
    if ((rc = ctx->misc_a.reserve(grid_scratch_words(n1, n2, ncell, q.pair_capacity) * 4 + 256))) return rc;
    char* h = ctx->pin_in.as<char>();
    char* d = ctx->in_a.as<char>();
    char* dout = ctx->out_a.as<char>();
    // (option "zero_copy_kb": a small upload image is read by the kernels where it lies in page-locked host memory -- the copy
    // command in front of them, with its completion signal, is the larger part of such a call's device-side time)
    // Taken where it was measured to pay (profiles/r6_r_grid_latency_dense_zero_copy.txt): a problem the dense one-workgroup kernel
    // takes -- it reads every input word ONCE, into LDS: 200 x 200 lines 57.3 -> 50.9 us per call; the general kernels walk the
    // cells and the descriptors again and again (neutral to 64 kB, slower beyond) and keep the copy unless the option is negative
    // (-kb: every problem whose image fits |kb|).
    bool zero_copy = false;
    const bool dense = grid_dense_ok(n1, n2, ncell, n_items, dirs, n_centres);
    const size_t zc_limit = (size_t)(ctx->zero_copy_kb < 0 ? -ctx->zero_copy_kb : ctx->zero_copy_kb) * 1024;
    if (zc_limit > 0 && ci.off <= zc_limit && (dense || ctx->zero_copy_kb < 0))
        if (char* m = static_cast<char*>(ctx->pin_in.dev)) { d = m; zero_copy = true; }
    memcpy(h + oC, centres1, (size_t)n1 * n_centres * 8);
    memcpy(h + oS, cell_start, (size_t)(ncell + 1) * 4);
    if (n_items) memcpy(h + oI, cell_items, (size_t)n_items * 4);
    memcpy(h + oA, d1, (size_t)n1 * 32);
    if (n2) memcpy(h + oB, d2, (size_t)n2 * 32);
    if (dirs) {
        memcpy(h + oD1, dir1, (size_t)n1 * 16);
        memcpy(h + oD2, dir2, (size_t)n2 * 16);
    }
    plslam_grid_problem dq = q;
    dq.centres1 = (const int32_t*)(d + oC);
    dq.cell_start = (const int32_t*)(d + oS);
    dq.cell_items = (const int32_t*)(d + oI);
    dq.d1 = (const uint8_t*)(d + oA);
    dq.d2 = (const uint8_t*)(d + oB);
    dq.dir1 = dirs ? (const double*)(d + oD1) : nullptr;
    dq.dir2 = dirs ? (const double*)(d + oD2) : nullptr;
    // results: the kernel writes the table, the count and the status word straight into the page-locked block when the
    // device can address it (one copy-engine command less on the call's critical path)
    char* hout_dev = static_cast<char*>(ctx->pin_out.dev);
    int32_t* hres = (int32_t*)(ctx->pin_out.as<char>() + oN);
    if (hout_dev) {
        hres[0] = hres[1] = 0;
        dout = hout_dev;
    }
    dq.matches_12 = (int32_t*)(dout + oM);
    dq.n_matches = (int32_t*)(dout + oN);
    if ((rc = grid_check_problem(dq))) return rc;                 // what the kernel reads: the staged, aligned rows
    // (no status word over PCIe -- it is bumped with an atomic; an overflow also shows as a count of -1)
    grid_fill_desc(dq, ctx->misc_a.as<uint32_t>(), hout_dev ? nullptr : (int32_t*)(dout + oN) + 1, (GridDesc*)(h + oT));
    grid_aux_fill(h + oX, n2);
    hipStream_t s = ctx->stream;
    StreamSyncOnError sg(s);
    if (!zero_copy) PLSLAM_HIP_CHECK(hipMemcpyAsync(d, h, ci.off, hipMemcpyHostToDevice, s));
    if (!hout_dev) PLSLAM_HIP_CHECK(hipMemsetAsync(dout + oN, 0, 8, s));
    if ((rc = grid_launch_single(dq, (const GridDesc*)(d + oT), s, (uint32_t*)(d + oX), false, (const GridDesc*)(h + oT)))) return rc;
    if (!hout_dev) PLSLAM_HIP_CHECK(hipMemcpyAsync(ctx->pin_out.p, dout, co.off, hipMemcpyDeviceToHost, s));
    PLSLAM_HIP_CHECK(hipStreamSynchronize(s));
    const int32_t* res = (const int32_t*)(ctx->pin_out.as<char>() + oN);
    if (res[1] != 0 || res[0] < 0) {   // cannot happen: the capacity above is an upper bound
        set_last_error("%s:%d: matchGrid candidate store overflow (%d slots provided)", __FILE__, __LINE__, (int)pairs);
        return PLSLAM_ERANGE;
    }
    memcpy(matches_12, ctx->pin_out.as<char>() + oM, (size_t)n1 * 4);
    if (n_matches) *n_matches = res[0];
    return PLSLAM_OK;
}

int64_t plslam_grid_pair_capacity(const int32_t* centres1, int32_t n1, int32_t n_centres, const int32_t* cell_start,
                                  int32_t grid_cols, int32_t grid_rows, const int32_t window[4], int mutual)
{
    if (!centres1 || !cell_start || !window || n1 < 0 || n_centres < 1 || grid_cols < 1 || grid_rows < 1) return -1;
    return plslam::grid_store_capacity_host(centres1, n1, n_centres, cell_start, grid_cols, grid_rows, window, mutual);
}

int64_t plslam_grid_pair_capacity_bound(int32_t n1, int32_t n_centres, const int32_t* cell_start, int32_t grid_cols,
                                        int32_t grid_rows, const int32_t window[4], int mutual)
{
    if (!cell_start || !window || n1 < 0 || n_centres < 1 || grid_cols < 1 || grid_rows < 1) return -1;
    return plslam::grid_store_capacity_bound(n1, n_centres, cell_start, grid_cols, grid_rows, window, mutual);
}

}  // extern "C"
