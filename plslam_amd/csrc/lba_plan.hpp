// lba_plan.hpp -- the LBA plan object as the two translation units that work on it see it: lba_plan.hip (lifetime, iterations,
// state, downloads) and lba_schur.hip (the Schur step on the blocks an iteration left on the device).  Internal.
//
// The plan's buffers are named ONCE: each is carved in one function (lba_plan.hip: carve_*; lba_schur.hip: carve_schur), which
// fills a view of typed pointers with the bytes behind each (Arr, ArrCarver: common.hpp); every launch site, upload and
// download reads the views.
#pragma once

#include "lba_blocks_dev.hpp"
#include "lba_lm_ctl.hpp"

struct plslam_lba_plan;

namespace plslam {

struct LbaStatView {               // `stat`: the observation lists, the observations, the CSR lists -- uploaded once
    Arr<int32_t> pt_lm, pt_slot, pt_kf;
    Arr<double> uv;
    Arr<int32_t> ls_lm, ls_slot, ls_kf;
    Arr<double> lobs;
    Arr<int32_t> pt_ptr, pt_ids, ls_ptr, ls_ids, kf_ptr, kf_ids;
};
struct LbaStateView { Arr<double> T, Xw, Lw; };                          // `dyn` and its page-locked image: the same layout
struct LbaRowsView { Arr<double> pJp, pJl, pr, pw, lJp, lJl, lr, lw; };  // `rows`
struct LbaOutView {                // `out`: g with err right behind it (one copy brings both back), the blocks, the partials
    Arr<double> g, H_pose, H_pt, H_ls, W_pt, W_ls, err, err_part, pose_part;
};

// S and the words behind it, in the Schur buffer on the device and in the page-locked image alike (ONE copy, or none when the
// kernels write the mapped image in place, brings them all to the host): S (n6 x n6, n6 = 6 nkf), b (n6), the diagonal maximum,
// the two counters of singular landmarks (int32 each: one word), the iteration's err
struct SchurTail {
    double *S = nullptr, *b = nullptr, *hmax = nullptr;
    int32_t* sing = nullptr;
    double* err = nullptr;
    static size_t bytes(size_t n6) { return (n6 * n6 + n6 + 3) * 8; }
    SchurTail() = default;
    SchurTail(double* base, size_t n6) : S(base), b(S + n6 * n6), hmax(b + n6), sing(reinterpret_cast<int32_t*>(hmax + 1)), err(hmax + 2) {}
};
struct LbaSchurView {              // `schur`
    Arr<SchurPair> pairs;
    Arr<int32_t> blk_ptr;
    Arr<double> Vp, Vl, tp, tl, spart, bpart;
    SchurTail tail;
    Arr<double> dp, dx, dx_part;   // dx: the points' steps, then the lines'; dx_part: a sum of squares per workgroup of the back-substitution
};
// the page-locked block of the Schur step, used for one thing at a time: the tail | dp with the back-substitution's sums of
// squares behind it | the landmark steps
struct SchurImage {
    SchurTail tail;
    double *dp = nullptr, *dx_part = nullptr, *dx = nullptr;
    SchurImage() = default;
    SchurImage(double* base, size_t n6) : tail(base, n6), dp(base), dx_part(base + n6), dx(base) {}
};

// (lba_plan.hip) the block kernels' arguments from the plan's views
LbaBlockArgs lba_block_args(plslam_lba_plan* P);
// (lba_plan.hip) upload X (one copy), rows + cross blocks + err partials (F1), landmark blocks + keyframe chunk partials (F2), keyframe
// blocks + err (F3): enqueued on the context's stream, nothing downloaded.  Caller holds ctx->mu.
// upload = false: the poses and landmarks already on the device are used (plslam_lba_plan_iterate_resident: a device-side
// solver has updated them in place)
// fused_lambda >= 0 (plslam_lba_plan_iterate_schur; the Schur step's buffers exist): the landmark inverses for that damping are
// written by the blocks' launch, and the last stage (K10) is NOT launched here -- it rides in the Schur partials' launch
// (lba_schur.hip: lba_schur_enqueue(fused)), which the caller enqueues next
// ctl (plslam_lba_plan_optimize_dev): every kernel returns at once when the loop's stop word is set, and the fused form reads the
// damping from the control block (fused_lambda >= 0 then only says "fused")
int lba_plan_enqueue(plslam_lba_plan* P, const double* T_kf_w, const double* Xw, const double* Lw, int compat_flags, bool upload = true,
                     double fused_lambda = -1.0, const LbaLmCtl* ctl = nullptr);
// (lba_schur.hip) the Schur step's launches on the blocks of the last iteration (fused: of the iteration whose last stage rides in
// the partials' launch); no copy, no synchronisation; *par_out = the counter word of singular landmarks this call counts in.
// ctl: behind the stop word, the damping from the control block, S and b left on the device (sc.tail) for the device's solve
int lba_schur_enqueue(plslam_lba_plan* P, double lambda, int* par_out, bool fused = false, const LbaLmCtl* ctl = nullptr);
// (lba_schur.hip) the back-substitution of the dp the device's solve left in sc.dp, applied when the control block says so
int lba_backsub_enqueue_lm(plslam_lba_plan* P, const LbaLmCtl* ctl);
int lba_backsub_wgs(const plslam_lba_plan* P);      // its workgroups: one sum of squares each in sc.dx_part
// (lba_schur.hip) on first use: the pair lists (lba_lists.hpp), the Schur buffers carved and the lists uploaded -- or, for a plan
// whose lists were built on the device (plslam_lba_plan_create_dev), lba_schur_prepare_dev
int lba_schur_prepare(plslam_lba_plan* P);
// (lba_schur.hip) the Schur buffer and its page-locked block for `npairs` pairs (P->nblk, P->schur_chunks set), both counters of
// singular landmarks cleared on the stream; nothing is synchronised
int lba_schur_reserve(plslam_lba_plan* P, size_t npairs);
// (lba_plan.hip) the plan's four buffers and the images of `dyn`, laid out from the plan's counts (n_kfi_cap, max_chunks): the
// sizes; views over whichever buffers exist
struct LbaPlanBytes { size_t stat, dyn, rows, out; };
LbaPlanBytes lba_plan_carve(plslam_lba_plan* P);
// (lba_plan_dev.hip) the pair lists of a device-built plan: enumerated, distributed by block and laid out on the device
int lba_schur_prepare_dev(plslam_lba_plan* P);

}  // namespace plslam

// ---------------------------------------------------------------------------------------------
// LBA plan: the LM loop of levMarquardtOptimizationLBA rebuilds rows + H/g up to max_iters_lba = 15
// times per call (src/mapHandler.cpp:1358-1540 once, :1587-1772 per iteration) while only X (poses,
// landmarks) changes.  The plan uploads the observation lists, the observations and the CSR lists
// once; iterate() uploads X, runs K3/K4 and K7-K10 device-resident and downloads the blocks.
// ---------------------------------------------------------------------------------------------
struct plslam_lba_plan {
    plslam_ctx* ctx = nullptr;
    plslam_cam cam{};
    double th = 0;
    int32_t n_slots = 0, nkf = 0, npt = 0, nls = 0, np = 0, nl = 0;
    plslam::DevBuf stat, dyn, rows, out;   // static lists / X / row arrays / blocks
    plslam::LbaStatView st;
    plslam::LbaStateView x;
    plslam::LbaRowsView rw;
    plslam::LbaOutView o;
    int32_t max_chunks = 0;
    // one iteration = one upload, three launches, one download: the poses and landmarks are packed into a page-locked image
    // of `dyn` (ONE copy instead of three from pageable memory), err sits right behind g (ONE copy back)
    plslam::HostBuf pin_in, pin_out;
    plslam::LbaStateView hx;       // pin_in
    plslam::Arr<double> hg;        // pin_out: g, and err behind it
    double* herr = nullptr;
    size_t dyn_bytes = 0;
    bool state_valid = false;      // T / Xw / Lw have been uploaded at least once (iterate_resident needs them)
    bool blocks_valid = false;     // an iteration has left H / g / W on the device (the Schur step consumes them)
    bool blocks_gba = false;       // ... with the pose x line cross blocks transposed (PLSLAM_LBA_COMPAT_GBA): not what the Schur step reads
    int32_t n_kfi = 0, n_kfi_cap = 0;  // entries of the keyframe list, and the room carved for them (a device-built plan carves
                                       // before it knows: every observation)
    // ---- the Schur step (round 5): pair lists built on first use from these host copies of the observation lists
    plslam::CsrLists csr;
    std::vector<int32_t> h_pt_kf, h_ls_kf;
    // ---- a plan built on the device (plslam_lba_plan_create_dev): no host copy of any list
    bool dev_lists = false;
    bool lm_resident = false;          // Xw / Lw were copied in at creation: plslam_lba_plan_set_poses completes the state
    plslam::DevBuf aux, aux_schur;     // the builders' scratch; aux keeps the pair counts for the Schur lists' first use
    plslam::HostBuf pin_cnt;           // the counts the builders bring back
    int32_t* d_pair_cnt = nullptr;     // (aux) pairs each position of the landmark lists starts: points' positions, then lines'
    int64_t n_pairs_enum = 0;          // their sum
    plslam::DevBuf schur;
    plslam::LbaSchurView sc;
    plslam::HostBuf schur_pin;
    plslam::SchurImage simg;       // schur_pin as the host addresses it
    plslam::SchurImage simg_dev;   // ... and as the device does (mapped page-locked memory)
    bool schur_mapped = false;     // ... if it can: the kernels write S, b in place.  Otherwise they write sc.tail and a copy follows
    bool schur_ready = false, schur_done = false;
    int schur_parity = 0;              // which of the two counters of singular landmarks the next plslam_lba_plan_schur counts in
    int32_t nblk = 0, schur_chunks = 0;
    // ---- plslam_lba_plan_optimize_dev (lba_lm_dev.hip): the loop's control block, x_kf, the solve's scratch | their images
    plslam::DevBuf lm;
    plslam::HostBuf lm_pin;
    int32_t lm_trace_cap = 0;          // trace records the two blocks have room for (0: not laid out yet)

    size_t n_unknowns() const { return 6 * (size_t)nkf + 3 * (size_t)npt + 6 * (size_t)nls; }
    void release()
    {
        stat.release(); dyn.release(); rows.release(); out.release(); pin_in.release(); pin_out.release();
        schur.release(); schur_pin.release(); aux.release(); aux_schur.release(); pin_cnt.release();
        lm.release(); lm_pin.release();
    }
};
