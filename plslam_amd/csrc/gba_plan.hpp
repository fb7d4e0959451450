// gba_plan.hpp -- the GBA plan object as the translation units that work on it see it: gba.hip (the host-built plan, the LM loop,
// the solve kernels), gba_plan_dev.hip (the plan built on the device from device columns, the lists' download) and local_map.hip
// (the write-back of the plan's resident landmarks into the map image).  Internal.
//
// The plan's buffers are named ONCE: each is carved in one function (gba.hip: gba_carve_stat, gba_carve_pairs, gba_carve_work),
// which fills a view of typed pointers with the bytes behind each; every launch site, upload and download reads the views.
#pragma once

#include <vector>

#include "common.hpp"
#include "gba_lists.hpp"

struct plslam_gba_plan;

namespace plslam {

// the host lists hold pairs of int32 (gba_lists.hpp has no HIP type); K29 reads the same bytes as int2
static_assert(sizeof(GbaPair) == sizeof(int2) && alignof(GbaPair) <= alignof(int2), "GbaPair is uploaded as int2");

struct GbaStats {               // what crosses to the host per solve
    double dx_sumsq;
    int32_t n_singular, n_bad_pivots;
};

struct GbaStatView {               // `stat` and `pairbuf`: the lists of gba_lists.hpp -- uploaded, or built on the device, once
    Arr<int32_t> plm, pkf, llm, lkf;                  // per observation: landmark, optimised keyframe
    Arr<int32_t> kpp, kpo, klp, klo;                  // keyframe -> observations (points, lines)
    Arr<int32_t> lpp, lpo, llp, llo;                  // landmark -> observations by optimised keyframes (points, lines)
    Arr<GbaBlock> blk;                                // (pairbuf from here)
    Arr<GbaChunk> chk;
    Arr<int2> pair;
};
struct GbaWorkView {               // `work`: what a solve computes
    Arr<double> Vp, tp, Vl, tl;                       // landmark inverses and Vj'^-1 gj (points, lines)
    Arr<int32_t> sing, sing_pt, sing_ls;              // singular flags: sing = the points' directly followed by the lines'
    Arr<double> Yp, Yl, part;                         // Y_o; the chunk sums of K29
    Arr<double> P, w, z, dp;                          // the L D L^T's panel, b, z and the pose steps
    Arr<int32_t> bad;                                 // bad pivots per tile
    Arr<double> ss_part;                              // partials of ||DX||^2: pose workgroups, point workgroups, line workgroups
    Arr<GbaStats> stats;
    Arr<double> hmax, x;                              // K26's result; the pose parameters x_kf
};

// the room the lists take: the CSR id lists (a device-built plan carves every observation's room before it knows how many
// are kept, and sets the arrays' byte counts afterwards), the blocks, chunks and pairs
struct GbaListRoom { size_t lpo, llo, kpo, klo, nblk, nchunk, npair; };

// (gba.hip) the three layouts: base = nullptr gives the size alone
size_t gba_carve_stat(plslam_gba_plan* G, const GbaListRoom& r, char* base);
size_t gba_carve_pairs(plslam_gba_plan* G, const GbaListRoom& r, char* base);
size_t gba_carve_work(plslam_gba_plan* G, char* base);
// (gba.hip) the plan's dimensions from the call's arguments: n, npad, nt
void gba_plan_dims(plslam_gba_plan* G, plslam_ctx* ctx, int32_t n_map_kf, int32_t nkf, int32_t npt, int32_t nls, int32_t n_pt_obs,
                   int32_t n_ls_obs);
// (gba.hip) the arguments both plan builders refuse before anything else happens
int gba_plan_args_ok(plslam_ctx* ctx, const plslam_cam* K, double homog_th, int32_t n_map_kf, int32_t nkf, const void* kf_list, int32_t npt,
                     int32_t nls, const void* pt_obs, const void* pt_obs_uv, int32_t n_pt_obs, const void* ls_obs, const void* ls_l_obs,
                     int32_t n_ls_obs, plslam_gba_plan** out);
// (gba.hip) a plan that is not returned: its LBA plan, its buffers and the object itself go; returns rc
int gba_fail(plslam_gba_plan* G, int rc);

}  // namespace plslam

struct plslam_gba_plan {
    plslam_ctx* ctx = nullptr;
    plslam_lba_plan* lba = nullptr;
    int32_t n_map = 0, nkf = 0, npt = 0, nls = 0, np = 0, nl = 0;
    int64_t n = 0, npad = 0;
    int32_t nblk = 0, nchunk = 0, nt = 0;
    int64_t npair = 0;
    std::vector<int32_t> kf_list;           // map index of optimised keyframe k
    plslam::DevBuf stat, pairbuf, work, Sbuf;
    plslam::GbaStatView st;
    plslam::GbaWorkView wk;
    bool optimized = false;                 // an optimize has left its landmarks in the LBA plan's resident state
    // ---- a plan built on the device (plslam_gba_plan_create_dev): the builders' scratch, which the last kernels of the build
    // read behind the call, and the page-locked words the counts come back in
    plslam::DevBuf aux, aux_pairs;
    plslam::HostBuf pin_cnt;

    // workgroups of K38 / K37<3> / K37<6>: each leaves one partial of ||DX||^2
    int nwk() const { return (nkf + 255) / 256; }
    int nwp() const { return (npt + 255) / 256; }
    int nwl() const { return (nls + 255) / 256; }
    void release() { stat.release(); pairbuf.release(); work.release(); Sbuf.release(); aux.release(); aux_pairs.release(); pin_cnt.release(); }
};
