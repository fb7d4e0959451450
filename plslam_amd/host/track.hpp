// track.hpp -- C++ host shim of include/plslam_track.h: PLSLAM::TrackBatch owns a plslam_track_batch over the caller's device
// tables (a match plan's match tables and stereo gates, the frames' key points and segments) and turns them, run after run,
// into the packed prev -> curr correspondences and the relative pose of every pair -- K108-K110 in front of K54, enqueued on
// the caller's stream.  Header-only; link with libplslam_hip.so.  Errors throw std::runtime_error.
#pragma once

#include <stdint.h>

#include <stdexcept>
#include <string>
#include <vector>

#include "plslam_track.h"

namespace PLSLAM {

class TrackBatch {
public:
    // pairs: device pointers that stay valid for the life of the object (the records themselves are copied)
    TrackBatch(plslam_ctx* ctx, const plslam_lc_params& params, const std::vector<plslam_track_pair>& pairs) : B_((int32_t)pairs.size())
    {
        check(plslam_track_batch_create(ctx, &params, pairs.data(), B_, &h_), "plslam_track_batch_create");
    }
    ~TrackBatch() { plslam_track_batch_destroy(h_); }
    TrackBatch(const TrackBatch&) = delete;
    TrackBatch& operator=(const TrackBatch&) = delete;

    int32_t size() const { return B_; }

    // enqueue only: behind `stream` (nullptr: the context's stream), no synchronisation
    void run(void* stream = nullptr) { check(plslam_track_batch_run(h_, stream), "plslam_track_batch_run"); }

    // the device-resident outputs: the same addresses for the life of the object
    plslam_track_buffers buffers() const
    {
        plslam_track_buffers b;
        check(plslam_track_batch_device_buffers(h_, &b), "plslam_track_batch_device_buffers");
        return b;
    }

    // everything on the host, after a synchronisation (tools and tests); the row arrays in full, to their capacity
    struct Host {
        std::vector<int32_t> pt_off, ls_off, pt_rows, ls_rows;
        std::vector<double> P, pl_obs, sPeP, le_obs;
        std::vector<uint8_t> pt_inlier, ls_inlier;
        std::vector<plslam_lc_result> results;
    };
    Host download() const
    {
        const plslam_track_buffers b = buffers();
        const size_t np = (size_t)b.pt_capacity, nl = (size_t)b.ls_capacity, nb = (size_t)B_;
        Host o;
        o.pt_off.assign(nb + 1, 0); o.ls_off.assign(nb + 1, 0);
        o.pt_rows.assign(2 * np, 0); o.ls_rows.assign(2 * nl, 0);
        o.P.assign(3 * np, 0.0); o.pl_obs.assign(2 * np, 0.0); o.sPeP.assign(6 * nl, 0.0); o.le_obs.assign(3 * nl, 0.0);
        o.pt_inlier.assign(np, 0); o.ls_inlier.assign(nl, 0);
        o.results.assign(nb, plslam_lc_result{});
        check(plslam_track_batch_download(h_, o.pt_off.data(), o.ls_off.data(), o.pt_rows.data(), o.ls_rows.data(), o.P.data(),
                                          o.pl_obs.data(), o.sPeP.data(), o.le_obs.data(), o.pt_inlier.data(), o.ls_inlier.data(),
                                          o.results.data()), "plslam_track_batch_download");
        return o;
    }

private:
    static void check(int rc, const char* where)
    {
        if (rc != PLSLAM_OK)
            throw std::runtime_error(std::string(where) + ": " + plslam_strerror(rc) + "; " + plslam_last_error());
    }

    plslam_track_batch* h_ = nullptr;
    int32_t B_;
};

}  // namespace PLSLAM
