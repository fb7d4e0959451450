// map2kf_dev.hpp -- the launchers of map2kf_kernels.hip (all asynchronous on `s`): what the map <-> keyframe and keyframe <->
// keyframe drivers (map2kf.hip) and the gate / visibility host calls (host_calls.hip) see of the kernels.
#pragma once

#include "common.hpp"

namespace plslam {

struct GridDesc;    // match_grid.hpp

// K5 / K6, the epipolar gates over nq rows the host knows; count (may be nullptr) is cleared here
int launch_point_gate(const plslam_cam& K, const double* Twf16, const double* Xw, const int32_t* m12,
                      int32_t nq, const double* pl, double th, uint8_t* mask, int32_t* count,
                      hipStream_t s);
int launch_line_gate(const plslam_cam& K, const double* Twf16, const double* Lw, const int32_t* m12,
                     int32_t nq, const double* le, double th, uint8_t* mask, int32_t* count,
                     hipStream_t s);
// the epipolar gate with the row count on the device (*n_dev <= n_max) and, optionally, the association behind it
int launch_gate_n(int lines, const plslam_cam& K, const double* Twf16, const double* LM, const int32_t* m12, const int32_t* n_dev,
                  int32_t n_max, const double* feat, double th, uint8_t* mask, int32_t* count, const int32_t* idx, const int32_t* ti,
                  int32_t* map_to_kf, hipStream_t s, int32_t* publish_done = nullptr, const int32_t* publish_src = nullptr,
                  int32_t* publish_dst = nullptr, int32_t publish_n = 0);
// the visibility pre-filter; _cand: AND the candidate flags, both on the device
int launch_visible(const plslam_cam& K, const double* Twf16, const double* X, int32_t n, int lines,
                   uint8_t* vis, hipStream_t s);
int launch_visible_cand(const plslam_cam& K, const double* Twf16, const double* X, const uint8_t* cand, int32_t n, int lines,
                        uint8_t* vis, hipStream_t s);
// cells (n x [1|2] x 2 int32) of the projected landmarks in grid units; lines: also dir1 (n x 2)
int launch_project_cells(const plslam_cam& K, const double* Twf16, const double* X, int32_t n, int lines, double inv_w,
                         double inv_h, int32_t* cells, double* dir1, hipStream_t s);
// visibility x candidate flags -> stable list + length (+ -1 fill of the association table, + the row count into a matchGrid
// descriptor); part: visible_compact_part_words(n) (map2kf_plan.hpp) zeroed device words
int launch_visible_compact(const plslam_cam& K, const double* Twf16, const double* X, const uint8_t* cand, int32_t n, int lines,
                           int32_t* idx, int32_t* n_out, int32_t* fill, GridDesc* desc, uint32_t* part, bool part_zeroed, hipStream_t s);
// Q rows + landmarks + window centres of the listed landmarks
int launch_prepare_rows(const plslam_cam& K, const double* Twf16, const void* md, const double* lm, const int32_t* idx,
                        const int32_t* n_dev, int32_t n_max, int lines, double inv_w, double inv_h, void* Q, double* QL, int32_t* cells,
                        double* dir1, hipStream_t s);
// dst[i] = src[idx[i]] for rows of row_bytes (a multiple of 8) bytes
int launch_gather_rows(const void* src, const int32_t* idx, int32_t n, int32_t row_bytes, void* dst,
                       hipStream_t s);
// n (<= 64) device words -> dst (page-locked, mapped), one lane per word
int launch_publish_words(const int32_t* src, int32_t* dst, int n, hipStream_t s);

}  // namespace plslam
