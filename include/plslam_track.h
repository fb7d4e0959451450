/* plslam_track.h -- tracking a batch of stereo pairs on the device: from the match tables and stereo gates of a match plan
 * (plslam_match_plan_run with plslam_match_plan_add_stereo_gates) to the relative pose prev -> curr of every pair, without
 * the host in between.  Part of libplslam_hip.so; the records of the loop-closure check (plslam_cam, plslam_lc_params,
 * plslam_lc_result) are reused as they stand.
 *
 * Per pair b, all arithmetic in fp64, no FMA contraction, operations in the order written:
 *
 *   point correspondence (i1, i2)  iff  i2 = m_pt[i1], 0 <= i2 < n_pt_curr, st_pt_prev[i1] >= 0, st_pt_curr[i2] >= 0
 *     (the prev <-> curr table is taken over EVERY left feature, so that it can run in the same plan as L <-> R; stvo-pl
 *     tracks stereo features only, which is what the two stereo tests restore).  An out-of-range entry is no correspondence.
 *     Rows are in ascending i1, as MapHandler::isLoopClosure builds lc_points / lc_lines (src/mapHandler.cpp:3225-3268).
 *   point row:  (u, v) = kp_prev[i1] widened to double, d = disp_pt_prev[i1], bd = b / d,
 *               P = (bd * (u - cx), bd * (v - cy), bd * fx)
 *                 -- stvo-pl's PinholeStereoCamera::backProjection, stated here from memory of that text [RECALL]: stvo-pl is
 *                    not in the tree, and the parity with it is not pinned by a test (as for the stereo gates);
 *               pl_obs = kp_curr[i2] widened.
 *   line row:   sP = backProjection(sx, sy, disp_ls_prev[2 i1]), eP = backProjection(ex, ey, disp_ls_prev[2 i1 + 1]) from
 *               seg_prev[i1]; le_obs from seg_curr[i2] = (sx, sy, ex, ey) widened:
 *               le = (sy - ey, ex - sx, sx * ey - sy * ex)   (Eigen's cross product of (sx, sy, 1) and (ex, ey, 1)),
 *               n = sqrt(le0 * le0 + le1 * le1), le_obs = (le0 / n, le1 / n, le2 / n)   (three divisions).
 *   No special cases: a kept zero-length segment gives NaN, a kept zero disparity gives inf.
 *
 * The rows of the whole batch are packed tightly: pair b owns rows [pt_off[b], pt_off[b + 1]) and [ls_off[b], ls_off[b + 1]).
 * Behind them runs computeRelativePoseRobustGN for the B pairs in one launch (K54): results[b] is what
 * plslam_relpose_robust_gn returns for pair b's rows, bit for bit (clk_* apart); its loop-closure decision fields are computed
 * as always and may be ignored. */
#ifndef PLSLAM_TRACK_H
#define PLSLAM_TRACK_H

#include "plslam_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct plslam_track_batch plslam_track_batch;

/* One stereo pair (prev, curr): device pointers, valid for the life of the object; a kind without rows: NULL / 0.
 * m_*: the prev <-> curr match table (n_*_prev entries: index into curr or -1); st_*: the stereo tables of the two frames
 * (plslam_stereo_gate_problem.stereo_12); disp_*: prev's disparities (points: n doubles, lines: 2 n); kp: n x 2 float32,
 * seg: n x 4 float32 (sx, sy, ex, ey) of the LEFT images. */
typedef struct plslam_track_pair {
    const int32_t* m_pt;
    const int32_t* st_pt_prev;
    const double* disp_pt_prev;
    const float* kp_prev;
    const int32_t* st_pt_curr;
    const float* kp_curr;
    int32_t n_pt_prev, n_pt_curr;
    const int32_t* m_ls;
    const int32_t* st_ls_prev;
    const double* disp_ls_prev;
    const float* seg_prev;
    const int32_t* st_ls_curr;
    const float* seg_curr;
    int32_t n_ls_prev, n_ls_curr;
} plslam_track_pair;

/* The object's outputs (device memory, owned by the object, the same addresses for its whole life).  pt_capacity /
 * ls_capacity: the rows the row arrays hold = the sum of n_pt_prev / n_ls_prev over the pairs; rows at and past
 * pt_off[B] / ls_off[B] are never written.  B == 0: every pointer is NULL. */
typedef struct plslam_track_buffers {
    const int32_t* pt_off;          /* B + 1 */
    const int32_t* ls_off;          /* B + 1 */
    const int32_t* pt_rows;         /* pt_capacity x 2: (i1, i2) */
    const int32_t* ls_rows;         /* ls_capacity x 2 */
    const double* P;                /* pt_capacity x 3 */
    const double* pl_obs;           /* pt_capacity x 2 */
    const double* sPeP;             /* ls_capacity x 6 */
    const double* le_obs;           /* ls_capacity x 3 */
    const uint8_t* pt_inlier;       /* pt_capacity: the flags after the outlier pass */
    const uint8_t* ls_inlier;       /* ls_capacity */
    const plslam_lc_result* results; /* B */
    int64_t pt_capacity, ls_capacity;
    int32_t B, reserved;
} plslam_track_buffers;

/* params: as for plslam_relpose_robust_gn (its match and gate fields are ignored), cam.fx, cx, cy and b are the
 * back-projection's; pairs: B host records, copied.
 * EINVAL: a NULL argument, a NULL array where rows exist (a kind's prev arrays when n_*_prev > 0, its curr arrays when both
 *         counts are > 0), a negative count, B < 0, params outside plslam_relpose_robust_gn's;
 * ERANGE: B > PLSLAM_LC_MAX_BATCH, a count over PLSLAM_LC_MAX_FEATURES, 2^31 rows or more of one kind in all.
 * B == 0 is an object whose run launches nothing.  A failed create leaves nothing allocated and *out NULL. */
int plslam_track_batch_create(plslam_ctx* ctx, const plslam_lc_params* params, const plslam_track_pair* pairs, int32_t B,
                              plslam_track_batch** out);
/* Enqueued behind `stream` (NULL = the context's stream), no synchronisation: K108 counts, K109 scans, K110 writes the rows,
 * K54 solves.  What `stream` is given next sees the outputs. */
int plslam_track_batch_run(plslam_track_batch* batch, void* stream);
int plslam_track_batch_device_buffers(plslam_track_batch* batch, plslam_track_buffers* out);
/* For tests and tools: waits for the context's stream and copies the outputs to host arrays of the sizes
 * plslam_track_buffers states (the row arrays in full, to their capacity); any of them may be NULL. */
int plslam_track_batch_download(plslam_track_batch* batch, int32_t* pt_off, int32_t* ls_off, int32_t* pt_rows, int32_t* ls_rows,
                                double* P, double* pl_obs, double* sPeP, double* le_obs, uint8_t* pt_inlier, uint8_t* ls_inlier,
                                plslam_lc_result* results);
void plslam_track_batch_destroy(plslam_track_batch* batch);

/* One frame's back-projection indexed by LEFT row, by the device function the tracker uses: lines == 0: f_l = n_l x 2 key
 * points, disp n_l, P_or_sPeP n_l x 3, pl_or_le n_l x 2; lines != 0: f_l = n_l x 4 segments, disp 2 n_l, P_or_sPeP n_l x 6,
 * pl_or_le n_l x 3 (the line through the LEFT segment).  Rows with stereo_12 < 0 are written as zeros.  Device pointers,
 * enqueued behind `stream` (NULL = the context's stream), no synchronisation.  EINVAL: NULL where n_l > 0, n_l < 0. */
int plslam_stereo_backproject_dev(plslam_ctx* ctx, const plslam_cam* cam, const int32_t* stereo_12, const double* disp,
                                  const float* f_l, int32_t n_l, int32_t lines, double* P_or_sPeP, double* pl_or_le,
                                  void* stream);

#ifdef __cplusplus
}
#endif

#endif /* PLSLAM_TRACK_H */
