/*
 * plslam_hip.h -- C ABI of the MI355X (gfx950) implementation of PL-SLAM's stereo
 * point+line matching front end and local-BA row build.
 *
 * This is the drop-in boundary: every entry point is extern "C", takes plain pointers and
 * sizes, never throws, and returns PLSLAM_OK (0) or a negative PLSLAM_E* code.  Each one
 * cites the reference interface it replaces (paths relative to the pl-slam repository).
 *
 * Descriptor matrices are N x 32 uint8, row-major, contiguous -- the layout of the
 * reference's cv::Mat descriptor blocks (ORB: DBoW2 FORB::L = 32,
 * 3rdparty/DBoW2/include/DBoW2/FORB.h:31; LBD: cv::Mat(n,32,CV_8UC1),
 * 3rdparty/line_descriptor/src/binary_descriptor_custom.cpp:639) and of the matrices the
 * map-level drivers assemble with Mat::push_back (src/mapHandler.cpp:555,567,660,672).
 * Rows must start on 4-byte boundaries (any cv::Mat / hipMalloc / torch allocation does).
 *
 * Pointer conventions: entry points WITHOUT a _dev suffix take HOST pointers and do their
 * own H2D/D2H on the context's stream; *_dev entry points and match plans take DEVICE
 * pointers and a hipStream_t (passed as void*) and are asynchronous with respect to the host.
 * A NULL stream means "the context's own (non-blocking) stream", NOT HIP's legacy default stream:
 * callers that need ordering against their own work must pass a real stream handle.
 *
 * Threading: the reference calls StVO::match() concurrently from the VO thread, the local
 * mapping thread and the loop-closure thread (app/plslam_dataset.cpp:127,
 * src/mapHandler.cpp:1103, :1164 -> :3223).  Host-pointer entry points serialise on the
 * context; use one context per thread for concurrency.  Plans are immutable after
 * creation; plslam_match_plan_run may be issued from any one thread at a time per plan.
 *
 * There is NO CPU fallback: without a HIP device plslam_ctx_create fails with
 * PLSLAM_ENODEV and nothing else can be called.
 */
#ifndef PLSLAM_HIP_H
#define PLSLAM_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 2: plslam_match_problem grew (keep_prior, reserved: 56 bytes), plslam_lba_plan_iterate's flags became a bit mask, options
 * "mfma_form" 3/4 and "exact_second"; 3 (round 4): "mfma_form" 5 (the default), "post_fuse", plslam_match_plan_key_state;
 * 4 (round 5): plslam_match_plan_set_wire16, the Schur step, plslam_lba_plan_host_state; 5 (round 6): plslam_lba_plan_get_landmarks, plslam_lba_plan_iterate_schur / _apply_step, plslam_lba_point_rows_dev_n / _line_rows_dev_n, plslam_match_plan_step_gather / _gather_sync, plslam_rccl_use / _rccl_available; additive within 5: the plslam_bow_* bag-of-words entry points; the loop-closure check plslam_loop_closure_verify[_dev] /
 * plslam_relpose_robust_gn with plslam_lc_params / plslam_lc_keyframe / plslam_lc_result; the global bundle adjustment
 * plslam_gba_plan_create / plslam_gba_optimize / plslam_gba_plan_destroy and plslam_dense_ldlt_solve; the loop-closure
 * correction plslam_pgo_plan_create / plslam_pgo_optimize / plslam_pgo_plan_destroy, plslam_lc_correct_map[_dev] and
 * plslam_envelope_ldlt_solve with plslam_pgo_params / plslam_pgo_trial / plslam_pgo_result / plslam_lc_landmarks; the local map
 * plslam_local_map_* with plslam_map_index / plslam_map_landmarks / plslam_local_map_buffers / plslam_local_map_counts; the map
 * insertion plslam_map_insert_* with plslam_map_insert_kind / _dst / _counts / _events; the loop-closure landmark fusion
 * plslam_lc_fuse_* with plslam_lc_fuse_kind / _counts / _buffers; the device-built LBA plan plslam_lba_plan_create_dev with
 * plslam_lba_plan_list_sizes / _lists, and plslam_local_map_apply_lba (plslam_local_map_buffers / _counts grew at the END); the
 * loop-closure correction on the map image plslam_lc_correct_image with plslam_lc_image_dst / plslam_lc_image_counts.
 * Clients compare plslam_abi_version() with the value they were compiled against. */
#define PLSLAM_ABI_VERSION 5
#define PLSLAM_DESC_BYTES 32
/* largest train set of one directed scan: the composite (distance,index) key keeps 23
 * index bits beside the 9 distance bits */
#define PLSLAM_MAX_TRAIN_ROWS (1 << 23)

enum {
    PLSLAM_OK = 0,
    PLSLAM_EINVAL = -1,  /* bad argument (NULL pointer, negative size, misaligned rows)   */
    PLSLAM_ENODEV = -2,  /* no usable HIP device / wrong architecture                     */
    PLSLAM_EHIP = -3,    /* a HIP runtime call failed; see plslam_last_error()            */
    PLSLAM_ENOMEM = -4,  /* device or host allocation failed                              */
    PLSLAM_ERANGE = -5,  /* size beyond a documented limit (PLSLAM_MAX_TRAIN_ROWS)        */
    PLSLAM_ENOTSUP = -6  /* optional component unavailable (e.g. RCCL not loadable)       */
};

/* kernel variants of the directed Hamming scan (plslam_ctx_set_option "scan_variant") */
enum {
    PLSLAM_SCAN_AUTO = 0,
    PLSLAM_SCAN_LANE_PER_QUERY = 1, /* query in VGPRs, train rows streamed as SGPRs        */
    PLSLAM_SCAN_WAVE_PER_QUERY = 2, /* train tile in LDS, query in SGPRs, wave best-2 reduce */
    PLSLAM_SCAN_SYMMETRIC = 3,      /* mutual problems: one distance serves both directions */
    PLSLAM_SCAN_MFMA = 4            /* symmetric scan with the distances from the matrix cores:
                                       d = (256 - <s(a),s(b)>)/2 over +-1 fp4 codes, exact; non-mutual
                                       problems take its directed form                               */
};

typedef struct plslam_ctx plslam_ctx;
typedef struct plslam_match_plan plslam_match_plan;

/* Pinhole stereo camera: the fields of stvo-pl's PinholeStereoCamera that the reference
 * reads through cam->projection / getFx / getFy / getWidth / getHeight / getB
 * (src/mapHandler.cpp:255,550-551,1374,1384-1385). */
typedef struct plslam_cam {
    double fx, fy, cx, cy, b;
    int32_t width, height;
} plslam_cam;

const char* plslam_strerror(int code);
/* text of the last failure on the calling thread (HIP error string, file:line) */
const char* plslam_last_error(void);
int plslam_abi_version(void);

/* ---- context ------------------------------------------------------------------------ */
/* Binds to HIP device `device_ordinal` (must be gfx950), creates the context stream and
 * scratch pools.  Replaces nothing in the reference (it has no device state). */
int plslam_ctx_create(int device_ordinal, plslam_ctx** out);
void plslam_ctx_destroy(plslam_ctx* ctx);
/* options: "scan_variant" (PLSLAM_SCAN_*), "scan_block" (queries per workgroup of the directed
 * scan: 256|512|1024), "sym_rows" (rows of d1 per lane in the symmetric scan: 0 = auto (default) | 1 | 4),
 * "group_cap" (workgroups of one problem co-scheduled on one XCD: 0 = auto (default) | 1..64),
 * "mfma_form" (bookkeeping of the matrix-core scan: 0 = auto (default; = 5) | 1 = best-2 push per tile (K1e) |
 * 2 = group minima in the row direction + second best by recomputation (K1f) | 3 = two directed scans per mutual problem
 * (K1g) | 4 = group minima in both directions, class-major layouts (K1h) | 5 = K1h with the two M-tiles of a wave
 * software-pipelined against each other (K1i); identical match tables),
 * "post_fuse" (K1h / K1i plans: the stages behind the scan -- merge of the column partials, ratio test + mutual check, stereo
 * gates -- as ONE kernel with a workgroup per problem and the merged column keys in LDS: 0 = auto (default; = never: measured
 * slower than the separate kernels on MI355X although it moves 0.8 GB less per 4096-pair step) | 1 = never | 2 = whenever the
 * plan is eligible (every problem mutual, at most 4096 columns and 4096 rows); identical tables),
 * "exact_second" (K1h: 0 (default) = the index of a row's SECOND neighbour in the internal key tables is exact only where
 * it is an output (plslam_knn2_hamming256) and the column keys are completed lazily by the finalize stage | 1 = every key
 * of plslam_match_plan_dump is exact; match tables are identical either way),
 * "post_workgroups" (0 = default: one workgroup per block-table entry; n > 0: in a split run (plslam_match_plan_run_split) the
 * stages behind the scan -- K1h's merge of the column partials, the finalize kernel -- run as at most n workgroups that walk
 * their block tables, i.e. they hold a bounded number of workgroup slots beside the next scan; measured neutral to +1 %),
 * "split_post" (column-split plans of mutual problems -- a few LARGE problems, e.g. one local map against one frame: 0 = auto
 * (default): everything behind the scan is ONE kernel, which merges the column partials and decides the matches from the
 * column side -- two launches per run | 1 = never: merge kernel + finalize kernel; identical tables and counts),
 * "post_xcd" (how the finalize kernel's workgroups take the block table: 2 = default: the table is dealt to the eight XCDs problem
 * by problem, so the row blocks of one problem gather the problem's column keys through ONE L2 while consecutive problems sit on
 * different XCDs -- by the counters 0.36 instead of 1.0 GB fetched per 4096-pair step, step time equal or 1 % better | 1 = every
 * XCD takes a contiguous eighth of the table: the same bytes, measured 8 % SLOWER for the stage | 0 = table order: a problem's
 * six row blocks sit on six XCDs and each fetches the whole column table; identical tables),
 * "split_target", "split_min_tiles" (column-split plans: workgroups per CU the split aims at, 0 = 3; tiles of 32 columns per
 * range at least, 0 = 4),
 * "graph" (plslam_match_plan_run as ONE replayed HIP graph -- the run's launches captured on the caller's stream at its first
 * use: 0 = plans of fewer waves than the chip has SIMDs | 1 = never (default: measured SLOWER on ROCm 7 -- C3's three-kernel
 * run 26.9 us per back-to-back run against 22.3 us with plain launches) | 2 = always; never while profiling),
 * "fuse" (K1f: one workgroup per problem that also merges the column results and applies the ratio test + mutual
 * check, i.e. one kernel per plan run: 0 = auto (currently: never -- measured no faster) | 1 = never | 2 = always),
 * "grid_dense" (plslam_match_grid, process-wide: 1 (default) = a lone problem of at most 256 x 256 rows runs on ONE workgroup with
 * everything in LDS (the SLAM loop's 200 x 200 line problems) | 0 = the general kernels; identical tables),
 * "zero_copy_kb" (plslam_match_grid: n > 0 (default 64) = an upload image of at most n KB is read by the dense kernel where it
 * lies in page-locked host memory -- no copy command in front of the kernel: 57 -> 51 us per 200 x 200 call | -n = for the general
 * kernels too (measured neutral to slower: they read their inputs many times) | 0 = always copy; identical tables),
 * "lba_loop_peek" (plslam_lba_plan_optimize_dev: 1 (default) = between two passes the host looks at the loop's stop word where
 * the device writes it and stops enqueuing | 0 = all max_iters_lba passes are enqueued blindly; identical results) */
int plslam_ctx_set_option(plslam_ctx* ctx, const char* key, int value);
int plslam_ctx_get_option(plslam_ctx* ctx, const char* key, int* value);
/* device facts for reports: CU count, max clock (kHz), LDS bytes per workgroup */
int plslam_ctx_device_info(plslam_ctx* ctx, int32_t* cu_count, int32_t* clock_khz,
                           int32_t* lds_bytes, char* name, int32_t name_len);

/* ---- K1: brute-force Hamming kNN-2 ---------------------------------------------------- */
/* Replaces cv::BFMatcher::create(NORM_HAMMING,false)->knnMatch(q, t, matches, 2) as called by
 * stvo-pl's matchNNR (matching.cpp; reached from src/mapHandler.cpp:277,424,597,712,3223,3249).
 * idx, dist: nq*2 int32.  Order is lexicographic (distance, trainIdx): ties keep the lowest
 * train index, the second neighbour may share the first one's distance.  Absent neighbours
 * (nt < 2) are idx = -1, dist = INT32_MAX. */
int plslam_knn2_hamming256(plslam_ctx* ctx, const uint8_t* q, int32_t nq, const uint8_t* t,
                           int32_t nt, int32_t* idx, int32_t* dist);

/* ---- K1+K2: StVO::match ----------------------------------------------------------------- */
/* Replaces  int StVO::match(const cv::Mat& desc1, const cv::Mat& desc2, float nnr,
 *                           std::vector<int>& matches_12)           (stvo-pl matching.h,
 * included at src/mapHandler.cpp:28; call sites :277,:424,:597,:712,:3223,:3249).
 * matches_12 has n1 entries: matches_12[i1] = i2 or -1 (contract used at :280-283).
 * Ratio test in fp32: accept iff (float)d0 < (float)d1 * nnr.  mutual != 0 is the
 * reference's Config::bestLRMatches() (config/config/config_kitti.yaml:17): also run
 * desc2 -> desc1 and keep i1 -> i2 only if matches_21[i2] == i1.  n2 < 2 => no matches
 * (upstream indexes matches_[idx][1] out of range there; this ABI defines the case).
 * *n_matches (may be NULL) receives the return value of StVO::match. */
int plslam_match(plslam_ctx* ctx, const uint8_t* d1, int32_t n1, const uint8_t* d2, int32_t n2,
                 float nnr, int mutual, int32_t* matches_12, int32_t* n_matches);

/* StVO::match on a matches_12 that already holds n1 entries (in: the earlier table, out: the result); see
 * plslam_match_problem.keep_prior.  The drop-in header calls this when the caller's vector is not empty. */
int plslam_match_prior(plslam_ctx* ctx, const uint8_t* d1, int32_t n1, const uint8_t* d2, int32_t n2,
                       float nnr, int mutual, int32_t* matches_12, int32_t* n_matches);

/* B independent match() problems in one launch.  off1/off2 have B+1 row offsets into d1/d2;
 * matches_12 has off1[B] entries (problem b writes rows off1[b]..off1[b+1]); n_matches has B
 * entries (may be NULL).  This is the per-frame work of StereoFrame::extractStereoFeatures +
 * StereoFrameHandler::f2fTracking (stvo-pl; app/plslam_dataset.cpp:127) for a batch of frames. */
int plslam_match_batched(plslam_ctx* ctx, const uint8_t* d1, const int32_t* off1,
                         const uint8_t* d2, const int32_t* off2, int32_t B, float nnr,
                         int mutual, int32_t* matches_12, int32_t* n_matches);

/* ---- device-resident match plans (the throughput path) --------------------------------- */
/* One StVO::match problem with DEVICE pointers.  matches_12: n1 int32 (device).
 * n_matches: device pointer to one int32, or NULL. */
typedef struct plslam_match_problem {
    const uint8_t* d1;
    const uint8_t* d2;
    int32_t n1, n2;
    float nnr;
    int32_t mutual;
    int32_t* matches_12;
    int32_t* n_matches;
    /* 0: every row is written (-1 where nothing is accepted) -- StVO::match on a fresh vector.
     * 1: matches_12 already holds n1 entries and rows the ratio test rejects KEEP theirs; the consistency loop then
     *    runs over every entry >= 0 and n_matches = (rows accepted) - (entries cleared).  This is StVO::match on the
     *    vector matchGrid filled, src/mapHandler.cpp:271+277, :418+424, :591+597, :706+712 ([RECALL] stvo-pl matchNNR
     *    opens with matches_12.resize(desc1.rows, -1)). */
    int32_t keep_prior;
    int32_t reserved;
} plslam_match_problem;

typedef struct plslam_plan_info {
    int64_t distance_evals;    /* 256-bit distances evaluated per run (directed, as executed) */
    int64_t directed_evals;    /* distances the reference would evaluate (n1*n2 per direction) */
    int64_t algorithmic_bytes; /* sum over directed scans of 32*(Q+T) + 16*Q      */
    int32_t n_scans;           /* directed scans                                             */
    int32_t scan_blocks;       /* workgroups of the scan kernel                               */
    int32_t scan_variant;      /* PLSLAM_SCAN_* actually used                                 */
    int32_t scan_block_threads;
} plslam_plan_info;

/* Builds the immutable launch tables for `nprob` problems (host array of structs holding
 * device pointers) and uploads them.  Runs no kernel. */
int plslam_match_plan_create(plslam_ctx* ctx, const plslam_match_problem* probs, int32_t nprob,
                             plslam_match_plan** out);
/* Enqueues scan + finalize on `stream` (hipStream_t; NULL = context stream).  Asynchronous. */
int plslam_match_plan_run(plslam_match_plan* plan, void* stream);
/* The same with the scan kernel(s) on `scan_stream` and the stages behind them (merge of the column partials, finalize,
 * stereo gates, count scatter) on `post_stream`: a stream of runs -- of several plans or of this one -- then overlaps
 * each run's last stages (HBM-bound) with the next run's scan (instruction-issue-bound).  Ordering is the plan's
 * business: the stages wait for their scan, and the plan's next scan (split or not) waits for them.  Results are
 * complete when `post_stream` has drained.  A plan created with option "fuse" = 2 has no stage behind its scan (the scan
 * kernel writes the tables itself): it is not split, all of it runs on `scan_stream` and its results are complete when
 * THAT stream has drained. */
int plslam_match_plan_run_split(plslam_match_plan* plan, void* scan_stream, void* post_stream);
/* With profiling on, every run brackets each kernel with HIP events on the launch stream. */
int plslam_match_plan_set_profiling(plslam_match_plan* plan, int enable);
/* Synchronises the recorded events and returns accumulated kernel milliseconds since the
 * last call (then resets): the scan kernel(s) alone, then everything after them (merge of the
 * symmetric scan's column partials + finalize), and the number of profiled runs. */
int plslam_match_plan_elapsed(plslam_match_plan* plan, double* scan_ms, double* finalize_ms,
                              int64_t* runs);
int plslam_match_plan_info(plslam_match_plan* plan, plslam_plan_info* info);
/* Diagnostics (no reference counterpart): after a device-wide synchronise, copies the plan's intermediate key
 * table (per problem: n1 then n2 rows of two composite keys (distance << 23 | index), the state between the scan
 * and the finalize kernel) and the symmetric scan's per-workgroup column partials to the host.  Either buffer may be
 * NULL / too small: the sizes are always returned.  The determinism check (tools/determinism_check.py and its GPU
 * test) compares these words between repeated runs -- ~10^4 x more sensitive than the match tables, where only a
 * difference that flips a ratio test shows. */
int plslam_match_plan_dump(plslam_match_plan* plan, void* keys_out, size_t keys_cap, void* part_out,
                           size_t part_cap, size_t* keys_bytes, size_t* part_bytes);
/* What the key table of plslam_match_plan_dump holds for THIS plan (a bit mask; 0 = every word is an exact
 * (distance << 23 | index) key):
 *   PLSLAM_KEYS_ROW_SECOND_INDEX_INEXACT   the INDEX of a row's second key is the first column of its (group, class), not
 *                                          necessarily the second neighbour's (its distance is exact) -- K1h / K1i without
 *                                          "exact_second";
 *   PLSLAM_KEYS_COLUMN_SECOND_LAZY         a column's second key is (an upper bound of the second-best distance, index all
 *                                          ones): the stage behind the scan completes it where a match decision needs it;
 *   PLSLAM_KEYS_COLUMNS_NOT_IN_MEMORY      the merged column keys never reach memory (the fused stage behind the scan keeps
 *                                          them in LDS: option "post_fuse"); the table's column rows are unspecified.
 * Option "exact_second" = 1 at plan creation clears all three. */
#define PLSLAM_KEYS_ROW_SECOND_INDEX_INEXACT 1
#define PLSLAM_KEYS_COLUMN_SECOND_LAZY 2
#define PLSLAM_KEYS_COLUMNS_NOT_IN_MEMORY 4
int plslam_match_plan_key_state(plslam_match_plan* plan, int32_t* flags);
void plslam_match_plan_destroy(plslam_match_plan* plan);

/* ---- K14: StVO::matchGrid, the windowed ("fast_matching") matcher ------------------------------ */
/* Replaces  int StVO::matchGrid(const std::vector<point_2d>& points1, const cv::Mat& desc1,
 *                               const GridStructure& grid, const cv::Mat& desc2, const GridWindow& w,
 *                               std::vector<int>& matches_12)                       (points) and
 *           int StVO::matchGrid(const std::vector<line_2d>& lines1, const cv::Mat& desc1,
 *                               const GridStructure& grid, const cv::Mat& desc2,
 *                               const std::vector<std::pair<double,double>>& directions2,
 *                               const GridWindow& w, std::vector<int>& matches_12)  (lines)
 * of stvo-pl matching.h (un-vendored, [RECALL]); call sites src/mapHandler.cpp:271 (KF<->KF points), :418
 * (KF<->KF lines), :591 (map points <-> KF), :706 (map lines <-> KF).  This is the matcher the shipped
 * configurations use first (fast_matching: true); the callers fall back to StVO::match when it finds fewer than
 * min_*_matches (:274-278, :421-426, :594-598, :709-713).
 *   centres1   n1 x n_centres x 2 int32: the grid cells (x, y) whose windows supply row i1's candidates --
 *              n_centres = 1: points1[i1] (a point_2d = pair<int,int>); n_centres = 2: start and end point of
 *              lines1[i1].  Any int32 value is legal (GridStructure::get clamps the window to the grid).
 *   grid       the GridStructure the caller filled (:258-264, :395-411) in CSR form: cell (x, y), 0 <= x <
 *              grid_cols, 0 <= y < grid_rows, has id x*grid_rows + y and owns cell_items[cell_start[id] ..
 *              cell_start[id+1]-1]; items outside [0, n2) are ignored as upstream does.  GRID_COLS x GRID_ROWS
 *              is 64 x 48 upstream.
 *   window     {width.first, width.second, height.first, height.second} of the GridWindow (>= 0): cells
 *              x - window[0] .. x + window[1], y - window[2] .. y + window[3].
 *   dir1/dir2  line overload only (else NULL): unit directions of the query lines (what upstream computes from
 *              lines1[i1] with normalize()) and `directions2`; a candidate is skipped when |dot| < sim_th
 *              (Config::lineSimTh()).  A NaN direction (zero-length segment) never skips, as upstream.
 *   nnr        Config::minRatio12P(), used by BOTH overloads upstream; the test is `best_d < best_d2 * nnr` in
 *              fp64 with best_d2 = INT_MAX when there is no second candidate (a lone candidate is accepted).
 *   mutual     Config::bestLRMatches(): upstream's sequential `if (d < distances[i2]) {...} else continue;`
 *              (a candidate only counts for row i1 if it strictly beats every EARLIER row's distance to the
 *              same i2) followed by the matches_21[i2] == i1 check; reproduced exactly, order-free.
 *   matches_12 n1 entries (i2 or -1); *n_matches (may be NULL) the return value.  (With nnr > 1 -- no shipped
 *              configuration -- upstream also counts every row that had candidates none of which counted:
 *              `INT_MAX < INT_MAX * nnr`; reproduced, so there n_matches can exceed the entries >= 0.)
 * One deliberate definition: among several candidates at the same best distance upstream keeps the one its
 * std::unordered_set<int> happens to visit first (implementation-defined); here the lowest i2 wins, the
 * brute-force matcher's rule.  Limits: n1 < 2^22, n2 <= PLSLAM_MAX_TRAIN_ROWS. */
#define PLSLAM_MAX_GRID_ROWS (1 << 22)
int plslam_match_grid(plslam_ctx* ctx, const int32_t* centres1, int32_t n_centres, const uint8_t* d1,
                      int32_t n1, const int32_t* cell_start, const int32_t* cell_items, int32_t grid_cols,
                      int32_t grid_rows, const uint8_t* d2, int32_t n2, const double* dir1,
                      const double* dir2, double sim_th, const int32_t window[4], double nnr, int mutual,
                      int32_t* matches_12, int32_t* n_matches);

/* Device-resident form: a batch of matchGrid problems in ONE kernel launch (one workgroup per problem).
 * Every pointer of a problem is a DEVICE pointer; d1 / d2 must be 16-byte aligned.  pair_capacity sizes the
 * kernel's candidate store (mutual problems only; 0 otherwise): rows are handled in blocks of 1024 and a block
 * needs 1024 x (the number of grid items -- duplicates and out-of-range items included -- inside the windows of
 * its fullest row) entries of 4 bytes.  That size is always sufficient.  A problem whose candidates do not fit
 * matches nothing, gets n_matches = -1 and is counted by plslam_grid_plan_overflows.  (Problems of at most 2048 x 2048
 * rows whose tables fit the LDS keep their candidates there and use the store only for the excess: they may succeed
 * with less.) */
typedef struct plslam_grid_problem {
    const uint8_t* d1;
    const uint8_t* d2;
    const int32_t* centres1;
    const int32_t* cell_start;
    const int32_t* cell_items;
    const double* dir1;
    const double* dir2;
    int32_t n1, n2, n_centres, grid_cols, grid_rows;
    int32_t n_items; /* entries of cell_items: cell_start[grid_cols*grid_rows] must not exceed it (else: overflow) */
    int32_t window[4];
    double sim_th, nnr;
    int32_t mutual;
    int32_t pair_capacity;
    int32_t* matches_12;
    int32_t* n_matches; /* device pointer to one int32, or NULL */
} plslam_grid_problem;
typedef struct plslam_grid_plan plslam_grid_plan;
/* uploads the problem table and allocates the scratch (column lists, keys); runs no kernel */
int plslam_grid_plan_create(plslam_ctx* ctx, const plslam_grid_problem* probs, int32_t nprob,
                            plslam_grid_plan** out);
/* enqueues the kernel on `stream` (hipStream_t; NULL = the context's stream); asynchronous */
int plslam_grid_plan_run(plslam_grid_plan* plan, void* stream);
/* synchronises `stream` and returns the number of pair-list overflows since the last call */
int plslam_grid_plan_overflows(plslam_grid_plan* plan, void* stream, int32_t* n_overflows);
void plslam_grid_plan_destroy(plslam_grid_plan* plan);
/* plslam_grid_problem.pair_capacity from HOST copies of a problem's window centres and cell_start (pure host code, no
 * device needed).  exact: the documented size (rows in blocks of 1024, 1024 x the item count of a block's fullest row);
 * bound: an upper bound of it from the grid alone -- fullest cell x cells of a window (at most every item) x n_centres
 * per row -- for callers whose centres only exist on the device.  Either is sufficient.  0 for non-mutual problems. */
int64_t plslam_grid_pair_capacity(const int32_t* centres1, int32_t n1, int32_t n_centres, const int32_t* cell_start,
                                  int32_t grid_cols, int32_t grid_rows, const int32_t window[4], int mutual);
int64_t plslam_grid_pair_capacity_bound(int32_t n1, int32_t n_centres, const int32_t* cell_start, int32_t grid_cols,
                                        int32_t grid_rows, const int32_t window[4], int mutual);

/* ---- host-to-host pipeline: descriptors born on the host, tables wanted on the host -------------------------------- */
/* plslam_match_batched is strictly serial (H2D -> kernels -> D2H) and uploads every problem's rows separately.  A
 * pipeline is created ONCE for a batch shape: the host hands over one ARENA of descriptor rows per batch (any layout;
 * problems name byte offsets into it, so prev<->curr and L<->R problems share the rows of an image instead of carrying
 * copies: 109 kB per C2 stereo pair instead of 218 kB) and receives one int32 output table.  `depth` (2..8) batches are
 * in flight: the upload of batch k+1 and the download of batch k-1 run on their own HIP streams under the kernels of
 * batch k.  submit() returns as soon as the work is enqueued (it first waits for the batch that used the slot `depth`
 * submits ago); the output of a submit is complete after the submit that re-uses its slot or after wait().  Tables in
 * page-locked memory are written by the GPU itself behind the finalize (a copy-engine download would queue between two
 * uploads and serialise the pipeline).  Host
 * buffers should come from plslam_pinned_alloc (pageable memory works but the runtime then stages every copy itself). */
typedef struct plslam_arena_problem {
    int64_t d1_off, d2_off;      /* byte offsets of the two descriptor sets inside the arena (4-byte aligned)  */
    int32_t n1, n2;
    float nnr;
    int32_t mutual;
    int64_t out_off;             /* first entry of this problem's matches_12 inside the output table (int32 units) */
} plslam_arena_problem;
typedef struct plslam_match_pipeline plslam_match_pipeline;
int plslam_match_pipeline_create(plslam_ctx* ctx, size_t arena_bytes, const plslam_arena_problem* probs, int32_t nprob,
                                 size_t out_entries, int32_t depth, plslam_match_pipeline** out);
/* out_host / counts_host: page-locked AND 16-byte aligned buffers are written by a kernel straight from the compute
 * stream; anything else (pageable memory, an offset slice of a pinned buffer) takes a copy-engine download. */
int plslam_match_pipeline_submit(plslam_match_pipeline* pipe, const void* arena_host, int32_t* out_host,
                                 int32_t* counts_host /* nprob entries or NULL */);
int plslam_match_pipeline_wait(plslam_match_pipeline* pipe);
void plslam_match_pipeline_destroy(plslam_match_pipeline* pipe);
void* plslam_pinned_alloc(size_t bytes);      /* hipHostMalloc; NULL on failure */
void plslam_pinned_free(void* p);

/* ---- K15/K16: the stereo L<->R gates of StVO::StereoFrame ---------------------------------------- */
/* stvo-pl stereoFrame.cpp, matchStereoPoints / matchStereoLines ([RECALL]; the un-vendored dependency): what turns
 * the match table of (pdesc_l, pdesc_r) / (ldesc_l, ldesc_r) -- from StVO::match or StVO::matchGrid with the window
 * {matching_s_ws, 0, 0, 0} -- into the frame's stereo features.  Thresholds are the reference's config keys
 * max_dist_epip, min_disp, line_horiz_th, stereo_overlap_th, ls_min_disp_ratio
 * (config/config/config_kitti.yaml:25,26,34,31,36).
 *   points: kp = n x 2 float32 (cv::KeyPoint::pt.x, .y).  Kept iff |pt_l.y - pt_r.y| <= max_dist_epip (float
 *           subtraction) and disp = pt_l.x - pt_r.x >= min_disp.  disp: n_l doubles (0 where dropped).
 *   lines:  seg = n x 4 float32 (KeyLine startPointX, startPointY, endPointX, endPointY).  The right end points are
 *           moved along the right line to the rows of the left end points, disp_s / disp_e are the differences of x
 *           (both -1 when min/max < ls_min_disp_ratio); kept iff both >= min_disp, neither segment is horizontal
 *           (|dy| > line_horiz_th) and lineSegmentOverlapStereo of the y ranges > stereo_overlap_th.
 *           disp_se: n_l x 2 doubles.
 * stereo_12[i1] = i2 or -1; *n_stereo (may be NULL) = number kept. */
int plslam_stereo_point_gate(plslam_ctx* ctx, const int32_t* matches_12, int32_t n_l, const float* kp_l,
                             const float* kp_r, int32_t n_r, double max_dist_epip, double min_disp,
                             int32_t* stereo_12, double* disp, int32_t* n_stereo);
int plslam_stereo_line_gate(plslam_ctx* ctx, const int32_t* matches_12, int32_t n_l, const float* seg_l,
                            const float* seg_r, int32_t n_r, double min_disp, double line_horiz_th,
                            double stereo_overlap_th, double ls_min_disp_ratio, int32_t* stereo_12,
                            double* disp_se, int32_t* n_stereo);

/* Device-pointer forms: every pointer is a device pointer (kp / seg rows 8 / 16-byte aligned), the kernel is enqueued on
 * `stream` (NULL = the context's stream) and NOT synchronised; *n_stereo (device, may be NULL) is zeroed on the stream
 * first.  matches_12 is normally the device table a match plan or plslam_match_dev wrote. */
int plslam_stereo_point_gate_dev(plslam_ctx* ctx, const int32_t* matches_12, int32_t n_l, const float* kp_l,
                                 const float* kp_r, int32_t n_r, double max_dist_epip, double min_disp,
                                 int32_t* stereo_12, double* disp, int32_t* n_stereo, void* stream);
int plslam_stereo_line_gate_dev(plslam_ctx* ctx, const int32_t* matches_12, int32_t n_l, const float* seg_l,
                                const float* seg_r, int32_t n_r, double min_disp, double line_horiz_th,
                                double stereo_overlap_th, double ls_min_disp_ratio, int32_t* stereo_12,
                                double* disp_se, int32_t* n_stereo, void* stream);

/* The gate stage of a match plan: StereoFrame::matchStereoPoints / matchStereoLines for a whole batch.  Each gate
 * problem names the L<->R match table of one frame (usually the matches_12 of one of the plan's problems) and that
 * frame's key points / segments; after plslam_match_plan_add_stereo_gates, every plslam_match_plan_run ends with ONE
 * more launch that turns all those tables into stereo associations (stereo_12, disparities, counts).  All pointers are
 * device pointers and must stay valid for the life of the plan.  n_stereo: either NULL in every problem, or the
 * problems' counters form one contiguous int32 array (gates[i].n_stereo == gates[0].n_stereo + i).  Calling it again
 * replaces the stage; ngates = 0 removes it. */
typedef struct plslam_stereo_gate_problem {
    const int32_t* matches_12;   /* n_l entries: right index or -1                                    */
    const float* f_l;            /* n_l x 2 (points: pt.x, pt.y) or n_l x 4 (lines: sx, sy, ex, ey)  */
    const float* f_r;            /* n_r x 2 / n_r x 4                                                */
    int32_t n_l, n_r;
    int32_t lines;               /* 0 = points, 1 = lines                                            */
    int32_t pad;
    double max_dist_epip;        /* points  (config_kitti.yaml:25)                                   */
    double min_disp;             /* both    (:26)                                                    */
    double line_horiz_th;        /* lines   (:34)                                                    */
    double stereo_overlap_th;    /* lines   (:31)                                                    */
    double ls_min_disp_ratio;    /* lines   (:36)                                                    */
    int32_t* stereo_12;          /* out: n_l entries                                                 */
    double* disp;                /* out: n_l (points) or 2 n_l (lines: disp_s, disp_e) doubles       */
    int32_t* n_stereo;           /* out: number kept; may be NULL                                    */
} plslam_stereo_gate_problem;
/* (Calling it again replaces the stage: the call then waits for the device, so that no run still in flight reads tables
 * that are being replaced.) */
int plslam_match_plan_add_stereo_gates(plslam_match_plan* plan, const plslam_stereo_gate_problem* gates,
                                       int32_t ngates);

/* A 16-bit mirror of a plan's match tables (round 5): the wire format of the N > 1 table gather (the per-frame
 * tables the reference's loop would hand on, app/plslam_dataset.cpp:111-135).  Every problem whose matches_12 lies in
 * [table32, table32 + n_entries) also stores its entries, as int16, at the same index of table16 (device pointers) -- by the
 * kernel that decides them, so that no narrowing pass over the table is needed before the gather.  Requires n2 <= 32768 for
 * those problems and a plan whose tables are written by the finalize kernel (PLSLAM_ENOTSUP for fused and column-split
 * plans).  table16 = NULL removes the mirror.  Like plslam_match_plan_add_stereo_gates the call waits for the device. */
int plslam_match_plan_set_wire16(plslam_match_plan* plan, const int32_t* table32, int16_t* table16, size_t n_entries);

/* ---- K3/K4: local-BA residual + Jacobian rows ------------------------------------------- */
/* Both kinds of row, every entry point: std::max(homogTh, x) is computed as (homogTh > x ? homogTh : x), so a NaN x (a landmark
 * at depth zero, a NaN / inf input) gives a NaN row as in the reference, while a NaN homogTh -- where libstdc++'s std::max
 * returns the NaN -- is passed over and the rows stay finite: on purpose, a threshold that is not a number is no configuration
 * of the reference.  An entry that is not a number is stored as ONE NaN, 0x7FF8000000000000: which NaN an operation hands on
 * (sign, payload) is the hardware's choice and differs between the GPU and a host. */
/* Point rows: the per-observation body of MapHandler::levMarquardtOptimizationLBA,
 * src/mapHandler.cpp:1358-1407 (first pass) == :1587-1642 (iteration pass; the caller
 * supplies poses/landmarks from X).  fp64, no FMA contraction, reference operation order.
 *   T_kf_w  nkf*16  row-major KF->world poses (map_keyframes[kf]->T_kf_w, :1370)
 *   Xw      npt*3   landmarks (:1368)          obs_uv nobs*2 observations (:1375)
 *   lm_loc[o] -> row of Xw, kf_slot[o] -> pose in T_kf_w
 * out: J_pose nobs*6 (:1392-1398, tangent order [t, w]), J_lm nobs*3 (:1401-1404),
 *      r nobs (||p_err||, :1377), w nobs (robustWeightCauchy, :1407). */
int plslam_lba_point_rows(plslam_ctx* ctx, const plslam_cam* K, double homog_th,
                          const double* T_kf_w, int32_t nkf, const double* Xw, int32_t npt,
                          const double* obs_uv, const int32_t* lm_loc, const int32_t* kf_slot,
                          int32_t nobs, double* J_pose, double* J_lm, double* r, double* w);
/* Line rows: src/mapHandler.cpp:1436-1516.  compat_iter_pass != 0 reproduces the iteration
 * pass :1668-1748 as written: both endpoints read Lw[3*lm_loc .. +3] (:1678-1679) and the
 * threshold is the literal 1e-7 (:1698).  Lw holds n_lw doubles (6 per line landmark).
 * out: J_pose nobs*6 (:1509), J_lm nobs*6 (:1486,:1506,:1512-1513), r (:1460), w (:1516). */
int plslam_lba_line_rows(plslam_ctx* ctx, const plslam_cam* K, double homog_th,
                         int compat_iter_pass, const double* T_kf_w, int32_t nkf,
                         const double* Lw, int32_t n_lw, const double* l_obs,
                         const int32_t* lm_loc, const int32_t* kf_slot, int32_t nobs,
                         double* J_pose, double* J_lm, double* r, double* w);
/* device-pointer forms (all arrays on the device; asynchronous on `stream`) */
int plslam_lba_point_rows_dev(plslam_ctx* ctx, const plslam_cam* K, double homog_th,
                              const double* T_kf_w, const double* Xw, const double* obs_uv,
                              const int32_t* lm_loc, const int32_t* kf_slot, int32_t nobs,
                              double* J_pose, double* J_lm, double* r, double* w, void* stream);
int plslam_lba_line_rows_dev(plslam_ctx* ctx, const plslam_cam* K, double homog_th,
                             int compat_iter_pass, const double* T_kf_w, const double* Lw,
                             const double* l_obs, const int32_t* lm_loc, const int32_t* kf_slot,
                             int32_t nobs, double* J_pose, double* J_lm, double* r, double* w,
                             void* stream);
/* The same with the length of T_kf_w stated (ABI v5, round 6): n_pose_slots = the number of 4 x 4 matrices behind T_kf_w (> max
 * kf_slot).  The kernels then keep the first 32 of them in LDS instead of gathering them from global memory row by row: K3 at C3
 * sizes 0.345 -> 0.276 ms per 12.8 M rows.  n_pose_slots = 0 is the call above.  Identical rows. */
int plslam_lba_point_rows_dev_n(plslam_ctx* ctx, const plslam_cam* K, double homog_th,
                                const double* T_kf_w, int32_t n_pose_slots, const double* Xw, const double* obs_uv,
                                const int32_t* lm_loc, const int32_t* kf_slot, int32_t nobs,
                                double* J_pose, double* J_lm, double* r, double* w, void* stream);
int plslam_lba_line_rows_dev_n(plslam_ctx* ctx, const plslam_cam* K, double homog_th,
                               int compat_iter_pass, const double* T_kf_w, int32_t n_pose_slots, const double* Lw,
                               const double* l_obs, const int32_t* lm_loc, const int32_t* kf_slot,
                               int32_t nobs, double* J_pose, double* J_lm, double* r, double* w,
                               void* stream);

/* ---- K7-K10: normal equations of the local BA in block form ------------------------------- */
/* Replaces the accumulation into the dense H / g of levMarquardtOptimizationLBA
 * (src/mapHandler.cpp:1410-1429 points, :1519-1538 lines) by its block structure:
 *   g       N = 6*nkf + 3*npt + 6*nls      (the layout of the reference's X / g)
 *   H_pose  nkf * 6x6   H.block(idx,idx,6,6)          H_pt  npt * 3x3   H.block(jdx,jdx,3,3)
 *   H_ls    nls * 6x6   H.block(jdx,jdx,6,6)
 *   W_pt    n_pt_obs * 3x6   the observation's Haux = H.block(jdx,idx,3,6) contribution (:1424-1426)
 *   W_ls    n_ls_obs * 6x6   (:1533-1535); zero when kf_loc == -1 (keyframe not optimised, :1413)
 *   err     sum r^2 w (:1416,1423,1525,1532)
 * Inputs are the rows of plslam_lba_*_rows plus the Vector6i columns lm_loc (1) and kf_loc (4)
 * (:1259,1263).  Every block entry is the sequential sum over the observations in list order
 * (points, then lines), i.e. the dense accumulation's own order; all blocks row-major. */
int plslam_lba_assemble(plslam_ctx* ctx, int32_t nkf, int32_t npt, int32_t nls,
                        const int32_t* pt_lm_loc, const int32_t* pt_kf_loc, int32_t n_pt_obs,
                        const double* pt_J_pose, const double* pt_J_lm, const double* pt_r,
                        const double* pt_w, const int32_t* ls_lm_loc, const int32_t* ls_kf_loc,
                        int32_t n_ls_obs, const double* ls_J_pose, const double* ls_J_lm,
                        const double* ls_r, const double* ls_w, double* g, double* H_pose,
                        double* H_pt, double* H_ls, double* W_pt, double* W_ls, double* err);

/* LBA plan: levMarquardtOptimizationLBA rebuilds rows + H/g once (:1358-1540) and then up to
 * max_iters_lba = 15 times (:1587-1772) while only X changes.  The plan uploads what is constant --
 * the Vector6i columns lm_loc (1) / kf_loc (4), the pose slot of each observation, the observations
 * themselves -- once; iterate() uploads poses (n_pose_slots*16, e.g. expmap_se3 of X, :1600-1603) and
 * landmarks (X.block(6Nkf..), :1597, :1678), runs K3/K4 and K7-K10 on the device and returns the
 * block-form normal equations (layout as plslam_lba_assemble).
 * Pose slots are per observation and separate for points and lines on purpose: in the iteration pass the reference
 * gives an optimised key frame's POINT observations the current estimate expmap_se3(X.block(6*kf_loc..)) (:1600-1601)
 * but its LINE observations the stored map_keyframes[kf]->T_kf_w (:1680) -- a caller that wants the reference's
 * numbers keeps one slot per key frame with the stored pose for ls_pose_slot and a second set with the current
 * estimates for pt_pose_slot, and passes compat_iter_pass = 1 (stride-3 end points :1677-1678, literal 1e-7 :1698).
 * All three quirks are checked against the reference's own source text by the CPU test suite. */
typedef struct plslam_lba_plan plslam_lba_plan;
int plslam_lba_plan_create(plslam_ctx* ctx, const plslam_cam* K, double homog_th, int32_t n_pose_slots,
                           int32_t nkf, int32_t npt, int32_t nls, const int32_t* pt_lm_loc,
                           const int32_t* pt_pose_slot, const int32_t* pt_kf_loc, const double* pt_obs_uv,
                           int32_t n_pt_obs, const int32_t* ls_lm_loc, const int32_t* ls_pose_slot,
                           const int32_t* ls_kf_loc, const double* ls_l_obs, int32_t n_ls_obs,
                           plslam_lba_plan** out);
/* compat_flags (a bit mask; 1 keeps its round-1 meaning "compat_iter_pass"):
 *   PLSLAM_LBA_COMPAT_ITER_PASS  the iteration pass's line quirks (see above)
 *   PLSLAM_LBA_COMPAT_GBA        levMarquardtOptimizationGBA writes the pose x line cross blocks TRANSPOSED
 *                                (src/mapHandler.cpp:2341-2352 against :1531-1532; H stays symmetric but the block is
 *                                J_l J_p^T where J_p J_l^T belongs): W_ls comes out the way the reference's GBA fills it */
#define PLSLAM_LBA_COMPAT_ITER_PASS 1
#define PLSLAM_LBA_COMPAT_GBA 2
int plslam_lba_plan_iterate(plslam_lba_plan* plan, const double* T_kf_w, const double* Xw, const double* Lw,
                            int compat_flags, double* g, double* H_pose, double* H_pt, double* H_ls,
                            double* W_pt, double* W_ls, double* err);
/* The same iteration with the blocks LEFT ON THE DEVICE: X goes up (0.34 MB at C3), only *err (and g, N doubles, unless
 * NULL) comes down -- not the 11.5 MB of blocks that made the host-to-host iteration 2.3 ms for 0.1 ms of kernels.
 * plslam_lba_plan_device_blocks names the device arrays (valid until the next iterate / destroy; ordered on `stream`, the
 * context's stream) for a device-side Schur complement / solver; plslam_lba_plan_blocks downloads any of them afterwards
 * (NULL = skip). */
int plslam_lba_plan_iterate_dev(plslam_lba_plan* plan, const double* T_kf_w, const double* Xw, const double* Lw,
                                int compat_flags, double* g, double* err);
typedef struct plslam_lba_blocks {
    const double *g, *H_pose, *H_pt, *H_ls, *W_pt, *W_ls, *err;   /* device pointers, layouts as plslam_lba_plan_iterate */
    void* stream;                                                  /* the HIP stream the blocks were computed on     */
} plslam_lba_blocks;
int plslam_lba_plan_device_blocks(plslam_lba_plan* plan, plslam_lba_blocks* out);
int plslam_lba_plan_blocks(plslam_lba_plan* plan, double* g, double* H_pose, double* H_pt, double* H_ls, double* W_pt,
                           double* W_ls, double* err);
/* The optimisation state itself on the device (round 4): after one plslam_lba_plan_iterate / _iterate_dev has uploaded it,
 * plslam_lba_plan_device_state names the device copies of T_kf_w (n_pose_slots x 16), Xw (npt x 3) and Lw (nls x 6) -- a
 * device-side solver applies its update to them in place (the reference's X <- X + delta, T <- T inv(exp(delta)),
 * src/mapHandler.cpp:1563-1568), on `stream` -- and plslam_lba_plan_iterate_resident runs the next iteration on them: no
 * upload, three launches, *err down (8 bytes).  Blocks as after plslam_lba_plan_iterate_dev. */
typedef struct plslam_lba_state {
    double *T_kf_w, *Xw, *Lw;                 /* device pointers */
    int32_t n_pose_slots, npt, nls;
    void* stream;                              /* the HIP stream the plan's iterations run on */
} plslam_lba_state;
int plslam_lba_plan_device_state(plslam_lba_plan* plan, plslam_lba_state* out);
int plslam_lba_plan_iterate_resident(plslam_lba_plan* plan, int compat_flags, double* err);
/* The plan's page-locked host images by name (round 5).  Every plslam_lba_plan_iterate / _iterate_dev copies the caller's
 * T_kf_w / Xw / Lw into one page-locked image (one upload) and g out of another (one download).  A host solver that keeps its
 * state IN that image -- X_aux of src/mapHandler.cpp:1231-1330 written there, X(i) += DX(i) applied there -- and reads g
 * there passes these very pointers to the iterate calls, which then skip both staging copies (0.34 MB each way at C3).  The
 * images belong to the plan (valid until plslam_lba_plan_destroy); the caller may write T / Xw / Lw and read g between calls
 * only (every plan call returns with the stream synchronised).  g is rewritten by every _iterate_dev with g != NULL;
 * pointers of any other origin keep working as before, array by array. */
typedef struct plslam_lba_host_state {
    double *T_kf_w, *Xw, *Lw;                 /* page-locked: n_pose_slots x 16, npt x 3, nls x 6 */
    double* g;                                 /* page-locked: n doubles (6 nkf + 3 npt + 6 nls) */
    int32_t n_pose_slots, npt, nls;
    int64_t n;
} plslam_lba_host_state;
int plslam_lba_plan_host_state(plslam_lba_plan* plan, plslam_lba_host_state* out);
/* The Schur step on the resident blocks (round 5) -- the solve of src/mapHandler.cpp:1544-1575 (and :1779-1800 in the loop)
 * with everything but a 6 nkf x 6 nkf system staying on the device.  The reference damps H(i,i) += lambda * H(i,i) and solves
 * the whole N x N system with a sparse LDLT; the landmark blocks of H are independent, so the same step is
 *     S dp = b,  S = Hpp' - sum_j Wj^T Vj'^-1 Wj,  b = gp - sum_j Wj^T Vj'^-1 gj,  dxj = Vj'^-1 (gj - Wj dp)
 * (Hpp', Vj': the damped pose / landmark blocks; Wj: the cross blocks of landmark j's observations).  All three calls work on
 * the blocks of the LAST plslam_lba_plan_iterate / _iterate_dev / _iterate_resident of the plan (run WITHOUT
 * PLSLAM_LBA_COMPAT_GBA: the transposed pose x line cross blocks of the reference's GBA are refused, PLSLAM_EINVAL).
 *   plslam_lba_plan_diag_max   *hmax = max |H(i,i)| over all N diagonal entries (the reference's "lambda *= Hmax", :1544-1550)
 *   plslam_lba_plan_schur      S (6 nkf x 6 nkf doubles, row-major, both triangles) and b (6 nkf) for the damping `lambda`;
 *                              *n_singular (may be NULL) = landmarks whose damped block is not positive definite (a zero
 *                              diagonal entry: no observation constrains that coordinate) -- they contribute nothing and get
 *                              a zero step.  Deterministic: fixed-shape sums, no atomics.
 *   plslam_lba_plan_backsub    the landmark steps for the pose step dpose (6 nkf doubles, the solution of S dp = b that the
 *                              host's dense LDLT found): dX_pt (npt x 3) / dX_ls (nls x 6), either may be NULL; apply != 0
 *                              also adds them to the resident Xw / Lw in place (X(i) += DX(i), :1570-1575).  Needs the
 *                              plslam_lba_plan_schur of the same blocks before it (its landmark inverses are reused).
 *   plslam_lba_plan_set_poses  uploads the poses alone (n_pose_slots x 16 doubles): the caller applies dp to them
 *                              (T <- T inv(exp(dp)), :1560-1566: the SE(3) maps stay on the host) -- after which
 *                              plslam_lba_plan_iterate_resident runs the next iteration with nothing else crossing PCIe. */
int plslam_lba_plan_diag_max(plslam_lba_plan* plan, double* hmax);
int plslam_lba_plan_schur(plslam_lba_plan* plan, double lambda, double* S, double* b, int32_t* n_singular);
int plslam_lba_plan_backsub(plslam_lba_plan* plan, const double* dpose, int apply, double* dX_pt, double* dX_ls);
int plslam_lba_plan_set_poses(plslam_lba_plan* plan, const double* T_kf_w);
/* An LM iteration of src/mapHandler.cpp:1583-1812 in TWO calls and two synchronisations (ABI v5, round 6):
 *   plslam_lba_plan_iterate_schur = plslam_lba_plan_iterate_resident + plslam_lba_plan_schur for a lambda known beforehand
 *                              (every iteration but the first pass, whose lambda needs plslam_lba_plan_diag_max): err, S, b and
 *                              the count of singular landmark blocks come back behind ONE synchronisation;
 *   plslam_lba_plan_apply_step = plslam_lba_plan_backsub(dpose, apply) + plslam_lba_plan_set_poses(T_kf_w; NULL = leave the
 *                              pose slots, a rejected step) + sum_i DX(i)^2 over the LANDMARK steps (dx_sumsq, may be NULL): with
 *                              |dpose|^2 added on the host this is the ||DX|| of the loop's last test (:1808), and 8 bytes
 *                              cross PCIe instead of the steps.  The sum is taken in a fixed order: the same bits on every run. */
int plslam_lba_plan_iterate_schur(plslam_lba_plan* plan, int compat_flags, double lambda, double* err, double* S, double* b,
                                  int32_t* n_singular);
int plslam_lba_plan_apply_step(plslam_lba_plan* plan, const double* dpose, const double* T_kf_w, int apply, double* dx_sumsq);
/* The resident landmarks, device -> host (ABI v5): Xw (npt x 3) / Lw (nls x 6), either may be NULL.  What
 * plslam_lba_plan_backsub(apply) updated in place comes back for the reference's write-back (src/mapHandler.cpp:1822-1852:
 * point3D / line3D <- X, inlier = false where ||X - old|| > 0.01).  The plan's page-locked images (plslam_lba_plan_host_state)
 * are refreshed by the same copy: after backsub(apply) the image holds the landmarks of BEFORE the step until this call (or the
 * caller) rewrites it -- an iterate / iterate_dev handed the image's pointers in between would upload the old ones. */
int plslam_lba_plan_get_landmarks(plslam_lba_plan* plan, double* Xw, double* Lw);
/* rows of the last iterate() (any pointer may be NULL), e.g. for the write-back logic of :1822-1855 */
int plslam_lba_plan_rows(plslam_lba_plan* plan, double* pt_J_pose, double* pt_J_lm, double* pt_r, double* pt_w,
                         double* ls_J_pose, double* ls_J_lm, double* ls_r, double* ls_w);
void plslam_lba_plan_destroy(plslam_lba_plan* plan);
/* The same plan built ON THE DEVICE from DEVICE columns (additive within 5; K74-K83, KERNELS.md): the eight observation columns
 * are device pointers with the layouts and meanings of plslam_lba_plan_create -- e.g. what plslam_local_map_gather leaves in
 * plslam_local_map_buffers -- read on the context's stream.  The range checks are the host call's, made on the device: an lm_loc,
 * kf_loc or pose_slot out of range gives PLSLAM_EINVAL and no plan, and no kernel follows a bad index; NULL and negative
 * arguments (and observations where npt / nls / n_pose_slots is 0) are refused before anything is launched.  The lists -- per
 * landmark, per keyframe, and on first use of the Schur step the pair lists -- are built on the device, equal entry for entry
 * to those plslam_lba_plan_create builds on the host (plslam_lba_plan_lists shows them); the plan keeps no host copy.  Every
 * plslam_lba_plan_* call works on the plan.  One synchronisation here, one when the Schur lists are built.
 *   d_Xw (npt x 3) / d_Lw (nls x 6)  device pointers or NULL: copied into the plan's resident landmarks (for the gather: X_aux +
 *                        6 nkf and X_aux + 6 nkf + 3 npt).  With both given (where the kind exists) ONE plslam_lba_plan_set_poses
 *                        makes the state valid: plslam_lba_plan_iterate_resident / _iterate_schur run with no landmark uploaded.
 *   first_estimate_slot  -1: the slots as given.  s >= 0 (s + nkf <= n_pose_slots): the slot of every POINT observation with
 *                        kf_loc >= 0 becomes s + kf_loc -- the current estimate of its keyframe (:1600-1601); line observations
 *                        and keyframes that are not optimised keep the given slot (:1680).  With the gather's *_pose_slot (the
 *                        keyframe index): n_pose_slots = n_map_kf + nkf, first_estimate_slot = n_map_kf.
 * PLSLAM_ERANGE: 2^30 observations, or (at the Schur lists' first use) 2^30 pairs with their padding. */
int plslam_lba_plan_create_dev(plslam_ctx* ctx, const plslam_cam* K, double homog_th, int32_t n_pose_slots, int32_t nkf,
                               int32_t npt, int32_t nls, const int32_t* d_pt_lm_loc, const int32_t* d_pt_pose_slot,
                               const int32_t* d_pt_kf_loc, const double* d_pt_obs_uv, int32_t n_pt_obs,
                               const int32_t* d_ls_lm_loc, const int32_t* d_ls_pose_slot, const int32_t* d_ls_kf_loc,
                               const double* d_ls_l_obs, int32_t n_ls_obs, const double* d_Xw, const double* d_Lw,
                               int32_t first_estimate_slot, plslam_lba_plan** out);
/* The lists of a plan of either kind, device -> host: a debugging aid (what the tests compare).  plslam_lba_plan_list_sizes
 * gives the lengths; prepare_schur != 0 builds the Schur pair lists first if no Schur call has yet (what the first
 * plslam_lba_plan_diag_max / _schur / _iterate_schur does).  plslam_lba_plan_lists: HOST pointers, NULL = skip.
 *   pt_ptr (npt + 1) / pt_ids (n_pt_obs), ls_ptr (nls + 1) / ls_ids (n_ls_obs), kf_ptr (nkf + 1) / kf_ids (n_kf_ids: points,
 *   then lines as n_pt_obs + o); the observation columns as the plan stores them (after the slot rewrite);
 *   blk_ptr (nblk + 1) and pairs (n_pairs x 4 int32: o1, o2, landmark, kind; kind 2 = a null pair of the padding): only after
 *   the Schur lists are built, PLSLAM_EINVAL before. */
typedef struct plslam_lba_list_sizes {
    int32_t nkf, npt, nls, n_pt_obs, n_ls_obs, n_kf_ids, max_chunks;
    int32_t schur_ready, nblk, n_pairs, schur_chunks;
} plslam_lba_list_sizes;
typedef struct plslam_lba_lists {
    int32_t *pt_ptr, *pt_ids, *ls_ptr, *ls_ids, *kf_ptr, *kf_ids;
    int32_t *pt_lm_loc, *pt_pose_slot, *pt_kf_loc;
    double* pt_obs_uv;
    int32_t *ls_lm_loc, *ls_pose_slot, *ls_kf_loc;
    double* ls_l_obs;
    int32_t *blk_ptr, *pairs;
} plslam_lba_lists;
int plslam_lba_plan_list_sizes(plslam_lba_plan* plan, int prepare_schur, plslam_lba_list_sizes* out);
int plslam_lba_plan_lists(plslam_lba_plan* plan, const plslam_lba_lists* host);

/* ---- K98-K104: the whole LM loop of levMarquardtOptimizationLBA (src/mapHandler.cpp:1334-1812) in one call (additive within 5) --
 * plslam_lba_plan_optimize_dev runs the loop that PLSLAM::LbaPlanSolver::optimizeResident (host/lba_rows.hpp) runs with two
 * synchronisations per iteration, on the device: the reduced system is solved there (L D L^T without pivoting, one workgroup),
 * the pose update x_k <- logmap(expmap(x_k) inverse(expmap(dp_k))) and the loop's decisions run there, and the loop's variables
 * live in a control block in device memory.  Every kernel of a pass returns at once when the loop has ended, so the call
 * enqueues passes without waiting and synchronises ONCE, at its end.
 *   plan          of either kind, its landmarks resident: plslam_lba_plan_create_dev with d_Xw / d_Lw, or any plan an earlier
 *                 plslam_lba_plan_iterate / _iterate_dev has filled; otherwise PLSLAM_EINVAL.  The landmarks stay in the plan:
 *                 plslam_local_map_apply_lba or plslam_lba_plan_get_landmarks take them from there.
 *   T_slots       n_pose_slots x 16 (host): the stored T_kf_w; the estimate slots first_estimate_slot + k must hold key frame k's
 *                 stored T_kf_w on entry -- the first pass reads the slots as given (:1369), expmap(x) appears from the first
 *                 update on (:1601)
 *   x_kf          nkf x 6 (host); x_kf_out: nkf x 6; T_out: nkf x 16 = expmap_se3(x_kf_out) (:1822-1826), may be NULL
 *   trace         max(max_iters_lba, 1) records, one per H / g build ([0] = the first pass), may be NULL
 * The loop's quirks are the reference's: the first err is divided by two counters that are never incremented (+inf, or NaN);
 * lambda0 = lambda_lba_lm * max |H(i,i)|; the first solve is always applied; later errs are divided by Npt + Nls; lambda GROWS on
 * an applied step; ||DX|| is taken over all N unknowns, for a rejected step too; err_prev = err after a rejected step too.
 * PLSLAM_EINVAL (nothing launched): a NULL plan, prm, T_slots, x_kf, x_kf_out or result; lambda_lba_k == 0; nkf < 1;
 * first_estimate_slot < 0 or first_estimate_slot + nkf > n_pose_slots.
 *   plslam_lba_reduced_ldlt_solve   the solve kernel alone: A (n x n, row-major, host; the lower triangle is read), b, x (n);
 *                 *n_bad_pivots (may be NULL) counts the pivots that are <= 0 or not finite.  n <= 120 runs on one workgroup with
 *                 A in LDS; larger systems go through the blocked L D L^T of plslam_dense_ldlt_solve on a padded copy. */
#define PLSLAM_LBA_STOP_MAX_ITERS 0   /* iters == max_iters_lba                                                              */
#define PLSLAM_LBA_STOP_ERR 1         /* |err - err_prev| < min_error_change || err < min_error (:1775)                       */
#define PLSLAM_LBA_STOP_DX 2          /* ||DX|| < min_error_change (:1808)                                                    */
#define PLSLAM_LBA_STOP_NOT_PD 3      /* a pivot of the reduced system was <= 0 or not finite: step NOT applied               */
typedef struct plslam_lba_lm_params {
    double lambda_lba_lm, lambda_lba_k;
    int32_t max_iters_lba, reserved;
    double min_error_change, min_error;
} plslam_lba_lm_params;
typedef struct plslam_lba_solve {      /* one per H / g build, [0] = the first pass */
    double lambda, err_raw, err, dx_norm;
    int32_t n_singular, n_bad_pivots;
    int32_t applied, reserved;         /* 1, 0, or -1: stopped before the solve */
} plslam_lba_solve;
typedef struct plslam_lba_result {
    int32_t iters, n_builds, stop_reason, n_enqueued_passes;
    double err, err_prev, lambda, hmax;
} plslam_lba_result;
int plslam_lba_plan_optimize_dev(plslam_lba_plan* plan, const plslam_lba_lm_params* prm, const double* T_slots, const double* x_kf,
                                 int32_t first_estimate_slot, double* x_kf_out, double* T_out, plslam_lba_solve* trace,
                                 plslam_lba_result* result);
int plslam_lba_reduced_ldlt_solve(plslam_ctx* ctx, int32_t n, const double* A, const double* b, double* x, int32_t* n_bad_pivots);

/* ---- K17: pose-only Gauss-Newton system of the loop-closure relative pose ------------------------------- */
/* The iteration body of MapHandler::computeRelativePoseGN (src/mapHandler.cpp:3324-3424) and of
 * computeRelativePoseRobustGN (:3588-3689; identical loops): per inlier point / line the reprojection error, the 6-vector
 * Jacobian wrt the pose increment (note: fx / max(homogTh, z^2) scales BOTH image coordinates, and the line rows use
 * l_obs(0..1) as multipliers -- unlike the local-BA rows) and the Cauchy weight, accumulated into
 *   H = H_p + H_l (6 x 6 row-major), g = g_p + g_l, *e = e_p + e_l (BEFORE the division by N_l + N_p of :3421),
 *   n_obs[0] = N_p, n_obs[1] = N_l (may be NULL).
 * T_inc: 16 doubles row-major; P npt x 3 (lc_points[i]->P), pl_obs npt x 2, pt_inlier npt bytes; sPeP nls x 6
 * (lc_lines[i]->sP, ->eP), le_obs nls x 3, ls_inlier nls bytes.  The solve (ColPivHouseholderQR of a 6 x 6, :3426-3428)
 * and the update T_inc = T_inc * inverse_se3(expmap_se3(x_inc)) stay with the caller. */
int plslam_pose_gn_accumulate(plslam_ctx* ctx, const plslam_cam* K, double homog_th, const double* T_inc,
                              const double* P, const double* pl_obs, const uint8_t* pt_inlier, int32_t npt,
                              const double* sPeP, const double* le_obs, const uint8_t* ls_inlier, int32_t nls,
                              double* H, double* g, double* e, int32_t* n_obs);

/* ---- K5/K6: map <-> keyframe geometric gates (the inlier masks) -------------------------- */
/* Points: src/mapHandler.cpp:601-613.  mask[i] = 1 iff matches_12[i] >= 0 and
 * || proj(Twf * Xw[i]) - pl[matches_12[i]] ||_2 < max_epip.  Twf: 16 doubles row-major.
 * Xw nq*3 (the matched map points, query order), pl nt*2.  *n_inliers = #mask (may be NULL). */
int plslam_map2kf_point_gate(plslam_ctx* ctx, const plslam_cam* K, const double* Twf,
                             const double* Xw, const int32_t* matches_12, int32_t nq,
                             const double* pl, int32_t nt, double max_epip, uint8_t* mask,
                             int32_t* n_inliers);
/* Lines: src/mapHandler.cpp:716-729 (signed test on both endpoints, no abs()).
 * Lw nq*6, le nt*3 (normalised 2D line equations). */
int plslam_map2kf_line_gate(plslam_ctx* ctx, const plslam_cam* K, const double* Twf,
                            const double* Lw, const int32_t* matches_12, int32_t nq,
                            const double* le, int32_t nt, double max_epip, uint8_t* mask,
                            int32_t* n_inliers);
/* Candidate pre-filter src/mapHandler.cpp:549-551 / :650-655: vis[i] = 1 iff the landmark
 * projects strictly inside the image with positive depth (both endpoints for lines). */
int plslam_map_point_visible(plslam_ctx* ctx, const plslam_cam* K, const double* Twf,
                             const double* Xw, int32_t n, uint8_t* vis);
int plslam_map_line_visible(plslam_ctx* ctx, const plslam_cam* K, const double* Twf,
                            const double* Lw, int32_t n, uint8_t* vis);

/* ---- the map <-> keyframe association drivers, fused ---------------------------------------- */
/* Replaces the compute of MapHandler::matchMap2KFPoints (src/mapHandler.cpp:532-632), brute-force
 * path (fast_matching == false); the map mutation (:614-626) stays with the caller.
 *   candidate[i] != 0  <=>  the reference's  pt != nullptr && pt->local && pt->kf_obs_list.back() != kf2_idx (:547)
 *   Xw n_map*3 = pt->point3D, med_desc n_map*32 = pt->med_desc (:555)
 *   kf_desc n_kf*32 = pdesc_l, kf_pl n_kf*2 = stereo_pt[i]->pl, kf_idx[i] = stereo_pt[i]->idx (-1 = unmatched, :565)
 *   min_matches = SlamConfig::minPointMatches() (:594-596), max_epip = SlamConfig::maxKFEpipP() (:613)
 * On the device: projection + inside-image test (:549-551), Q/T matrix construction (:555, :567),
 * StVO::match (:597), epipolar gate (:610-613).  map_to_kf[n_map] receives, per map landmark, the
 * ORIGINAL keyframe feature index it is associated with, or -1; *n_matches the return value. */
int plslam_map2kf_match_points(plslam_ctx* ctx, const plslam_cam* K, const double* Twf, const double* Xw,
                               const uint8_t* med_desc, const uint8_t* candidate, int32_t n_map,
                               const uint8_t* kf_desc, const double* kf_pl, const int32_t* kf_idx,
                               int32_t n_kf, float nnr, int mutual, double max_epip, int32_t min_matches,
                               int32_t* map_to_kf, int32_t* n_matches);
/* MapHandler::matchMap2KFLines (src/mapHandler.cpp:634-752): Lw n_map*6 = ls->line3D, kf_le n_kf*3 =
 * stereo_ls[i]->le; both endpoints must project inside (:654-655); signed gate (:727-729);
 * min_matches = SlamConfig::minLineMatches() (:709-711). */
int plslam_map2kf_match_lines(plslam_ctx* ctx, const plslam_cam* K, const double* Twf, const double* Lw,
                              const uint8_t* med_desc, const uint8_t* candidate, int32_t n_map,
                              const uint8_t* kf_desc, const double* kf_le, const int32_t* kf_idx,
                              int32_t n_kf, float nnr, int mutual, double max_epip, int32_t min_matches,
                              int32_t* map_to_kf, int32_t* n_matches);

/* The same drivers with SlamConfig::fastMatching() (`fast_matching: true`, the shipped configurations):
 * src/mapHandler.cpp:578-592 (points) / :681-707 (lines).  The candidates' projections become grid cells
 * (pj_points / pj_lines: pixels * inv_width / inv_height truncated to int) on the device, the unmatched
 * keyframe features fill the GridStructure (points: their cell, :581-584; lines: the Bresenham cells of
 * (spl, epl) and their directions, :686-698), StVO::matchGrid runs with a window of `ws` cells and the
 * ratio nnr_grid (Config::minRatio12P() for BOTH kinds); then, exactly as in the plain drivers,
 * StVO::match(nnr) replaces its result when |Q| > min_matches && matches < min_matches (:594-598,
 * :709-713).  *used_match (may be NULL) reports whether that happened.  fm == NULL or !fm->enabled is the
 * plain driver.  kf_seg: n_kf x 4 doubles = stereo_ls[i]->spl, ->epl (lines only).
 * PRECONDITION (as in the reference's getLineCoords): kf_seg holds PIXELS of the image.  The grid of the windowed matcher is
 * filled on the host by walking every Bresenham cell between the two end points times inv_width / inv_height, whether it lies
 * in the grid or not: a coordinate of 1e19 keeps the call busy for 2^31 cells.  Finite values of the image's size are expected;
 * the entry points do not clamp them. */
typedef struct plslam_fast_matching {
    int32_t enabled;              /* SlamConfig::fastMatching() */
    int32_t grid_cols, grid_rows; /* GRID_COLS (64), GRID_ROWS (48) */
    int32_t ws;                   /* SlamConfig::matchingF2FWs() */
    double inv_width, inv_height; /* StereoFrame::inv_width / inv_height (GRID_COLS / width, GRID_ROWS / height) */
    double nnr_grid;              /* Config::minRatio12P() */
    double line_sim_th;           /* Config::lineSimTh() */
} plslam_fast_matching;
int plslam_map2kf_match_points_fast(plslam_ctx* ctx, const plslam_cam* K, const double* Twf, const double* Xw,
                                    const uint8_t* med_desc, const uint8_t* candidate, int32_t n_map,
                                    const uint8_t* kf_desc, const double* kf_pl, const int32_t* kf_idx,
                                    int32_t n_kf, float nnr, int mutual, double max_epip, int32_t min_matches,
                                    const plslam_fast_matching* fm, int32_t* map_to_kf, int32_t* n_matches,
                                    int32_t* used_match);
int plslam_map2kf_match_lines_fast(plslam_ctx* ctx, const plslam_cam* K, const double* Twf, const double* Lw,
                                   const uint8_t* med_desc, const uint8_t* candidate, int32_t n_map,
                                   const uint8_t* kf_desc, const double* kf_le, const double* kf_seg,
                                   const int32_t* kf_idx, int32_t n_kf, float nnr, int mutual, double max_epip,
                                   int32_t min_matches, const plslam_fast_matching* fm, int32_t* map_to_kf,
                                   int32_t* n_matches, int32_t* used_match);
/* The same drivers with the MAP SIDE DEVICE-RESIDENT: d_Xw / d_Lw, d_med_desc and d_candidate are device pointers (8-byte
 * aligned) -- a local map lives on the GPU across keyframes (the representative descriptors come from
 * plslam_median_desc_batched_dev, the landmarks from the LBA plan); the host-pointer forms above stage and upload 0.56 MB of
 * it per call at C3 sizes (10 000 landmarks), which is a quarter of their time.  The keyframe side (kf_*), the results and the
 * semantics are those of the _fast forms (fm == NULL or !fm->enabled: the plain driver).  kf_seg: lines only. */
int plslam_map2kf_match_points_dev(plslam_ctx* ctx, const plslam_cam* K, const double* Twf, const double* d_Xw,
                                   const uint8_t* d_med_desc, const uint8_t* d_candidate, int32_t n_map,
                                   const uint8_t* kf_desc, const double* kf_pl, const int32_t* kf_idx, int32_t n_kf,
                                   float nnr, int mutual, double max_epip, int32_t min_matches,
                                   const plslam_fast_matching* fm, int32_t* map_to_kf, int32_t* n_matches,
                                   int32_t* used_match);
int plslam_map2kf_match_lines_dev(plslam_ctx* ctx, const plslam_cam* K, const double* Twf, const double* d_Lw,
                                  const uint8_t* d_med_desc, const uint8_t* d_candidate, int32_t n_map,
                                  const uint8_t* kf_desc, const double* kf_le, const double* kf_seg,
                                  const int32_t* kf_idx, int32_t n_kf, float nnr, int mutual, double max_epip,
                                  int32_t min_matches, const plslam_fast_matching* fm, int32_t* map_to_kf,
                                  int32_t* n_matches, int32_t* used_match);


/* ---- the keyframe <-> keyframe association drivers ------------------------------------------------ */
/* Replace the compute of MapHandler::matchKF2KFPoints (src/mapHandler.cpp:234-363; :246-278) and matchKF2KFLines
 * (:365-530; :378-426); creating the MapPoints / MapLines from matches_12 (:280-363, :428-530) stays with the caller.
 *   fm enabled: the previous keyframe's stereo features are projected with DT (16 doubles row-major; :254-256,
 *     :384-394) on the device, the current keyframe's features fill the GridStructure (:259-263 / :397-411), window of
 *     matching_f2f_ws cells, StVO::matchGrid.  Points: pj_points = projection * inv_width / inv_height.  Lines: pj_lines
 *     are the projected PIXELS -- upstream does not multiply them by inv_width (:392-393) -- truncated to int like
 *     everything that goes into a point_2d; a projection that is not a finite int32 becomes INT_MIN (x86 cvttsd2si).
 *   then StVO::match(prev, curr, nnr) iff n_curr > min_matches && n_prev > min_matches && matches < min_matches
 *     (:274-278, :421-425).
 * P_prev n_prev x 3 (stereo_pt[i]->P) / sPeP_prev n_prev x 6 (stereo_ls[i]->sP, ->eP); pl_curr n_curr x 2 /
 * seg_curr n_curr x 4 (spl, epl).  matches_12: n_prev entries (all -1 when no matcher ran). */
int plslam_kf2kf_match_points(plslam_ctx* ctx, const plslam_cam* K, const double* DT, const double* P_prev,
                              const uint8_t* desc_prev, int32_t n_prev, const double* pl_curr,
                              const uint8_t* desc_curr, int32_t n_curr, float nnr, int mutual, int32_t min_matches,
                              const plslam_fast_matching* fm, int32_t* matches_12, int32_t* n_matches,
                              int32_t* used_match);
int plslam_kf2kf_match_lines(plslam_ctx* ctx, const plslam_cam* K, const double* DT, const double* sPeP_prev,
                             const uint8_t* desc_prev, int32_t n_prev, const double* seg_curr,
                             const uint8_t* desc_curr, int32_t n_curr, float nnr, int mutual, int32_t min_matches,
                             const plslam_fast_matching* fm, int32_t* matches_12, int32_t* n_matches,
                             int32_t* used_match);
/* The same with the ROWS ON THE DEVICE: d_P_prev / d_sPeP_prev (n_prev x 3 | 6 doubles), d_desc_prev and d_desc_curr (x 32
 * bytes, 16-byte aligned) are device pointers -- a keyframe's descriptors and 3D features stay on the GPU from one call to
 * the next (they are the rows the stereo and frame-to-frame plans already hold); nothing is staged or uploaded but the grid
 * the host builds from pl_curr / seg_curr (HOST pointers, as above).  Results and semantics are those of the forms above. */
int plslam_kf2kf_match_points_dev(plslam_ctx* ctx, const plslam_cam* K, const double* DT, const double* d_P_prev,
                                  const uint8_t* d_desc_prev, int32_t n_prev, const double* pl_curr,
                                  const uint8_t* d_desc_curr, int32_t n_curr, float nnr, int mutual,
                                  int32_t min_matches, const plslam_fast_matching* fm, int32_t* matches_12,
                                  int32_t* n_matches, int32_t* used_match);
int plslam_kf2kf_match_lines_dev(plslam_ctx* ctx, const plslam_cam* K, const double* DT, const double* d_sPeP_prev,
                                 const uint8_t* d_desc_prev, int32_t n_prev, const double* seg_curr,
                                 const uint8_t* d_desc_curr, int32_t n_curr, float nnr, int mutual,
                                 int32_t min_matches, const plslam_fast_matching* fm, int32_t* matches_12,
                                 int32_t* n_matches, int32_t* used_match);

/* ---- representative ("median") descriptor of every landmark, batched ------------------------ */
/* Replaces the descriptor part of MapPoint::updateAverageDescDir (src/mapFeatures.cpp:51-84) and of
 * MapLine::updateAverageDescDir (:121-157), which the reference runs per landmark whenever an
 * observation is added (:47, :118): per landmark, the observation whose row of the pairwise
 * Hamming matrix has the smallest element int(1+0.5*(n-1)) after sorting (:77), first row winning
 * ties (strict '<' :78).  All landmarks in one call, observation lists concatenated:
 *   desc_lists  total x 32 uint8  landmark l owns rows offsets[l] .. offsets[l+1]-1 (desc_list order)
 *   offsets     n_lm+1 int32, offsets[0] = 0, non-decreasing; every list shorter than 2^23 rows
 *   med_idx     n_lm int32: winner's position within its own list (0 for a single observation --
 *               the constructors :28-38 -- and -1 for an empty list, which the reference never has)
 *   med_desc    n_lm x 32 uint8 = desc_list[med_idx] (zeros for an empty list); may be NULL.  These
 *               rows are the `med_desc` argument of plslam_map2kf_match_points/_lines.
 * The direction average (:86-91) accumulates into an uninitialised vector upstream and is not
 * reproduced.  The _dev form takes device pointers (4-byte aligned) plus the total row count and
 * enqueues on `stream` (NULL = the context's stream) without synchronising. */
int plslam_median_desc_batched(plslam_ctx* ctx, const uint8_t* desc_lists, const int32_t* offsets,
                               int32_t n_lm, int32_t* med_idx, uint8_t* med_desc);
int plslam_median_desc_batched_dev(plslam_ctx* ctx, const uint8_t* desc_lists, const int32_t* offsets,
                                   int32_t n_lm, int32_t total, int32_t* med_idx, uint8_t* med_desc,
                                   void* stream);

/* ---- K18: the LBD float descriptor of a line (producer of the 72 floats K11 binarises) -------------------- */
/* Replaces BinaryDescriptor::computeLBD, 3rdparty/line_descriptor/src/binary_descriptor_custom.cpp:1026-1372, for the
 * lines of ONE octave: gradient images dx / dy (int16, width x height, row stride = width: dxImg_vector[octave] /
 * dyImg_vector[octave], :1095-1101) and, per line, the OctaveSingleLine fields the function reads (numOfPixels,
 * sPointInOctaveX/Y, ePointInOctaveX/Y, direction).  width_of_band = params.widthOfBand_ (7; 1..7 supported),
 * NUM_OF_BANDS = 9.  lbd_f32: n x 72 float32 = the lines' `descriptor` vectors -- the input of
 * plslam_lbd_binarise.  fp32 with the source's sequential summation order and no FMA; the weight tables and
 * cos / sin(direction) are evaluated on the host with libm as upstream does.
 * _dev form: dx_img / dy_img / lbd_f32 are DEVICE pointers (the line records stay host data: they are the line
 * detector's small output); enqueues on `stream` (NULL = the context's stream). */
typedef struct plslam_lbd_line {
    int32_t num_pixels;
    float sx, sy, ex, ey;
    float direction;
} plslam_lbd_line;
int plslam_lbd_compute(plslam_ctx* ctx, const int16_t* dx_img, const int16_t* dy_img, int32_t width, int32_t height,
                       const plslam_lbd_line* lines, int32_t n, int32_t width_of_band, float* lbd_f32);
int plslam_lbd_compute_dev(plslam_ctx* ctx, const int16_t* dx_img, const int16_t* dy_img, int32_t width,
                           int32_t height, const plslam_lbd_line* lines_host, int32_t n, int32_t width_of_band,
                           float* lbd_f32, void* stream);

/* ---- LBD float -> 256-bit binary line descriptor (producer of the matcher's LBD rows) ----- */
/* Replaces the "fill current row with binary descriptor" loop of BinaryDescriptor::computeImpl,
 * 3rdparty/line_descriptor/src/binary_descriptor_custom.cpp:653-668, with
 * binaryConversion (:401-412: bit i of a byte set iff f1[i] > f2[i]) over the 32 band pairs of
 * combinations[32][2] (:74-107); NUM_OF_BANDS 9 (:57) x 8 floats = 72 floats per line.
 *   lbd_f32  n x 72 float32, row-major contiguous (the ScaleLines' `descriptor` vectors, packed)
 *   desc_u8  n x 32 uint8: the cv::Mat(n,32,CV_8UC1) rows StVO::match consumes for lines
 * Comparisons with a NaN operand leave the bit clear, as in the reference.  The _dev form takes
 * device pointers (both 16-byte aligned) and enqueues on `stream`
 * (NULL = the context's stream) without synchronising. */
#define PLSLAM_LBD_FLOATS 72
int plslam_lbd_binarise(plslam_ctx* ctx, const float* lbd_f32, int32_t n, uint8_t* desc_u8);
int plslam_lbd_binarise_dev(plslam_ctx* ctx, const float* lbd_f32, int32_t n, uint8_t* desc_u8,
                            void* stream);

/* ---- multi-GPU: gather of per-frame match tables over RCCL/xGMI -------------------------- */
/* No reference counterpart (the reference is single-process).  `comm` is an ncclComm_t the
 * host created (one rank per GPU); `local` is this rank's n_local int32 match-table entries
 * (device); `gathered` (device, root only) receives nranks*n_local entries in rank order.
 * Implemented as one ncclGroup of point-to-point sends to root so each peer uses its own
 * xGMI link.  RCCL is loaded lazily (dlopen); returns PLSLAM_ENOTSUP if it cannot be. */
int plslam_gather_match_tables(plslam_ctx* ctx, void* comm, int nranks, int rank, int root,
                               const int32_t* local, int64_t n_local, int32_t* gathered,
                               void* stream);

/* Which librccl the host's communicators come from (call before the first gather; NULL = the default search: librccl.so,
 * librccl.so.1, /opt/rocm/lib/librccl.so).  A communicator belongs to ONE loaded copy of the library -- PyTorch ships its own
 * beside ROCm's -- and the send / receive entry points must be that copy's. */
int plslam_rccl_use(const char* path);
/* 1 when librccl's group / send / recv entry points could be loaded (the first call loads them), 0 otherwise: asked before the
 * first plslam_match_plan_step_gather, so that a missing library is a set-up failure and the caller can keep its own gather. */
int plslam_rccl_available(void);

/* One step of the N > 1 path in one call (ABI v5): the plan's scan on scan_stream, everything behind it on post_stream
 * (plslam_match_plan_run_split), then the gather of the finished table to `root` -- one ncclGroup of point-to-point transfers,
 * each peer on its own xGMI link -- and, on the root with the int16 wire format, the widening to int32; all enqueued, nothing
 * waited for on the host.  The next step of the SAME plan orders itself behind this gather (both streams) before anything
 * rewrites the table; plslam_match_plan_gather_sync waits for it on the host.
 *   wire_bytes 4: `send` = the plan's int32 match table itself (n_entries entries), `recv` (root) = nranks * n_entries int32 in
 *                 rank order -- the gathered tables of the C ABI; `wide` unused
 *   wire_bytes 2: `send` = the int16 mirror the finalize kernel writes (plslam_match_plan_set_wire16), `recv` (root) = nranks *
 *                 n_entries int16, `wide` (root; may be NULL) = nranks * n_entries int32, written behind the gather
 *   comm_stream   the stream the collective (and the widening) is enqueued on; NULL = post_stream
 * nranks == 1: no communicator needed (the root's own slice is copied / widened). */
typedef struct plslam_gather_step {
    void* comm;                  /* ncclComm_t of this rank */
    int32_t nranks, rank, root;
    int32_t wire_bytes;
    const void* send;
    int64_t n_entries;
    void* recv;
    int32_t* wide;
    void *scan_stream, *post_stream, *comm_stream;
} plslam_gather_step;
int plslam_match_plan_step_gather(plslam_match_plan* plan, const plslam_gather_step* step);
int plslam_match_plan_gather_sync(plslam_match_plan* plan);

/* ---- Bag of words: DBoW2 vocabulary transform and the keyframe confusion matrix (bow.hip, bow_plan.hpp) --------------------
 * Replaces the bag-of-words step of MapHandler::addKeyFrame (src/mapHandler.cpp:196-201 -> insertKFBowVector{P,L,PL},
 * :3007-3128): TemplatedVocabulary<FORB>::transform (3rdparty/DBoW2/include/DBoW2/TemplatedVocabulary.h:1046-1100,
 * :1198-1240) and L1Scoring::score (src/DBoW2/ScoringObject.cpp:23-67) against every earlier keyframe.
 * Results are bit-identical to the reference's double arithmetic (fixed fold orders, DESIGN.md section "Bag of words"). */

/* DBoW2's enums (3rdparty/DBoW2/include/DBoW2/BowVector.h:29-55) */
enum { PLSLAM_BOW_TF_IDF = 0, PLSLAM_BOW_TF = 1, PLSLAM_BOW_IDF = 2, PLSLAM_BOW_BINARY = 3 };
enum { PLSLAM_BOW_L1_NORM = 0 };   /* the only scoring supported; the others get PLSLAM_ENOTSUP */
/* largest descriptor set of one transform / one modality of one keyframe (PLSLAM_ERANGE beyond it) */
#define PLSLAM_BOW_MAX_SET 16384

/* the records of TemplatedVocabulary::load (TemplatedVocabulary.h:1437-1485), in FILE order */
typedef struct plslam_bow_node {
    int32_t node_id, parent_id;     /* 1..n_nodes, 0..n_nodes (0 = the root, which has no record) */
    double weight;
    uint8_t descriptor[32];         /* FORB::fromString's 32 bytes */
} plslam_bow_node;
typedef struct plslam_bow_word {
    int32_t word_id, node_id;       /* 0..n_words-1, 1..n_nodes */
} plslam_bow_word;
typedef struct plslam_bow_vocab_desc {
    int32_t k, L, scoring_type, weighting_type;
    int32_t n_nodes, n_words;
    const plslam_bow_node* nodes;
    const plslam_bow_word* words;
} plslam_bow_vocab_desc;
typedef struct plslam_bow_vocab plslam_bow_vocab;

/* Copies the vocabulary to the device.  Children keep the order in which their records appear (load()'s push_back): the
 * descent keeps the FIRST child of that list on a distance tie.  PLSLAM_EINVAL (with plslam_last_error()) for ids out of
 * range, a duplicate node or word id, a parent that is not a node, a cycle, a leaf without a word, an empty vocabulary;
 * PLSLAM_ENOTSUP for a scoring other than PLSLAM_BOW_L1_NORM.  The vocabulary belongs to ctx and must be destroyed first. */
int plslam_bow_vocab_create(plslam_ctx* ctx, const plslam_bow_vocab_desc* desc, plslam_bow_vocab** out);
void plslam_bow_vocab_destroy(plslam_bow_vocab* voc);

/* TemplatedVocabulary::transform of `nsets` descriptor sets (set s = rows offsets[s] .. offsets[s+1]-1 of desc, every set at
 * most PLSLAM_BOW_MAX_SET rows, else PLSLAM_ERANGE).  Per descriptor: word_id / word_weight of the leaf it descends to (stopped
 * words included).  Per set: the BowVector after normalize(L1) as ascending word ids and weights at bow_word / bow_weight
 * + offsets[s], bow_len[s] entries.  Any output pointer but bow_len may be NULL. */
int plslam_bow_transform(plslam_bow_vocab* voc, const uint8_t* desc, const int32_t* offsets, int32_t nsets,
                         int32_t* word_id, double* word_weight, int32_t* bow_word, double* bow_weight, int32_t* bow_len);
/* Device pointers, enqueued on `stream` (NULL = the context's stream), no synchronisation.  total = offsets[nsets] and
 * max_set (>= every set's size, <= PLSLAM_BOW_MAX_SET) come from the caller; a set longer than max_set gets bow_len = -1.
 * word_weight may be NULL; the other outputs are required (total / total / total / nsets entries).  desc 16-byte aligned. */
int plslam_bow_transform_dev(plslam_bow_vocab* voc, const uint8_t* desc, const int32_t* offsets, int32_t nsets, int32_t total,
                             int32_t max_set, int32_t* word_id, double* word_weight, int32_t* bow_word, double* bow_weight,
                             int32_t* bow_len, void* stream);

/* the per-keyframe inputs of insertKFBowVectorPL's combination (src/mapHandler.cpp:3063-3098): vector_stdv lives in stvo-pl,
 * so the caller computes std_pt / std_ls */
typedef struct plslam_bow_pl_stats {
    int32_t n_pt, n_ls;
    double std_pt, std_ls;
} plslam_bow_pl_stats;
typedef struct plslam_bow_db plslam_bow_db;

/* The keyframe BowVectors on the device.  vocab_p / vocab_l: either may be NULL, which selects insertKFBowVectorL / P; both
 * set = insertKFBowVectorPL (src/mapHandler.cpp:196-201).  capacity_hint: keyframes to reserve for (grows by itself). */
int plslam_bow_db_create(plslam_ctx* ctx, plslam_bow_vocab* vocab_p, plslam_bow_vocab* vocab_l, int32_t capacity_hint,
                         plslam_bow_db** out);
void plslam_bow_db_destroy(plslam_bow_db* db);
/* insertKFBowVector{P,L,PL}(kf) for kf_idx: transforms the keyframe's left descriptors, stores the vectors, and writes
 * conf_row[i] = score(new, i) for every i < kf_idx with alive[i] != 0 (= map_keyframes[i] != NULL; each such i must have been
 * inserted), and conf_row[kf_idx] = score(new, new).  Other entries are left untouched.  The inputs of an absent modality are
 * ignored; stats is read in PL mode only.  One launch sequence (3 kernels) and one synchronisation. */
int plslam_bow_db_insert(plslam_bow_db* db, int32_t kf_idx, const uint8_t* pdesc, int32_t n_pdesc, const uint8_t* ldesc,
                         int32_t n_ldesc, const plslam_bow_pl_stats* stats, const uint8_t* alive, double* conf_row);
/* Device pointers for pdesc / ldesc / alive / conf_row (kf_idx + 1 entries each); stats is a host struct.  Enqueued on the
 * context's stream, no synchronisation; an alive entry that was never inserted is left untouched. */
int plslam_bow_db_insert_dev(plslam_bow_db* db, int32_t kf_idx, const uint8_t* pdesc, int32_t n_pdesc, const uint8_t* ldesc,
                             int32_t n_ldesc, const plslam_bow_pl_stats* stats, const uint8_t* alive, double* conf_row);
/* *n = 1 + the largest keyframe index inserted (0 when empty) */
int plslam_bow_db_size(plslam_bow_db* db, int32_t* n);
/* Throughput form: out[q * n + i] (n = plslam_bow_db_size) = the value plslam_bow_db_insert would have written at i with
 * queries[q] as the new keyframe (its stored PL stats), for every stored keyframe i; NaN where i was never inserted.
 * Every query must have been inserted. */
int plslam_bow_db_score(plslam_bow_db* db, const int32_t* queries, int32_t nq, double* out);

/* ---- K25: loop-closure verification (MapHandler::isLoopClosure + computeRelativePoseRobustGN) ------------------------ */
/* src/mapHandler.cpp:3192-3300 and :3566-3957 in one call: the two StVO::match problems between the keyframes' left
 * descriptors, the correspondences in i1 order, the inlier-ratio gate, the two-stage robust pose-only Gauss-Newton (the
 * 6 x 6 solve restates Eigen's ColPivHouseholderQR), the outlier pass, and the five-way decision.  See DESIGN.md,
 * "Loop-closure verification", for every reference quirk kept. */
#define PLSLAM_LC_MAX_FEATURES 16384      /* per kind and keyframe (n_pt, n_ls); larger -> PLSLAM_ERANGE */
#define PLSLAM_LC_MAX_ITERS 10000         /* max_iters and max_iters_ref each; larger or negative -> PLSLAM_EINVAL */

typedef struct plslam_lc_params {
    plslam_cam cam;                 /* the stereo camera (MapHandler::cam; fx, fy, cx, cy are read)                 */
    double homog_th;                /* stvo Config::homogTh()                                                      */
    float min_ratio_12_p;           /* SlamConfig::minRatio12P()                                                   */
    float min_ratio_12_l;           /* SlamConfig::minRatio12L()                                                   */
    int32_t mutual;                 /* stvo Config::bestLRMatches() (StVO::match's cross check)                     */
    int32_t has_points, has_lines;  /* SlamConfig::hasPoints() / hasLines()                                        */
    int32_t max_iters;              /* SlamConfig::maxIters()     (stage 1)                                        */
    int32_t max_iters_ref;          /* SlamConfig::maxItersRef()  (stage 2)                                        */
    int32_t reserved;
    double lc_inlier_ratio;         /* SlamConfig::lcInlierRatio() (percent)                                       */
    double lc_res;                  /* SlamConfig::lcRes()                                                         */
    double lc_unc;                  /* SlamConfig::lcUnc()                                                         */
    double lc_inl;                  /* SlamConfig::lcInl()  (computed and reported; the decision ignores it, :3903) */
    double lc_trs;                  /* SlamConfig::lcTrs()                                                         */
    double lc_rot;                  /* SlamConfig::lcRot()  (degrees)                                              */
} plslam_lc_params;

/* one keyframe's stereo features (kf->stereo_frame): row i of every array is stereo_pt[i] / stereo_ls[i] */
typedef struct plslam_lc_keyframe {
    const uint8_t* pdesc;           /* n_pt x 32: pdesc_l                                      */
    const double* P;                /* n_pt x 3:  stereo_pt[i]->P                              */
    const double* pl;               /* n_pt x 2:  stereo_pt[i]->pl                             */
    const int32_t* pt_idx;          /* n_pt:      stereo_pt[i]->idx (-1 allowed); NULL = all -1 */
    int32_t n_pt;
    int32_t n_ls;
    const uint8_t* ldesc;           /* n_ls x 32: ldesc_l                                      */
    const double* sPeP;             /* n_ls x 6:  stereo_ls[i]->sP, ->eP                       */
    const double* le;               /* n_ls x 3:  stereo_ls[i]->le                             */
    const int32_t* ls_idx;          /* n_ls:      stereo_ls[i]->idx; NULL = all -1             */
} plslam_lc_keyframe;

typedef struct plslam_lc_result {
    int32_t is_lc;                  /* isLoopClosure's return value                                             */
    int32_t gn_ran;                 /* the inlier-ratio gate passed and computeRelativePoseRobustGN ran         */
    int32_t common_pt, common_ls;   /* match() counts = correspondences (rows of pt_corr / ls_corr)             */
    int32_t n_pt_inliers, n_ls_inliers;   /* inlier flags after the outlier pass                                */
    int32_t iters_1, iters_2;       /* systems assembled in stage 1 / stage 2                                   */
    int32_t ok_res, ok_unc, ok_inl, ok_trs, ok_rot;   /* the five tests (ok_inl as computed, before :3903)     */
    int32_t reserved;
    double inl_ratio_pt, inl_ratio_ls;   /* :3273-3274 (NaN where a keyframe has no features of the kind)       */
    double e;                       /* the last assembled system's normalised error                             */
    double cov_eig;                 /* largest eigenvalue of H^-1                                               */
    double ratio_inliers, t, r;
    double x_inc[6];                /* logmap_se3(T_inc)                                                        */
    double T_inc[16];               /* row-major                                                                */
    double pose_inc[6];             /* logmap_se3(inverse_se3(expmap_se3(x_inc))) when is_lc, else 0            */
    double H[36], g[6];             /* the last assembled system (row-major H)                                  */
    int64_t clk_total, clk_serial;  /* diagnostics: K25's time, and its one-lane part (solve, update, decision),
                                       in ticks of the 100 MHz wall clock                                       */
} plslam_lc_result;

/* Host pointers, one synchronisation.  pt_corr: kf0.n_pt x 4 capacity; row k (k < common_pt) = (kf0.pt_idx[i1], i1,
 * kf1.pt_idx[i2], i2) for the k-th match in i1 order (lc_pt_idx before the decision); pt_inlier[k] = its flag after the
 * outlier pass.  ls_corr / ls_inlier likewise with kf0.n_ls rows.  The reference's outputs are: lc_pt_idx = rows with
 * pt_inlier set if is_lc, all common_pt rows otherwise (and likewise for lines).  Any of the four may be NULL.
 * EINVAL: NULL inputs, negative sizes, max_iters / max_iters_ref outside [0, PLSLAM_LC_MAX_ITERS];
 * ERANGE: a feature count over PLSLAM_LC_MAX_FEATURES. */
int plslam_loop_closure_verify(plslam_ctx* ctx, const plslam_lc_params* params, const plslam_lc_keyframe* kf0,
                               const plslam_lc_keyframe* kf1, plslam_lc_result* result, int32_t* pt_corr, uint8_t* pt_inlier,
                               int32_t* ls_corr, uint8_t* ls_inlier);
/* Device pointers throughout (the keyframe arrays, result, and the four outputs, which must not be NULL where the kind has
 * rows); params and the two keyframe records are host structs.  Enqueued behind `stream` (NULL = the context's stream),
 * no synchronisation; the result is in device memory when `stream` reaches this point. */
int plslam_loop_closure_verify_dev(plslam_ctx* ctx, const plslam_lc_params* params, const plslam_lc_keyframe* kf0,
                                   const plslam_lc_keyframe* kf1, plslam_lc_result* result, int32_t* pt_corr,
                                   uint8_t* pt_inlier, int32_t* ls_corr, uint8_t* ls_inlier, void* stream);
/* computeRelativePoseRobustGN (:3566-3957) alone on the caller's correspondences (lc_points / lc_lines, all inlier on
 * entry): P npt x 3, pl_obs npt x 2, sPeP nls x 6, le_obs nls x 3.  Host pointers, one synchronisation; the params' match
 * and gate fields are ignored.  common_pt / common_ls = npt / nls; inl_ratio_* are 0; pt_inlier / ls_inlier may be NULL. */
int plslam_relpose_robust_gn(plslam_ctx* ctx, const plslam_lc_params* params, const double* P, const double* pl_obs,
                             int32_t npt, const double* sPeP, const double* le_obs, int32_t nls, plslam_lc_result* result,
                             uint8_t* pt_inlier, uint8_t* ls_inlier);

/* ---- K54: the same check for B candidate pairs in one call --------------------------------------------------------------
 * One match plan of up to 2 B problems (per pair exactly the problems of the single call; kept while the batch's problem list
 * -- shapes and addresses -- stays the same) and ONE launch of B workgroups, each running the single call's per-problem code:
 * results[b], pair b's rows and masks are those of plslam_loop_closure_verify[_dev](kf0[b], kf1[b]) bit for bit (clk_* apart).
 * kf0 / kf1: B host records each; records (and device arrays) may repeat across pairs -- every pair of a top-K verification
 * has the same kf1.  Pair b's rows of pt_corr / pt_inlier start at row sum_{b' < b} kf0[b'].n_pt, of ls_corr / ls_inlier at
 * row sum_{b' < b} kf0[b'].n_ls.  The params are fixed at creation.  Every buffer belongs to the batch object and only grows.
 * EINVAL / ERANGE per pair as for the single call; B < 0 or B > max_pairs: EINVAL; B == 0: OK, nothing is launched.  A failed
 * call leaves the object usable.  Calls on one context are serialised. */
#define PLSLAM_LC_MAX_BATCH 65536         /* max_pairs, and B of plslam_relpose_robust_gn_batched_dev; larger -> PLSLAM_ERANGE */
typedef struct plslam_lc_batch plslam_lc_batch;
int plslam_lc_batch_create(plslam_ctx* ctx, const plslam_lc_params* params, int32_t max_pairs, plslam_lc_batch** out);
void plslam_lc_batch_destroy(plslam_lc_batch* batch);
/* Device pointers throughout (the keyframe arrays, results -- B records --, and the four outputs, which must not be NULL
 * where some kf0 has rows of the kind); the records are host structs.  Enqueued behind `stream` (NULL = the context's
 * stream), no synchronisation. */
int plslam_lc_batch_verify_dev(plslam_lc_batch* batch, const plslam_lc_keyframe* kf0, const plslam_lc_keyframe* kf1, int32_t B,
                               plslam_lc_result* results, int32_t* pt_corr, uint8_t* pt_inlier, int32_t* ls_corr,
                               uint8_t* ls_inlier, void* stream);
/* Host pointers: one upload image (a repeated record is uploaded once), one download, one synchronisation.  Any of the four
 * outputs may be NULL. */
int plslam_lc_batch_verify(plslam_lc_batch* batch, const plslam_lc_keyframe* kf0, const plslam_lc_keyframe* kf1, int32_t B,
                           plslam_lc_result* results, int32_t* pt_corr, uint8_t* pt_inlier, int32_t* ls_corr, uint8_t* ls_inlier);
/* computeRelativePoseRobustGN alone for B problems on the caller's correspondences, device pointers, enqueued behind `stream`
 * without a synchronisation.  The arrays are concatenated: problem b owns rows [pt_off[b], pt_off[b + 1]) of P, pl_obs and
 * pt_inlier and rows [ls_off[b], ls_off[b + 1]) of sPeP, le_obs and ls_inlier; pt_off / ls_off are B + 1 non-decreasing int32
 * in DEVICE memory (a producer on the device can write them), each problem at most PLSLAM_LC_MAX_FEATURES rows per kind (a
 * count outside that range is taken as 0).  A kind without rows anywhere passes NULL arrays.  results[b] is what
 * plslam_relpose_robust_gn returns for problem b, bit for bit (clk_* apart). */
int plslam_relpose_robust_gn_batched_dev(plslam_ctx* ctx, const plslam_lc_params* params, const double* P, const double* pl_obs,
                                         const int32_t* pt_off, const double* sPeP, const double* le_obs, const int32_t* ls_off,
                                         int32_t B, plslam_lc_result* results, uint8_t* pt_inlier, uint8_t* ls_inlier, void* stream);

/* ---- K26-K39: global bundle adjustment (MapHandler::globalBundleAdjustment + levMarquardtOptimizationGBA,
 * src/mapHandler.cpp:1995-2099, :2101-2703) ---------------------------------------------------------------------------
 * The rows and blocks of every pass are the LBA plan's: the first pass reads the stored T_kf_w of every keyframe (:2136,
 * :2246) and writes the pose x line cross blocks transposed in both triangles (:2349-2350, PLSLAM_LBA_COMPAT_GBA); every
 * later pass gives the points of an optimised keyframe expmap_se3(X) (:2411-2416) but the lines the STORED T_kf_w and both
 * end points from one stride-3 block (:2520-2523, PLSLAM_LBA_COMPAT_ITER_PASS), and writes the correct block J_l J_p^T into
 * the lower triangle, the only one SimplicialLDLT reads (:2628-2629).  The LBA text spells the iteration pass's homogTh as the
 * literal 1e-7 where the GBA reads SlamConfig::homogTh(): the plan refuses any other homog_th (PLSLAM_EINVAL).
 * The solve is the Schur complement on the covisible keyframe blocks plus a dense fp64 L D L^T of the 6 nkf x 6 nkf reduced
 * camera system on the device.  A landmark block that is not positive definite after damping contributes nothing and gets a
 * zero step (counted: n_singular) where the reference's full-system SimplicialLDLT would carry non-finite values; pivots of
 * the reduced system that are zero or not finite are counted (n_bad_pivots), not repaired.
 *   plslam_gba_plan_create  n_map_kf keyframe slots (map indices), nkf optimised keyframes (kf_list[k] = map index of local
 *                           keyframe k: every non-null keyframe but kf_idx 0, :2001-2013), npt / nls landmarks, and the
 *                           observation lists as the reference builds them (:2017-2092): pt_obs / ls_obs are Vector6i rows
 *                           (landmark map index, landmark local index, observation index, keyframe map index, keyframe local
 *                           index or -1, inlier flag), pt_obs_uv n x 2 / ls_l_obs n x 3 the observations themselves.
 *                           EINVAL: nkf above PLSLAM_GBA_MAX_KEYFRAMES (S alone takes 4.8 GB there), homog_th != 1e-7,
 *                           indices out of range, sizes that overflow the plan's 32-bit element offsets.
 *   plslam_gba_optimize     the LM loop (:2101-2672): lambda = lambda_lba_lm * trunc(max |H(i,i)|) (`int Hmax`, :2359), the
 *                           first solve always applied, then up to max_iters_lba - 1 passes with the reference's tests.  Its err
 *                           is divided by Npt_obs + Nls_obs, which are never incremented (:2121, :2230): +inf (NaN for a zero
 *                           sum) on every pass, so every step is taken and lambda grows by lambda_lba_k after each solve; the
 *                           stops are numeric_limits<double>::epsilon() (:2637, :2667).  In: the stored T_kf_w (n_map_kf x 16),
 *                           x_kf (nkf x 6, the keyframes' x_kf_w), Xw (npt x 3), Lw (nls x 6).  Out: x_kf_out (nkf x 6),
 *                           T_out (nkf x 16, expmap_se3 of x_kf_out: what the write-back stores, :2674-2680; may be NULL),
 *                           Xw_out, Lw_out.  trace (may be NULL) receives one record per solve: max(max_iters_lba, 1) entries.
 *                           Per solve only the err and ||DX||^2 scalars cross to the host.
 *   plslam_dense_ldlt_solve the device L D L^T alone: A (n x n, row-major, host; its LOWER triangle is read), b, x (n);
 *                           *n_bad_pivots (may be NULL) counts zero / non-finite pivots. */
#define PLSLAM_GBA_MAX_KEYFRAMES 4096
#define PLSLAM_GBA_STOP_MAX_ITERS 0    /* the loop ran out (iters == max_iters_lba)                                  */
#define PLSLAM_GBA_STOP_ERR 1          /* abs(err - err_prev) < eps || err < eps, before the solve (:2637)            */
#define PLSLAM_GBA_STOP_DX 2           /* DX.norm() < eps, after the solve (:2667)                                    */
typedef struct plslam_gba_plan plslam_gba_plan;
typedef struct plslam_gba_solve {
    double lambda;                     /* the damping this solve used                                              */
    double err_raw, err;               /* the pass's sum of r^2 w, and err as the reference normalises it           */
    double dx_norm;                    /* ||DX|| over all N unknowns                                               */
    int32_t n_singular, n_bad_pivots;  /* landmark blocks not positive definite; zero / non-finite pivots of S      */
    int32_t accepted, reserved;        /* the step was applied (err <= err_prev, or the first solve)                */
} plslam_gba_solve;
typedef struct plslam_gba_result {
    int32_t iters;                     /* the reference's `iters` when the loop ends                                */
    int32_t n_solves, stop_reason, reserved;
    double err, err_prev, lambda;      /* the loop's variables when it ends                                         */
    double hmax;                       /* max |H(i,i)| of the first pass (before the truncation)                    */
} plslam_gba_result;
int plslam_gba_plan_create(plslam_ctx* ctx, const plslam_cam* K, double homog_th, int32_t n_map_kf, int32_t nkf,
                           const int32_t* kf_list, int32_t npt, int32_t nls, const int32_t* pt_obs, const double* pt_obs_uv,
                           int32_t n_pt_obs, const int32_t* ls_obs, const double* ls_l_obs, int32_t n_ls_obs,
                           plslam_gba_plan** out);
int plslam_gba_optimize(plslam_gba_plan* plan, double lambda_lba_lm, double lambda_lba_k, int32_t max_iters_lba,
                        const double* T_kf_w, const double* x_kf, const double* Xw, const double* Lw, double* x_kf_out,
                        double* T_out, double* Xw_out, double* Lw_out, plslam_gba_solve* trace, plslam_gba_result* result);
void plslam_gba_plan_destroy(plslam_gba_plan* plan);
/* The same plan built ON THE DEVICE from DEVICE columns (additive within 5; K89-K96, KERNELS.md): plslam_gba_plan_create's
 * signature with d_kf_list (nkf), d_pt_obs (n x 6), d_pt_obs_uv (n x 2), d_ls_obs (n x 6), d_ls_l_obs (n x 3) as device pointers
 * -- what plslam_local_map_form_all + plslam_local_map_gather leave in plslam_local_map_buffers (kf_list, pt_obs, pt_obs_uv, ls_obs,
 * ls_l_obs) -- read on the context's stream.  Every list gba_lists_build makes on the host -- the per-observation arrays, the four
 * CSR lists, the covisible blocks, their chunks of at most 64 pairs and the compact pair list -- is built on the device, equal
 * entry for entry (plslam_gba_plan_lists shows them); the inner LBA plan is plslam_lba_plan_create_dev with n_pose_slots =
 * n_map_kf + nkf and first_estimate_slot = n_map_kf.  The plan keeps no host copy of any list but kf_list (downloaded once).
 * The checks are the host call's, made on the device: a column out of range, kf_list[v4] != v3, a kf_list entry out of range give
 * PLSLAM_EINVAL and no plan, and no kernel follows a bad index.  Refused before anything is launched, as the host call refuses
 * them: nkf < 1, nkf > PLSLAM_GBA_MAX_KEYFRAMES, homog_th != 1e-7, NULL or negative arguments, the 32-bit size limits; also
 * n_map_kf < 1 and observations of a kind with no landmark (rows the host builder refuses one by one).
 * PLSLAM_ERANGE: 2^30 or more observation pairs (the look-back's sums are 30-bit words, as for the LBA plan's device-built lists;
 * the host builder's limit is INT32_MAX pairs, PLSLAM_EINVAL) -- refused after the count, before any pair is emitted.  36 x the
 * chunk count at or above INT32_MAX: PLSLAM_EINVAL like the host, refused when the chunk total is known (behind the emit, before
 * anything is carved from it).
 * Synchronisations: the inner LBA plan's one, plus TWO here (the pair total, from which the scratch is carved; the block and
 * chunk totals, from which the solve's buffers are).  The last layout kernel is enqueued behind the second one on the context's
 * stream, which every later call of the plan uses.  Every plslam_gba_* call works on the plan. */
int plslam_gba_plan_create_dev(plslam_ctx* ctx, const plslam_cam* K, double homog_th, int32_t n_map_kf, int32_t nkf,
                               const int32_t* d_kf_list, int32_t npt, int32_t nls, const int32_t* d_pt_obs,
                               const double* d_pt_obs_uv, int32_t n_pt_obs, const int32_t* d_ls_obs, const double* d_ls_l_obs,
                               int32_t n_ls_obs, plslam_gba_plan** out);
/* The lists of a plan of either kind, device -> host: a debugging aid (what the tests compare).  plslam_gba_plan_list_sizes gives
 * the lengths.  plslam_gba_plan_lists: HOST pointers, NULL = skip.
 *   blk (nblk x 4 int32: k1, k2, c0, c1), chk (nchunk x 4: block, kind, first pair, pair count), pair (n_pairs x 2: o1, o2);
 *   plm / pkf (n_pt_obs), llm / lkf (n_ls_obs): landmark local index, keyframe local index or -1;
 *   kpp / klp (nkf + 1), kpo (n_kpo), klo (n_klo): optimised keyframe -> its observations;
 *   lpp (npt + 1) / lpo (n_lpo), llp (nls + 1) / llo (n_llo): landmark -> its observations by optimised keyframes. */
typedef struct plslam_gba_list_sizes {
    int32_t nkf, npt, nls, n_pt_obs, n_ls_obs;
    int32_t nblk, nchunk, n_pairs, n_lpo, n_llo, n_kpo, n_klo;
} plslam_gba_list_sizes;
typedef struct plslam_gba_lists {
    int32_t *blk, *chk, *pair;
    int32_t *plm, *pkf, *llm, *lkf;
    int32_t *kpp, *kpo, *klp, *klo, *lpp, *lpo, *llp, *llo;
} plslam_gba_lists;
int plslam_gba_plan_list_sizes(plslam_gba_plan* plan, plslam_gba_list_sizes* out);
int plslam_gba_plan_lists(plslam_gba_plan* plan, const plslam_gba_lists* host);
/* plslam_gba_optimize's loop -- one shared body, the same kernels, the same bits -- on state that lives on the device: d_x_kf
 * (nkf x 6), d_Xw (npt x 3), d_Lw (nls x 6) are DEVICE pointers (for the gather: X_aux, X_aux + 6 nkf, X_aux + 6 nkf + 3 npt),
 * copied device to device into the plan's state on the context's stream.  T_kf_w (n_map_kf x 16) stays a HOST pointer: poses stay
 * with the host, as everywhere in this library.  x_kf_out, T_out (may be NULL), trace and result come back to the host; the
 * landmarks stay resident in the plan (plslam_local_map_apply_gba writes them into the map image).  Works on a plan of either
 * kind, as plslam_gba_optimize does. */
int plslam_gba_optimize_dev(plslam_gba_plan* plan, double lambda_lba_lm, double lambda_lba_k, int32_t max_iters_lba,
                            const double* T_kf_w, const double* d_x_kf, const double* d_Xw, const double* d_Lw, double* x_kf_out,
                            double* T_out, plslam_gba_solve* trace, plslam_gba_result* result);
int plslam_dense_ldlt_solve(plslam_ctx* ctx, int32_t n, const double* A, const double* b, double* x, int32_t* n_bad_pivots);

/* ---- K40-K53: loop-closure correction (MapHandler::loopClosureOptimizationCovGraphG2O, src/mapHandler.cpp:4185-4410, up to
 * loopClosureFuseLandmarks()) -------------------------------------------------------------------------------------------
 * The pose graph: kf_curr_idx = max lc_idx[k][1]; vertices every non-NULL keyframe 0 .. kf_curr_idx, vertex 0 fixed; edges in
 * the reference's creation order -- covisibility (i ascending, j > i ascending: full_graph[i][j] >= min_lm_ess_graph or
 * >= min_lm_cov_graph or |i - j| == 1, measured from the stored T_kf_w), then one per LC entry (all of them, (2) == 0
 * included).  The optimiser restates g2o's Levenberg-Marquardt over EdgeSE3 / VertexSE3 with computeInitialGuess (DESIGN.md
 * section 5; parity unpinned).  The damped system is solved in a reverse Cuthill-McKee order by an envelope L D L^T on one
 * workgroup; a zero or non-finite pivot rejects the trial (g2o's failed Cholmod).  Per trial only chi', dx.(lambda dx + b)
 * and the pivot flag cross to the host.
 *   plslam_pgo_plan_create  n_map_kf keyframe slots, kf_valid (n_map_kf, 0 = NULL), full_graph (n_map_kf^2 int32, row-major),
 *                           lc_idx (n_lc x 3: the two keyframes and the (2) flag).  EINVAL: n_lc = 0, keyframe 0 NULL, an LC
 *                           entry naming a NULL or out-of-range keyframe or the same keyframe twice, no active vertex, an
 *                           active vertex without a path to vertex 0 (a singular system: a documented deviation).  ERANGE: more
 *                           than PLSLAM_GBA_MAX_KEYFRAMES active vertices.
 *   plslam_pgo_optimize     In: T_kf_w (n_map_kf x 16, row-major), x_kf_w (n_map_kf x 6), lc_pose (n_lc x 6).  Out, per slot:
 *                           T_out / x_out the corrected poses (:4298-4304, :4358-4362), T_corr the correction that slot's
 *                           landmarks take (Tkfw * inverse_se3(T_prev); the last vertex's for the slots after kf_curr_idx; the
 *                           identity elsewhere), corrected (1 where the reference corrects).  NULL slots after kf_curr_idx are
 *                           skipped (the reference dereferences them).  trace (trace_cap records, may be NULL with 0) receives
 *                           one record per trial.
 *   plslam_lc_correct_map[_dev]  :4306-4355 / :4364-4397: every corrected slot, in slot order, applies its T_corr to each valid
 *                           landmark of its anchor list -- X (both end points of a line), med_obs_dir and every dir_list entry
 *                           (p <- R p + t, the translation added to the directions as the reference does).  A landmark listed
 *                           under two slots is transformed twice, in slot order.  _dev: device pointers, on `stream` (NULL:
 *                           the context's); returns when the correction is done.
 *   plslam_envelope_ldlt_solve  the envelope L D L^T alone, in the caller's ordering: A (n x n, row-major, host; the lower
 *                           triangle read, its envelope = the first nonzero of every row), b, x; *n_bad_pivots (may be NULL),
 *                           *env_width (may be NULL): max over rows of (row - first column). */
#define PLSLAM_PGO_STOP_MAX_ITERS 0    /* max_iters_pgo iterations ran                                                */
#define PLSLAM_PGO_STOP_TERMINATE 1    /* max_trials failed trials in one iteration, or rho == 0                      */
typedef struct plslam_pgo_plan plslam_pgo_plan;
typedef struct plslam_pgo_params {
    int32_t min_lm_ess_graph, min_lm_cov_graph;   /* SlamConfig::minLMEssGraph / minLMCovGraph (75)              */
    int32_t max_iters_pgo, max_trials;            /* SlamConfig::maxItersPGO (100); g2o's maxTrialsAfterFailure (10) */
    double lambda_init;                           /* setUserLambdaInit (1e-10)                                     */
} plslam_pgo_params;
typedef struct plslam_pgo_trial {
    int32_t iteration, trial;
    double lambda, chi, chi_new, scale, rho;      /* chi_new = DBL_MAX after a failed factorisation; scale includes 1e-3 */
    int32_t ok, accepted;
} plslam_pgo_trial;
typedef struct plslam_pgo_result {
    int32_t iterations, trials, stop_reason;
    int32_t n_vertices, n_active, n_edges, n_lc_edges;
    int32_t env_width;                            /* max over rows of the reordered system of (row - first column)  */
    int64_t env_entries;                          /* doubles in the envelope                                        */
    double chi_initial, chi_final, lambda;        /* chi of computeInitialGuess's estimate and of the final state   */
} plslam_pgo_result;
typedef struct plslam_lc_landmarks {
    int32_t n, n_anchor, n_dir;
    const int32_t* anchor_ptr;   /* n_map_kf + 1: slot k lists anchor_idx[anchor_ptr[k] .. anchor_ptr[k+1]) (map_*_kf_idx) */
    const int32_t* anchor_idx;   /* n_anchor landmark indices                                                               */
    const uint8_t* valid;        /* n (0 = NULL)                                                                           */
    double* X;                   /* n x 3 (points) or n x 6 (lines)                                                        */
    double* med_dir;             /* n x 3                                                                                  */
    const int32_t* dir_ptr;      /* n + 1: landmark j's dir_list is dirs[dir_ptr[j] .. dir_ptr[j+1])                       */
    double* dirs;                /* n_dir x 3                                                                              */
} plslam_lc_landmarks;
int plslam_pgo_plan_create(plslam_ctx* ctx, const plslam_pgo_params* params, int32_t n_map_kf, const uint8_t* kf_valid,
                           const int32_t* full_graph, int32_t n_lc, const int32_t* lc_idx, plslam_pgo_plan** out);
int plslam_pgo_optimize(plslam_pgo_plan* plan, const double* T_kf_w, const double* x_kf_w, const double* lc_pose, double* T_out,
                        double* x_out, double* T_corr, uint8_t* corrected, plslam_pgo_trial* trace, int32_t trace_cap,
                        plslam_pgo_result* result);
void plslam_pgo_plan_destroy(plslam_pgo_plan* plan);
int plslam_lc_correct_map(plslam_ctx* ctx, int32_t n_map_kf, const double* T_corr, const uint8_t* corrected,
                          const plslam_lc_landmarks* points, const plslam_lc_landmarks* lines);
int plslam_lc_correct_map_dev(plslam_ctx* ctx, int32_t n_map_kf, const double* T_corr, const uint8_t* corrected,
                              const plslam_lc_landmarks* points, const plslam_lc_landmarks* lines, void* stream);
int plslam_envelope_ldlt_solve(plslam_ctx* ctx, int32_t n, const double* A, const double* b, double* x, int32_t* n_bad_pivots,
                               int32_t* env_width);

/* ---- the local map on the device: formLocalMap, the gather of localBundleAdjustment, removeBadMapLandmarks ------------- */
/* MapHandler::addKeyFrame runs formLocalMap() -> localBundleAdjustment() -> removeBadMapLandmarks() every keyframe
 * (src/mapHandler.cpp:212-225); each is a host loop over the WHOLE map.  Over a CSR image of the map kept on the device they
 * are flag scatters, stable compactions and a segmented expansion (K55-K61, KERNELS.md).
 *
 * plslam_map_index: DEVICE pointers, owned and kept up to date by the caller across keyframes.
 *   keyframes  kf_valid[n_map_kf] (0 = a NULL slot of map_keyframes; the slot index is kf_idx), x_kf_w[n_map_kf x 6]
 *   landmarks  per kind: valid[n] (0 = NULL), inlier[n], X (n x 3 point3D / n x 6 line3D), obs_ptr[n + 1] / obs_kf[n_obs] =
 *              kf_obs_list in list order, obs_val = obs_list in plslam_lba_plan_create's layout (n_obs x 2 / n_obs x 3)
 *   features   per kind: feat_ptr[n_map_kf + 1], feat_idx[n_feat] = stereo_pt[i]->idx / stereo_ls[i]->idx: -1 = no landmark,
 *              PLSLAM_FEAT_NULL = the feature pointer itself is NULL
 * plslam_local_map_cull writes valid and feat_idx; nothing else is written.  n_obs < 2^30 per kind.
 * Every index read from the image is range-checked on the device; one out of range is treated as "no landmark" / "NULL slot". */
#define PLSLAM_FEAT_NULL (-2)
typedef struct plslam_map_landmarks {
    int32_t n, n_obs;
    uint8_t* valid;
    const uint8_t* inlier;
    const double* X;
    const int32_t* obs_ptr;
    const int32_t* obs_kf;
    const double* obs_val;
    int32_t n_feat;
    const int32_t* feat_ptr;
    int32_t* feat_idx;
} plslam_map_landmarks;
typedef struct plslam_map_index {
    int32_t n_map_kf;
    const uint8_t* kf_valid;
    const double* x_kf_w;
    plslam_map_landmarks points, lines;
} plslam_map_index;
/* What the calls leave on the device (plslam_local_map_buffers: device pointers, valid until the next form / destroy, ordered on
 * `stream`) or bring to the host (plslam_local_map_download: the same struct with HOST pointers, NULL = skip; `stream` ignored).
 *   form        kf_local[n_map_kf], pt_local[npt], ls_local[nls]   uint8
 *   candidates  pt_candidate[npt], ls_candidate[nls]               uint8: d_candidate of plslam_map2kf_match_{points,lines}_dev
 *   gather      kf_list[nkf], pt_list[npt_l], ls_list[nls_l]; pt_obs / ls_obs: n_obs x 6 int32, the Vector6i columns (lm idx, lm
 *               local idx, obs idx, kf idx, kf local idx or -1, 1); the columns plslam_lba_plan_create takes: *_lm_loc (column 1),
 *               *_kf_loc (column 4), *_pose_slot (column 3: n_pose_slots = n_map_kf), pt_obs_uv (n x 2), ls_l_obs (n x 3);
 *               X_aux[6 nkf + 3 npt_l + 6 nls_l]
 *   cull        pt_removed[npt], ls_removed[nls]                   uint8
 *   apply_lba   pt_moved[npt_l], ls_moved[nls_l]                   uint8 (appended behind `stream`: the struct's prefix is unchanged) */
typedef struct plslam_local_map_buffers {
    uint8_t *kf_local, *pt_local, *ls_local, *pt_candidate, *ls_candidate, *pt_removed, *ls_removed;
    int32_t *kf_list, *pt_list, *ls_list, *pt_obs, *ls_obs;
    int32_t *pt_lm_loc, *pt_kf_loc, *pt_pose_slot, *ls_lm_loc, *ls_kf_loc, *ls_pose_slot;
    double *pt_obs_uv, *ls_l_obs, *X_aux;
    void* stream;
    uint8_t *pt_moved, *ls_moved;
} plslam_local_map_buffers;
typedef struct plslam_local_map_counts {
    int32_t n_kf_local, n_pt_local, n_ls_local;          /* form: flags set                                                  */
    int32_t nkf, npt, nls, n_pt_obs, n_ls_obs;           /* gather: list lengths (nkf excludes slot 0, :1231)                */
    int32_t empty;                                       /* gather: n_pt_obs + n_ls_obs == 0, the reference's return -1 (:1327) */
    int32_t n_pt_removed, n_ls_removed;                  /* cull                                                             */
    int32_t n_pt_moved, n_ls_moved;                      /* apply_lba (appended)                                             */
} plslam_local_map_counts;
typedef struct plslam_local_map plslam_local_map;
int plslam_local_map_create(plslam_ctx* ctx, plslam_local_map** out);
void plslam_local_map_destroy(plslam_local_map* lm);
/* formLocalMap() (:836-902; anchor_kf = n_map_kf - 1) and formLocalMap(kf) (:904-968; anchor_kf = kf->kf_idx).  row: HOST pointer
 * to full_graph[n_map_kf - 1] (n_map_kf int32) -- the overload reads the LAST row too (:946), not the anchor's.  All flags are
 * cleared; the anchor and every landmark its non-NULL features name (idx != -1 && valid) become local; every valid slot
 * i < n_map_kf - 1 with row[i] >= min_lm_cov_graph || |n_map_kf - 1 - i| <= min_kf_local_map becomes local with its features'
 * landmarks.  Deviations: the reference dereferences a NULL map_keyframes[i] (:885) and NULL features (:889) in that loop; here
 * a NULL slot and a PLSLAM_FEAT_NULL feature are skipped (so is a NULL anchor slot).  counts: the three form fields are set. */
int plslam_local_map_form(plslam_local_map* lm, const plslam_map_index* map, int32_t anchor_kf, const int32_t* row,
                          int32_t min_lm_cov_graph, int32_t min_kf_local_map, plslam_local_map_counts* counts);
/* candidate[i] = valid && local && kf_obs_list.back() != kf2_idx (:547, :649); an empty observation list gives 0 (the reference's
 * back() is undefined there).  After form on the same map. */
int plslam_local_map_candidates(plslam_local_map* lm, const plslam_map_index* map, int32_t kf2_idx);
/* The gather of localBundleAdjustment (:1225-1321), order for order.  After form on the same map; counts: the gather fields. */
int plslam_local_map_gather(plslam_local_map* lm, const plslam_map_index* map, plslam_local_map_counts* counts);
/* removeBadMapLandmarks (:2705-2786): a valid landmark with observations is removed when !local && max_kf_idx - obs_kf[first] >
 * 10 and (!inlier || n_obs < min_lm_obs).  In place on the index: valid cleared; in keyframe obs_kf[first] the FIRST feature whose
 * feat_idx equals the landmark becomes -1 (a later duplicate stays).  Erasing from map_*_kf_idx stays with the caller, driven by
 * the removed masks (a caller that corrects with plslam_lc_correct_image keeps no such lists).  Deviations: a NULL first-observer keyframe or a NULL feature (:2720-2723) is skipped; an empty observation
 * list is not culled.  After form on the same map; counts: the cull fields. */
int plslam_local_map_cull(plslam_local_map* lm, const plslam_map_index* map, int32_t max_kf_idx, int32_t min_lm_obs,
                          plslam_local_map_counts* counts);
/* The write-back of localBundleAdjustment (:1828-1855) from the plan's RESIDENT landmarks into the image, after gather on the
 * handle: for local point i, j = pt_list[i]: d = Xw[i] - X[j] per component, s2 = ((0 + d0^2) + d1^2) + d2^2 (left to right, no
 * contraction), moved = sqrt(s2) > moved_th (the reference's literal: 0.01); a moved landmark's inlier[j] is cleared (never
 * set); X[j] = Xw[i], a verbatim copy.  Lines the same over six components.  dst: WRITABLE device pointers into the caller's
 * image (plslam_map_landmarks declares X and inlier const: this call is their writer); they may be the very arrays of the index
 * the gather read -- a listed landmark occurs once in its list, so in place is safe.  pt_moved[npt_l] / ls_moved[nls_l] go into
 * the handle's buffers, n_pt_moved / n_ls_moved into counts.  One launch on the context's stream, one synchronisation.
 * Keyframe poses are not touched: the reference stores T_kf_w = expmap_se3(X_k) and leaves x_kf_w as it was (:1822-1826), and
 * the image holds x_kf_w only -- nothing to write.  The removal of observations behind the write-back (:1857-1979) never runs
 * in the reference (obs(5) is never -1) and is not here.
 * PLSLAM_EINVAL: no gather has run on the handle; the plan's npt / nls differ from the gather's counts; the plan's state is not
 * resident (no iterate / set_poses yet); the plan belongs to another context. */
typedef struct plslam_local_map_lba_dst {
    double* pt_X;
    uint8_t* pt_inlier;
    double* ls_X;
    uint8_t* ls_inlier;
} plslam_local_map_lba_dst;
int plslam_local_map_apply_lba(plslam_local_map* lm, plslam_lba_plan* plan, const plslam_local_map_lba_dst* dst, double moved_th,
                               plslam_local_map_counts* counts);
/* The flags of globalBundleAdjustment's gather (:1995-2092: localBundleAdjustment's gather without the ->local tests):
 * kf_local[i] = kf_valid[i], pt_local = valid, ls_local = valid; counts: the three form fields; the handle is formed.
 * plslam_local_map_gather then yields the GBA's kf_list (every non-NULL keyframe but slot 0), pt_list, ls_list, the Vector6i
 * rows, pt_obs_uv, ls_l_obs and X_aux, order for order.  form_all OVERWRITES the flags of the last plslam_local_map_form: a
 * plslam_local_map_cull or plslam_local_map_candidates afterwards needs a new form. */
int plslam_local_map_form_all(plslam_local_map* lm, const plslam_map_index* map, plslam_local_map_counts* counts);
/* The write-back of globalBundleAdjustment (:2681-2697) from the GBA plan's RESIDENT landmarks into the image, after gather on the
 * handle: X[pt_list[i]] = Xw[i], X[ls_list[i]] = Lw[i], verbatim copies.  No moved test; inlier is not touched (dst's inlier
 * pointers are ignored and may be NULL).  x_kf_w is not written: the reference stores only T_kf_w = expmap_se3(X) (:2676-2680),
 * which is plslam_gba_optimize's T_out.  One launch on the context's stream, one synchronisation.
 * PLSLAM_EINVAL: no gather has run on the handle; the plan's npt / nls differ from the gather's counts; no optimize has run on the
 * plan; the plan belongs to another context. */
int plslam_local_map_apply_gba(plslam_local_map* lm, plslam_gba_plan* plan, const plslam_local_map_lba_dst* dst);
int plslam_local_map_device_buffers(plslam_local_map* lm, plslam_local_map_buffers* out);
int plslam_local_map_download(plslam_local_map* lm, const plslam_local_map_buffers* host);

/* ---- a keyframe's matches into the device-resident map: the four insertion loops of MapHandler::addKeyFrame ------------- */
/* matchKF2KFPoints :280-360, matchKF2KFLines :428-527, matchMap2KFPoints :601-629 (after the gate), matchMap2KFLines :716-749
 * (src/mapHandler.cpp), over plslam_map_index, OUT OF PLACE: `src` is read, every array of `dst` is written (K63-K67, KERNELS.md);
 * the caller ping-pongs two images.  Slot kf2 is already present in src with its features at -1 / PLSLAM_FEAT_NULL.
 *
 * An EVENT is a table entry i2 >= 0 the reference acts on, in ascending i1.
 *   kf2kf   table[n_table] = matches_12 (i1: feature of kf1, i2: feature of kf2).  feat_idx[kf1][i1] == -1: a NEW landmark, index
 *           n + (rank among the new-landmark events), valid, inlier, X = T_kf1_w applied to P (lines: sP, eP), two observations
 *           (kf1, obs1[i1]) then (kf2, obs2[i2]), both features receive the index, row_delta[kf1] += 1.  Otherwise lm =
 *           feat_idx[kf1][i1]: out of range or not valid -> nothing (:333, :493); else feat_idx[kf2][i2] = lm, one observation
 *           (kf2, obs2[i2]) appended, row_delta[obs] += 1 for every entry obs != kf2 of the landmark's list.
 *   map2kf  table[n_table <= n] = map_to_kf as the plslam_map2kf_match_* drivers return it (i1: the landmark, i2: ORIGINAL feature
 *           of kf2), already gated: feat_idx[kf2][i2] = i1, one observation appended, row_delta as above; the reference has no
 *           validity check here (:615-619) and neither has this.
 * Two events that name the same i2 both append; the later one's index stays in feat_idx.  Two events on one landmark append in
 * event order.  Deviation: an event that names a PLSLAM_FEAT_NULL feature, or an i1 / i2 beyond the keyframe's features or the
 * arrays given, is SKIPPED (the reference throws, :285-288, or reads out of bounds).
 * row_delta[n_map_kf] (HOST, int32, overwritten): the increment of full_graph[kf2][.] and of full_graph[.][kf2]; full_graph
 * stays with the caller.  Also with the caller: hasRefinement's matched_pt / matched_ls, --matches and map_*_kf_idx -- driven by
 * the event records (plslam_map_insert_events).  desc_list / dir_list / pts_list and the representative descriptor follow the
 * insert on the device: plslam_map_insert_carry (below, plslam_map_lists).
 * All arithmetic fp64 without contraction: R p + t as ((r0 p0 + r1 p1) + r2 p2) + t, the norm as sqrt((x^2 + y^2) + z^2).
 *
 * plslam_map_insert_kind: HOST arrays of one landmark kind; a NULL struct or table = no entry of that kind (the kind's image is
 *   still copied).  P1 / P2: n_prev / n_curr x 3 (PointFeature::P) or x 6 (LineFeature::sP, eP) of kf1 / kf2; obs1 / obs2: x 2
 *   (pl) or x 3 (le).  map2kf reads n_curr, P2 and obs2 only.  kf2kf: n_table <= PLSLAM_MAP_INSERT_MAX_TABLE.
 * plslam_map_insert_dst: a plslam_map_index over caller-owned DEVICE buffers (every pointer is written through; kf_valid,
 *   x_kf_w and the two feat_ptr may be the source's own pointers, nothing else may) and their capacities in landmarks and
 *   observations per kind (feat_idx: the source's n_feat).  The growth is bounded by the tables alone, m = entries i2 >= 0:
 *   kf2kf needs n + m landmarks and n_obs + 2 m observations, map2kf n and n_obs + m; a smaller capacity -> PLSLAM_ERANGE before
 *   anything is launched or written.  On success map.n_map_kf and each kind's n, n_obs, n_feat are set: &dst->map is the next
 *   call's source.  PLSLAM_EINVAL: NULL arguments, slots out of range, kf1 == kf2, a destination array that is a source array.
 * Every index read from the image or a table is range-checked on the device. */
#define PLSLAM_MAP_INSERT_MAX_TABLE 65536
typedef struct plslam_map_insert_kind {
    const int32_t* table;
    int32_t n_table, n_prev, n_curr;
    const double *P1, *obs1, *P2, *obs2;
} plslam_map_insert_kind;
typedef struct plslam_map_insert_dst {
    plslam_map_index map;
    int32_t pt_cap, pt_obs_cap, ls_cap, ls_obs_cap;
} plslam_map_insert_dst;
typedef struct plslam_map_insert_kind_counts {
    int32_t n_events, n_new, n_appended, n_skipped;      /* n_appended = n_events + n_new; n_skipped: entries i2 >= 0 not acted on */
} plslam_map_insert_kind_counts;
typedef struct plslam_map_insert_counts {
    plslam_map_insert_kind_counts points, lines;
} plslam_map_insert_counts;
/* The event records of the last insert, per kind, in event order: ev n_events x 4 int32 (landmark, i1, i2, is_new); dir
 * n_events x 6 doubles: the direction of the new landmark's FIRST observation (zeros for an existing landmark), then that of the
 * kf2 observation -- new point: P3d.normalized() (:299), then P3d / P3d.norm() (:311); existing point: p3d.normalized() (:338);
 * map2kf point: R normalized(P) + t (:608, :618: the translation added to a direction is the reference's); lines: the
 * transformed midpoint, normalised (:449-450, :463-465, :496-498, :734-736).
 * obs_src[dst n_obs] int32 (appended behind `stream`: the struct's prefix is unchanged), the encoding of plslam_lc_fuse_buffers:
 * >= 0 the source observation now at that position; -1 - (2 e + w): event e (its row in ev) made it, w = 0 the keyframe-1
 * observation of a new landmark, w = 1 the keyframe-2 observation.
 * Device pointers (valid until the next insert / destroy, ordered on `stream`) or, for download, HOST pointers (NULL = skip;
 * `stream` ignored). */
typedef struct plslam_map_insert_events {
    int32_t *pt_ev, *ls_ev;
    double *pt_dir, *ls_dir;
    void* stream;
    int32_t *pt_obs_src, *ls_obs_src;
} plslam_map_insert_events;
typedef struct plslam_map_insert plslam_map_insert;
int plslam_map_insert_create(plslam_ctx* ctx, plslam_map_insert** out);
void plslam_map_insert_destroy(plslam_map_insert* mi);
/* T_kf1_w / T_kf2_w: KeyFrame::T_kf_w of the two slots, 16 doubles row-major. */
int plslam_map_insert_kf2kf(plslam_map_insert* mi, const plslam_map_index* src, plslam_map_insert_dst* dst, int32_t kf1_idx,
                            int32_t kf2_idx, const double* T_kf1_w, const double* T_kf2_w, const plslam_map_insert_kind* points,
                            const plslam_map_insert_kind* lines, int32_t* row_delta, plslam_map_insert_counts* counts);
int plslam_map_insert_map2kf(plslam_map_insert* mi, const plslam_map_index* src, plslam_map_insert_dst* dst, int32_t kf2_idx,
                             const double* T_kf2_w, const plslam_map_insert_kind* points, const plslam_map_insert_kind* lines,
                             int32_t* row_delta, plslam_map_insert_counts* counts);
int plslam_map_insert_device_buffers(plslam_map_insert* mi, plslam_map_insert_events* out);
int plslam_map_insert_download(plslam_map_insert* mi, const plslam_map_insert_events* host);

/* ---- a loop closure's landmarks fused into the device-resident map: MapHandler::loopClosureFuseLandmarks ---------------- */
/* src/mapHandler.cpp:4412-4687 over plslam_map_index, OUT OF PLACE like plslam_map_insert_*: `src` is read, every array of `dst`
 * is written (K68-K73, KERNELS.md); one launch sequence on the context's stream, one synchronisation, the counts through
 * page-locked memory.  plslam_pgo_* / plslam_lc_correct_map run loopClosureOptimizationCovGraphG2O up to this point.
 *
 * lc_idx[n_lc x 3] (HOST, int32) = lc_idx_list: (kf_prev, kf_curr, flag); an entry whose flag is not 1 contributes nothing
 * (:4419) and is not validated.  Marking the entries optimised (:4401-4402) stays with the caller.
 * plslam_lc_fuse_kind (HOST): tuples[m x 4] = the rows (lm_idx0, lm_ldx0, lm_idx1, lm_ldx1) of lc_pt_idxs / lc_ls_idxs, all
 *   entries concatenated, entry_ptr[n_lc + 1] (entry_ptr[0] = 0, m = entry_ptr[n_lc] <= PLSLAM_LC_FUSE_MAX_TUPLES); per tuple the
 *   two features' values, gathered by the caller: P0 / P1 = P of the kf_prev / kf_curr feature (m x 3; lines sP, eP: m x 6),
 *   obs0 / obs1 = pl (m x 2) or le (m x 3).  A NULL struct or entry_ptr = no tuple of that kind (its image is still copied).
 * T_kf_w[n_map_kf x 16] (HOST): KeyFrame::T_kf_w of every slot, row-major -- what plslam_pgo_optimize writes as T_out.
 *
 * An EVENT is a tuple of a flagged entry, in entry order then tuple order; its number t is its row in `tuples`.  With (a, l0, b,
 * l1) the tuple, kp / kc the entry's slots, "valid" a landmark's flag AS THE EARLIER EVENTS LEFT IT:
 *   A (-1, b)   feature l0 of kp not NULL and b valid: feat_idx[kp][l0] = b; (kp, obs0) appended to b; for every entry k of b's
 *               list after the append, full_graph[k][kc]++ and [kc][k]++ (against kf_curr, :4441; k == kc adds 2 to the
 *               diagonal).  Direction P0 / |P0|, unguarded (:4436); lines (sP + eP) / |sP + eP|.
 *   B (a, -1)   the mirror: feature l1 of kc, (kc, obs1) appended to a, increments against kp (:4446-4462).
 *   C (-1, -1)  both features not NULL: a NEW landmark n + (rank among the acted C events), valid, inlier, X = T_kp P0 (lines: sP,
 *               eP), observations (kp, obs0) then (kc, obs1), both features receive the index, full_graph[kp][kc]++ and
 *               [kc][kp]++.  Directions (T_kp P0) / |.| then (T_kc P1) / |.|; lines: 0.5 (s + e) of the transformed ends.
 *   D (a, b)    a valid, b valid, feature l1 of kc not NULL: with Nprev = len(a), b's whole list is appended to a in order;
 *               full_graph[i][j]++ and [j][i]++ for every i among the first Nprev entries of a and every j of b;
 *               feat_idx[kc][l1] = a; b becomes invalid with an empty list.  Features elsewhere that name b keep the stale index.
 * State carries from event to event: an event on a dead landmark does nothing, a later D takes a's grown list, two events that
 * write one feature leave the later one's index.
 * Deviations, where the reference has undefined behaviour; each is SKIPPED and counted in n_skipped, checked in this order: an
 * entry whose slot is NULL in kf_valid; a landmark index other than -1 outside [0, n) of the SOURCE image (a tuple cannot name a
 * landmark this call creates); an ldx the branch reads (A: l0; B, D: l1; C: both) beyond the keyframe's features; then, the
 * reference's own condition holding, a == b in D (it pushes onto the vector it iterates) and a D whose b has an empty list
 * (kf_obs_list[0], :4521).  An obs_kf entry outside [0, n_map_kf) adds nothing to the graph; each such PAIR is counted too.
 * The LEVEL of an event is 1 + the largest level among the latest earlier events that name one of its landmarks (every event
 * names its indices in [0, n), acted or not); a level above PLSLAM_LC_FUSE_MAX_LEVEL -> PLSLAM_ERANGE with dst untouched.  So
 * is a call whose graph increments number 2^30 (event, pair) items or more (A / B: the list's length, D: len(a) x len(b)).
 * A run that fails after validation (PLSLAM_ENOMEM, PLSLAM_EHIP, the two refusals above) invalidates the previous run's records.
 * desc_list / dir_list / pts_list follow on the device with plslam_lc_fuse_carry (below: one gather by obs_src from the per-tuple
 * rows the caller gathers, so the pts quirk of :4626 stays with whoever gathers).  With the caller stay
 * map_*_kf_idx (push ev's landmark to the anchor's list for C, erase the dead landmark from the anchor's for D; not needed by a
 * caller that corrects with plslam_lc_correct_image) and full_graph.
 * Arithmetic as plslam_map_insert_*: fp64 without contraction, R p + t as ((r0 p0 + r1 p1) + r2 p2) + t, the norm as
 * sqrt((x^2 + y^2) + z^2), the division per component.
 *
 * dst: as for plslam_map_insert_* (which pointers may alias, capacities).  With cC tuples (-1, -1) and cAB tuples with exactly one
 * -1 among the flagged entries the call needs n + cC landmarks and n_obs + cAB + 2 cC observations per kind; a smaller capacity ->
 * PLSLAM_ERANGE before anything is staged, launched or written.  PLSLAM_EINVAL: NULL arguments, n_lc <= 0, a flagged entry with a
 * slot out of range or kf_prev == kf_curr, a destination array that is a source array.
 * graph_delta: HOST, n_map_kf^2 int32 row-major, overwritten: the increment of full_graph; NULL: it stays on the device
 * (plslam_lc_fuse_buffers).  n_map_kf^2 < 2^28. */
#define PLSLAM_LC_FUSE_MAX_TUPLES 65536
#define PLSLAM_LC_FUSE_MAX_LEVEL 64
typedef struct plslam_lc_fuse_kind {
    const int32_t *tuples, *entry_ptr;
    const double *P0, *obs0, *P1, *obs1;
} plslam_lc_fuse_kind;
typedef struct plslam_lc_fuse_kind_counts {
    int32_t n_a, n_b, n_c, n_d;                          /* events acted on per branch                                       */
    int32_t n_new, n_dead, n_skipped;                    /* n_new = n_c, n_dead = n_d; n_skipped: the deviations above       */
} plslam_lc_fuse_kind_counts;
typedef struct plslam_lc_fuse_counts {
    plslam_lc_fuse_kind_counts points, lines;
} plslam_lc_fuse_counts;
/* The records of the last run, per kind.  ev: m x 6 int32, one row per tuple: the code (0 not acted, 1 A, 2 B, 3 C, 4 D); the
 * landmark that keeps or receives the observations, or -1; the dead landmark for D, else -1; the anchor keyframe (kf_prev for C,
 * b's first observer before the fusion for D: the key of map_*_kf_idx the caller pushes to / erases from), else -1; the position
 * in the destination's observation arrays of the first observation the event placed, or -1; the count (1, 2 or len(b)).
 * dir: m x 6 doubles: columns 0-2 the kf_prev observation's direction, 3-5 the kf_curr one, zeros where the event made none.
 * obs_src[dst n_obs] int32: >= 0 the source observation now at that position; -1 - (2 t + w): tuple t made it (w = 0 kf_prev's
 * observation, 1 kf_curr's).  graph_delta: n_map_kf^2 int32.  Device pointers (valid until the next run / destroy, ordered on
 * `stream`) or, for download, HOST pointers (NULL = skip; `stream` ignored). */
typedef struct plslam_lc_fuse_buffers {
    int32_t *pt_ev, *ls_ev;
    double *pt_dir, *ls_dir;
    int32_t *pt_obs_src, *ls_obs_src;
    int32_t* graph_delta;
    void* stream;
} plslam_lc_fuse_buffers;
typedef struct plslam_lc_fuse plslam_lc_fuse;
int plslam_lc_fuse_create(plslam_ctx* ctx, plslam_lc_fuse** out);
void plslam_lc_fuse_destroy(plslam_lc_fuse* lf);
int plslam_lc_fuse_run(plslam_lc_fuse* lf, const plslam_map_index* src, plslam_map_insert_dst* dst, int32_t n_lc,
                       const int32_t* lc_idx, const double* T_kf_w, const plslam_lc_fuse_kind* points,
                       const plslam_lc_fuse_kind* lines, int32_t* graph_delta, plslam_lc_fuse_counts* counts);
int plslam_lc_fuse_device_buffers(plslam_lc_fuse* lf, plslam_lc_fuse_buffers* out);
int plslam_lc_fuse_download(plslam_lc_fuse* lf, const plslam_lc_fuse_buffers* host);

/* ---- desc_list / dir_list / pts_list and the representative descriptor in the device-resident map ----------------------- */
/* The per-observation side lists of MapPoint / MapLine (include/mapFeatures.h) in the observation order of plslam_map_index, and
 * what MapPoint::updateAverageDescDir (src/mapFeatures.cpp:51-84, :121-157) derives from desc_list.  The reference runs it inside
 * every addMapPointObservation / addMapLineObservation (:41-49, :110-119) and behind every push of a fusion
 * (src/mapHandler.cpp:4515, :4663); the carries below refresh exactly those landmarks (K85-K88, KERNELS.md).
 * med_obs_dir is NOT kept: the reference's average accumulates into an uninitialised vector (src/mapFeatures.cpp:88-91), which
 * plslam_median_desc_batched declines to reproduce as well.
 *
 * plslam_map_lists_kind: DEVICE pointers, caller-owned; row o belongs to observation o of the image (obs_kf[o]).  Alignment: desc,
 * med_desc and pts 16 bytes, dir 8, med_idx 4 (the kernels move the 32-byte rows as two 16-byte words). */
typedef struct plslam_map_lists_kind {
    uint8_t* desc;       /* n_obs x 32: desc_list                                                       */
    double*  dir;        /* n_obs x 3 : dir_list (plslam_lc_landmarks.dirs with dir_ptr = obs_ptr)        */
    double*  pts;        /* n_obs x 4 : pts_list, lines only (may be NULL: not carried); NULL for points  */
    int32_t* med_idx;    /* n: position of the representative inside the landmark's list, -1 = empty list */
    uint8_t* med_desc;   /* n x 32: the d_med_desc of plslam_map2kf_match_*_dev                           */
    uint8_t* refreshed;  /* n, may be NULL: 1 where this call recomputed med_idx / med_desc               */
} plslam_map_lists_kind;
typedef struct plslam_map_lists { plslam_map_lists_kind points, lines; } plslam_map_lists;
/* The keyframes' rows of one kind for plslam_map_insert_carry (DEVICE): desc1 n_prev x 32 (kf2kf only), desc2 n_curr x 32 -- the
 * rows the _dev kf <-> kf drivers hold; lines: pts1 / pts2 x 4 (spl, epl).  desc 16-byte aligned, pts 16. */
typedef struct plslam_map_insert_rows {
    const uint8_t *desc1, *desc2;
    const double *pts1, *pts2;
} plslam_map_insert_rows;
/* The per-tuple rows of one kind for plslam_lc_fuse_carry (DEVICE): desc0 / desc1 m x 32, lines pts0 / pts1 m x 4, gathered by the
 * caller exactly as P0 / P1 of plslam_lc_fuse_kind. */
typedef struct plslam_lc_fuse_rows {
    const uint8_t *desc0, *desc1;
    const double *pts0, *pts1;
} plslam_lc_fuse_rows;
/* All three calls ENQUEUE on the context's stream and do not synchronise: the insert / run in front of them has synchronised and
 * left its counts on the host, so every size is known.
 *
 * plslam_map_lists_refresh: med_idx / med_desc of every landmark of both kinds recomputed from lists->desc with map's obs_ptr as
 *   offsets (the rule of plslam_median_desc_batched); refreshed, where given, becomes 1.  For the first upload.
 * plslam_map_insert_carry: after a successful plslam_map_insert_kf2kf / _map2kf on mi, with that call's images.
 * plslam_lc_fuse_carry: after a successful plslam_lc_fuse_run on lf, with that call's images.
 * Both carries, per kind and per destination observation j with s = obs_src[j]:
 *   s >= 0               desc / dir / pts rows copied verbatim from row s of src_lists
 *   s = -1 - (2 e + w)   event / tuple e made the observation: desc (pts) is the keyframe's row -- insert: desc1[i1] for w = 0,
 *                        desc2[i2] for w = 1 (i1, i2 of the event record); fuse: desc0[e] / desc1[e]; dir is columns
 *                        3 w .. 3 w + 2 of the event's direction record
 * then per destination landmark: TOUCHED (it is new, its list's length changed or its valid flag changed -- every acted event
 * lengthens one surviving landmark or empties a dead one) -> med_idx / med_desc recomputed from its destination list: element
 * int(1 + 0.5 (n - 1)) of each sorted row of distances, the smallest value wins, the first row on ties; one observation gives 0, an
 * empty list -1 and zero bytes; refreshed = 1.  UNTOUCHED -> med_idx / med_desc copied verbatim from src_lists, whatever is
 * stored there (the reference does not recompute an untouched landmark); refreshed = 0.
 * Rows beyond the destination's n_obs / n are not written.  The destination lists have the capacities of plslam_map_insert_dst.
 * A kind's lines.pts is carried when src_lists, dst_lists and (where the kind has events) the rows all give it, and not at all
 * when none does.
 * PLSLAM_EINVAL, nothing launched or written: NULL arguments; no successful insert / run on the handle (a failed one invalidates
 * the records); src_map / dst_map counts that are not the ones the handle's last call read and produced; a kind that has events
 * (fuse: tuples) but lacks its rows; pts given by some and not all of src_lists, dst_lists and the rows; a destination list
 * pointer equal to a source list pointer; a misaligned pointer; a list that is not memory of the context's device. */
int plslam_map_lists_refresh(plslam_ctx* ctx, const plslam_map_index* map, const plslam_map_lists* lists);
int plslam_map_insert_carry(plslam_map_insert* mi, const plslam_map_index* src_map, const plslam_map_lists* src_lists,
                            const plslam_map_index* dst_map, const plslam_map_lists* dst_lists,
                            const plslam_map_insert_rows* points, const plslam_map_insert_rows* lines);
int plslam_lc_fuse_carry(plslam_lc_fuse* lf, const plslam_map_index* src_map, const plslam_map_lists* src_lists,
                         const plslam_map_index* dst_map, const plslam_map_lists* dst_lists,
                         const plslam_lc_fuse_rows* points, const plslam_lc_fuse_rows* lines);

/* ---- the loop-closure map correction on the device-resident map, without anchor lists ------------------------------------ */
/* src/mapHandler.cpp:4306-4355 / :4364-4397 over plslam_map_index (K105-K107, KERNELS.md).  In the code the reference runs,
 * map_points_kf_idx[k] / map_lines_kf_idx[k] is at any time the ascending list of the valid landmarks whose FIRST observation is
 * keyframe k (pushed on creation only, :299-311, :461, :4472-4477, :4619; erased at kf_obs_list[0] only, :2717-2777, :4521-4529,
 * :4669-4676; no live code removes a first observation): a landmark has one anchor, and the image names it.  So landmark j of a
 * kind is CORRECTED when valid[j], [obs_ptr[j], obs_ptr[j + 1]) is a non-empty list inside obs_kf, k = obs_kf[obs_ptr[j]] is in
 * [0, n_map_kf) and corrected[k]; then X[j] (both end points of a line), med_dir[j] (where given) and every row of its list in
 * dir (where given; dir_ptr = obs_ptr) become R p + t with T_corr[k], ((r0 p0 + r1 p1) + r2 p2) + t without contraction, the
 * translation added to the directions as the reference does.  Everything else is left as it is.  The result is that of
 * plslam_lc_correct_map_dev given those lists, bit for bit.  A port that revives the observation removal of :1857-1979 or
 * removeRedundantKFs breaks the first-observer rule and must keep the lists and use plslam_lc_correct_map_dev.
 * A row of dir finds its landmark by bisection of obs_ptr (ascending, as every call on the image leaves it); a row that lies in
 * no landmark's list, or in the list of a landmark that is not corrected, is not touched.
 *
 * T_corr[n_map_kf x 16] and corrected[n_map_kf] (HOST): what plslam_pgo_optimize returns.  x_kf_w_new (HOST, n_map_kf x 6, may be
 * NULL): its x_out; where it and dst->x_kf_w are given, the rows of the corrected slots are written into dst->x_kf_w (:4310,
 * :4358) and no other row.  dst: WRITABLE device pointers, 8-byte aligned; in place on the image (pt_X = map->points.X, ...) is
 * the normal use.  A NULL *_dir or *_med_dir: that array is not carried (med_obs_dir is not part of plslam_map_lists).
 * counts (may be NULL): the corrected landmarks and the transformed dir rows per kind.  One staged upload, one launch sequence on the context's
 * stream, one synchronisation; the counts come back through page-locked memory.
 * PLSLAM_EINVAL, nothing launched or written: a NULL ctx / map / T_corr / corrected / dst, n_map_kf < 1, a kind of the
 * image whose counts and arrays do not agree, a kind with n > 0 and a NULL *_X, a misaligned destination.
 * Every index read from the image is range-checked on the device before it is used as an address. */
typedef struct plslam_lc_image_dst {        /* WRITABLE device pointers, caller-owned; in place on the image is the normal use */
    double *pt_X, *pt_dir, *pt_med_dir;     /* n x 3, n_obs x 3 (plslam_map_lists_kind.dir), n x 3                              */
    double *ls_X, *ls_dir, *ls_med_dir;     /* n x 6, n_obs x 3, n x 3                                                          */
    double *x_kf_w;                         /* n_map_kf x 6: the image's x_kf_w, or NULL                                        */
} plslam_lc_image_dst;
typedef struct plslam_lc_image_counts { int32_t n_pt, n_ls, n_pt_dirs, n_ls_dirs; } plslam_lc_image_counts;
int plslam_lc_correct_image(plslam_ctx* ctx, const plslam_map_index* map, const double* T_corr, const uint8_t* corrected,
                            const double* x_kf_w_new, const plslam_lc_image_dst* dst, plslam_lc_image_counts* counts);

#ifdef __cplusplus
}
#endif
#endif /* PLSLAM_HIP_H */
