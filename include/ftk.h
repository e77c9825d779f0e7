/*
 * ftk.h — C ABI of the MI355X-native sparse feature tracker (libftk_hip.so).
 *
 * This is the drop-in boundary for ONE hot path of Horizon1026/Feature_Tracker: the pyramidal
 * Lucas-Kanade trackers and the BRIEF descriptor matcher.  Every entry point names the
 * reference interface it replaces (file:line relative to the reference repo).  Signatures use
 * plain pointers and sizes only; the host-side C++ classes with the reference's names
 * (feature_tracker_amd/host/) and the Python binding (feature_tracker_amd/) sit on top.
 *
 * Conventions
 *   - (u, v) pairs are contiguous {float u(=x, col), float v(=y, row)} — the memory layout of
 *     std::vector<Vec2> (optical_flow.h:38-42).
 *   - status is one uint8_t per feature with the TrackStatus codes (src/feature_tracker.h:8-14).
 *   - images are 8-bit gray, row-major, pitch == cols (GrayImage).
 *   - 2x2 matrices (prior) are row-major [m00, m01, m10, m11].
 *   - every function returns FTK_OK (0) or a negative FTK_E_* code; ftk_last_error() gives text.
 *     There is NO CPU fallback: without a usable HIP device every compute call fails.
 *   - a context is bound to one device and one HIP stream.  Calls on ONE context may come from several
 *     threads: every entry point holds the context's lock for its duration (the context-owned scratch,
 *     pinned staging and workspaces are reused by every call), so they are serialised, not concurrent —
 *     separate tracker / matcher objects sharing a context stay independent, as in the reference.
 *     For concurrency use one context per thread.  ftk_last_error() text is valid until the next call
 *     on that context.
 */
#ifndef FTK_H_
#define FTK_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FTK_ABI_VERSION 1
#define FTK_MAX_LEVELS 12

enum {
    FTK_OK = 0,
    FTK_E_INVALID_ARGUMENT = -1,
    FTK_E_NO_DEVICE = -2,
    FTK_E_HIP = -3,
    FTK_E_UNSUPPORTED = -4,
    FTK_E_OUT_OF_MEMORY = -5,
};

/* TrackStatus, src/feature_tracker.h:8-14 */
enum {
    FTK_NOT_TRACKED = 0,
    FTK_TRACKED = 1,
    FTK_LARGE_RESIDUAL = 2,
    FTK_OUTSIDE = 3,
    FTK_NUMERIC_ERROR = 4,
};

/* OpticalFlowMethod, src/optical_flow_tracker/optical_flow.h:12-18.  kSse / kNeon (3, 4) take
 * the reference's `default:` branch, i.e. behave as kFast (basic_klt.cpp:31-34). */
enum { FTK_METHOD_INVERSE = 0, FTK_METHOD_DIRECT = 1, FTK_METHOD_FAST = 2, FTK_METHOD_SSE = 3, FTK_METHOD_NEON = 4 };

/* which tracker class: OpticalFlowBasicKlt / OpticalFlowAffineKlt / OpticalFlowLssdKlt */
enum { FTK_MODEL_BASIC = 0, FTK_MODEL_AFFINE = 1, FTK_MODEL_LSSD = 2 };

/* GrayImage view (Slam_Utility datatype_image.h; call sites basic_klt.cpp:22-23) */
typedef struct ftk_image {
    const uint8_t *data;
    int32_t rows;
    int32_t cols;
} ftk_image;

/* OpticalFlowOptions, src/optical_flow_tracker/optical_flow.h:20-28 (same defaults) */
typedef struct ftk_klt_options {
    uint32_t max_track_points;         /* kMaxTrackPointsNumber   = 500  */
    uint32_t max_iteration;            /* kMaxIteration           = 15   */
    uint32_t max_tolerance_large_step; /* kMaxToleranceLargeStep  = 3    */
    int32_t half_rows;                 /* kPatchRowHalfSize       = 6    */
    int32_t half_cols;                 /* kPatchColHalfSize       = 6    */
    float max_converge_step;           /* kMaxConvergeStep        = 4e-2 */
    int32_t method;                    /* kMethod                 = kFast */
} ftk_klt_options;

typedef struct ftk_context ftk_context;
typedef struct ftk_pyramid ftk_pyramid;

/* ---- runtime ----------------------------------------------------------------------------- */

int ftk_abi_version(void);
/* "key=value; ..." text describing this build of the library: source_hash (over every source file of libftk_hip.so; bench.py
 * compares it with the hash recorded next to committed counter figures), compiler (hipcc's version line), arch, mllvm (the
 * internal LLVM options the toolchain accepted when the library was built — each is probed, csrc/Makefile) and mllvm_rejected. */
const char *ftk_build_info(void);
/* Number of visible HIP devices (0 when none / no driver). Does not create a HIP context. */
int ftk_device_count(void);
/* stream: a hipStream_t to launch on (borrowed, e.g. a torch stream), or NULL to let the context
 * create and own one.  device < 0 keeps the calling thread's current device. */
int ftk_context_create(int device, void *stream, ftk_context **out);
void ftk_context_destroy(ftk_context *ctx);
/* Text of the last failure on this context (or of the last failed ftk_context_create when ctx is NULL).  One successful call leaves
 * text too: ftk_direct_track, when its spread launch could not become co-resident and the problem was re-run on one workgroup
 * ("note: ..."; the result is correct, the call took two launches). */
const char *ftk_last_error(const ftk_context *ctx);
int ftk_synchronize(ftk_context *ctx);
/* First-use cost out of the caller's timed region.  The reference constructs its tracker / matcher objects BEFORE it starts its
 * timer (test/test_optical_flow.cpp:64 vs :69, test_descriptor_matcher_brief.cpp:79 vs :84); the first real call of a process
 * otherwise pays for loading the kernels' code objects onto the device and for the first pinned / device staging allocations
 * (about 1.3 ms of a 1.5 ms first TrackFeatures).  `what` is a mask of the families to prepare; the C++ classes call this from
 * their constructors.  Synchronous; results of later calls do not depend on it. */
enum { FTK_WARM_KLT = 1, FTK_WARM_HAMMING = 2, FTK_WARM_COSINE = 4, FTK_WARM_DIRECT = 8, FTK_WARM_FEATURES = 16, FTK_WARM_ALL = 31 };
int ftk_warmup(ftk_context *ctx, unsigned what);
void ftk_default_klt_options(ftk_klt_options *opt);

/*
 * How the trackers sum their normal equations.
 *   FTK_REDUCTION_EXACT (default, the contract): every sum in the reference's row-major pixel order, one dependent add per
 *     term (basic_klt.cpp:139-144, affine_klt.cpp:229-256, lssd_klt.cpp:214-215) — results bit-identical to the CPU path.
 *   FTK_REDUCTION_TREE (throughput mode; measured and reported, never the default): the SAME per-pixel products,
 *     summed as per-lane partials combined by a cross-lane butterfly.  The sums then differ from the reference's in the last
 *     bits, and because the convergence test |v|^2 < kMaxConvergeStep turns such differences into an extra or a missing
 *     iteration, a small fraction of the features moves by more than the 1e-3 px the contract allows (bench.py reports max /
 *     p99 / fraction > 1e-3 px and status mismatches next to the speed).  It exists to show what bit-exactness costs.
 *     Implemented for every tracker variant except the two non-fast affine ones (24 sums of a 13 x 13 patch already run as 24
 *     parallel chains; they ignore the setting and stay exact) and for the direct method (ftk_direct_track*), whose 50 700-term
 *     chains per iteration are where the summation order costs most.  Asserted (tests/test_reduction_tree_gpu.py): bit-identical
 *     to the exact mode where every partial sum is an exact float (integer-valued terms, sums below 2^24); elsewhere one step is
 *     at least roughly as close to exactly summed products as the exact chain is (max error <= 4 x the chain's + 2 ulp, median
 *     <= the chain's + 1 ulp); repeated calls are bit-identical; affine inverse / direct and the large-patch form stay exact.
 */
enum { FTK_REDUCTION_EXACT = 0, FTK_REDUCTION_TREE = 1 };
int ftk_set_reduction_mode(ftk_context *ctx, int mode);

/* Diagnostics.  The library's FTK_* environment switches (launch shapes, kernel choices; none changes a result) are read ONCE, when
 * the context is created — no entry point calls getenv.  A test or a sweep that flips one for an existing context calls this
 * to have them read again.  Nothing in the reference corresponds to it. */
int ftk_context_refresh_env(ftk_context *ctx);

/* ---- image pyramids resident in HBM ------------------------------------------------------ */

/* A level may have up to 2^24 - 1 rows / columns and fewer than 2^32 pixels (the trackers address pixels with 32-bit
 * offsets); larger levels fail with FTK_E_UNSUPPORTED in the three calls below. */

/* Copies the levels of a host ImagePyramid (ImagePyramid::GetImageConst(i), basic_klt.cpp:22-23)
 * into ONE device allocation, level after level, each level 256-byte aligned. */
int ftk_pyramid_upload(ftk_context *ctx, const ftk_image *host_levels, int32_t n_levels, ftk_pyramid **out);
/* Borrows levels that already live in device memory (e.g. torch tensors); nothing is copied. */
int ftk_pyramid_wrap_device(ftk_context *ctx, const ftk_image *device_levels, int32_t n_levels, ftk_pyramid **out);
/* Replaces ImagePyramid::CreateImagePyramid (call sites test/test_optical_flow.cpp:70-71):
 * uploads (or borrows, image_on_device != 0) the raw image as level 0 and builds levels
 * 1..n_levels-1 on the device with the truncating 2x2 box mean. */
int ftk_pyramid_build(ftk_context *ctx, const uint8_t *image, int32_t rows, int32_t cols, int32_t n_levels, int image_on_device,
                      ftk_pyramid **out);
/* The next frame into an EXISTING pyramid (same geometry): level 0 is overwritten with `image` (rows x cols of the pyramid's
 * level 0) and levels >= 1 are rebuilt on the device — ImagePyramid::CreateImagePyramid for a tracker that is called frame after
 * frame, without an allocation per frame.  image_location: FTK_IMAGE_HOST (pageable or pinned host memory; synchronous: the
 * buffer is free again on return), FTK_IMAGE_DEVICE (device memory, stream-ordered), FTK_IMAGE_HOST_ASYNC (PINNED host memory
 * that stays valid and unchanged until the stream has passed this call; no synchronisation — when the device can address the
 * buffer (hipHostMalloc / hipHostRegister memory) the pyramid launch reads the frame itself over PCIe, without a copy-engine
 * transfer first; otherwise it is copied as with FTK_IMAGE_HOST, stream-ordered).  Only pyramids that own their level 0 (ftk_pyramid_upload,
 * ftk_pyramid_build of a host image) can be refilled. */
enum { FTK_IMAGE_HOST = 0, FTK_IMAGE_DEVICE = 1, FTK_IMAGE_HOST_ASYNC = 2 };
int ftk_pyramid_update(ftk_context *ctx, ftk_pyramid *pyr, const uint8_t *image, int image_location);
int ftk_pyramid_levels(const ftk_pyramid *pyr);
/* Device-side descriptor of one level (data is a device pointer). */
int ftk_pyramid_level(const ftk_pyramid *pyr, int32_t level, ftk_image *out);
/* Copies one level back to host memory (rows*cols bytes); for tests and for callers that still
 * need the pyramid on the host. */
int ftk_pyramid_download_level(ftk_context *ctx, const ftk_pyramid *pyr, int32_t level, uint8_t *host_out);
void ftk_pyramid_destroy(ftk_pyramid *pyr);

/* ---- KLT trackers ------------------------------------------------------------------------ */

/*
 * Replaces OpticalFlow{Basic,Affine,Lssd}Klt::TrackMultipleLevel
 * (basic_klt.cpp:7-57, affine_klt.cpp:6-59, lssd_klt.cpp:7-61) when single_level == 0 and
 * ::TrackSingleLevel (basic_klt.cpp:59-86, affine_klt.cpp:61-91, lssd_klt.cpp:63-94) when
 * single_level != 0 (only level 0 of the pyramids is used).
 *
 * Host buffers, synchronous.  cur_uv and status are in/out exactly as in the reference
 * (prediction in, result out; features whose incoming status > kTracked are skipped;
 * features beyond max_track_points are left untouched).  prior is predict_affine_
 * (affine_klt.h:50; used by the single-level path only) or predict_R_cr_ (lssd_klt.h:53);
 * NULL means identity.  consider_luminance is consider_patch_luminance_ (lssd_klt.h:54).
 * iters (optional, n entries) receives per feature the number of Gauss-Newton iterations that
 * sampled the images, summed over levels — the it(f,l) of the bytes-moved model.
 * The input normalisation of OpticalFlow::TrackFeatures (optical_flow.cpp:6-26: empty input,
 * level mismatch, vector resizing) lives in the host-side classes above this ABI.
 */
int ftk_klt_track(ftk_context *ctx, int model, const ftk_klt_options *opt, const ftk_pyramid *ref, const ftk_pyramid *cur, const float *ref_uv,
                  float *cur_uv, uint8_t *status, int32_t n, const float *prior, int consider_luminance, int single_level, uint32_t *iters);

/*
 * Same computation on device-resident buffers, asynchronous on the context's stream.
 * d_cur_uv_out / d_status_out may alias the *_in buffers (in-place, as the reference) or be
 * separate (repeatable launches for benchmarking).  d_iters may be NULL.
 * The (u, v) arrays are read and written a PAIR at a time (one 64-bit access per feature): pass them 8-byte aligned — any
 * hipMalloc'ed / pinned buffer and any offset into one by whole features is.
 * Launch order (performance only, results are independent of it): calls of >= 4 096 features keep every feature's
 * iteration count in the context, and from the third consecutive call with the same n on the features are launched
 * longest-first by the counts of two calls before (sorted by one extra workgroup of the launch in between; frame-to-frame
 * coherence of a tracker's feature list; environment FTK_KLT_SCHED=0 keeps list order).
 */
int ftk_klt_track_device(ftk_context *ctx, int model, const ftk_klt_options *opt, const ftk_pyramid *ref, const ftk_pyramid *cur,
                         const float *d_ref_uv, const float *d_cur_uv_in, float *d_cur_uv_out, const uint8_t *d_status_in,
                         uint8_t *d_status_out, int32_t n, const float *prior, int consider_luminance, int single_level, uint32_t *d_iters);

/* Replaces OpticalFlow::ExtractExtendPatchInReferenceImage (optical_flow.cpp:49-102, a public
 * helper of the reference API).  Host buffers: ex_patch has ex_rows*ex_cols floats, valid one
 * byte per pixel; *valid_count receives the return value of the reference function. */
int ftk_extract_extend_patch(ftk_context *ctx, const ftk_pyramid *ref, int32_t level, float u, float v, int32_t ex_rows, int32_t ex_cols,
                             float *ex_patch, uint8_t *valid, uint32_t *valid_count);

/* ---- BRIEF descriptors (the step in front of the matcher) ------ */

/*
 * Replaces feature_detector::BriefDescriptor::Compute (un-vendored Feature_Detector repo; call
 * sites test/test_descriptor_matcher_brief.cpp:70-76, kLength = 256, kHalfPatchSize = 8) for the
 * sampling pattern this repo defines (oracle/oracle_brief.c): bit i = S(p + a_i) < S(p + b_i) on
 * the 3x3 box sums S, p = the feature rounded to the pixel grid, offsets from a fixed-seed LCG.
 * Output is bit-packed — ceil(n_bits / 32) uint32 words per descriptor, bit i in bit (i % 32) of
 * word i / 32 — i.e. exactly what ftk_hamming_match* reads, so on the device path the descriptors
 * never visit the host.  Features closer than half_patch + 1 px to the border get all-zero words.
 */
int ftk_brief_compute(ftk_context *ctx, const ftk_pyramid *image, int32_t level, const float *uv, int32_t n, int32_t n_bits,
                      int32_t half_patch, uint32_t *words);
int ftk_brief_compute_device(ftk_context *ctx, const ftk_pyramid *image, int32_t level, const float *d_uv, int32_t n, int32_t n_bits,
                             int32_t half_patch, uint32_t *d_words);

/* ---- Harris corners (the step in front of the trackers) -------- */

/*
 * Replaces feature_detector::FeaturePointHarrisDetector::DetectGoodFeatures (un-vendored
 * Feature_Detector repo; call sites test/test_optical_flow.cpp:34-39: kMinFeatureDistance = 25,
 * kMinValidResponse = 40, at most 300 features) for the definition in oracle/oracle_harris.c:
 * 3x3 Sobel, 5x5 structure tensor in exact integers, response = (det - 0.04 tr^2) * 1e-6 in fp32,
 * candidates above min_response, window-maximum suppression over (2*min_distance - 1)^2, strongest
 * max_count survivors as (u, v) = (col, row).  uv holds 2*max_count floats; *n_out <= max_count.
 */
int ftk_harris_detect(ftk_context *ctx, const ftk_pyramid *image, int32_t level, int32_t max_count, int32_t min_distance, float min_response,
                      float *uv, int32_t *n_out);
/* The response map alone (rows*cols floats, host memory; 0 outside the 11-pixel border). */
int ftk_harris_response(ftk_context *ctx, const ftk_pyramid *image, int32_t level, float *response);

/*
 * ftk_harris_detect on the device, with a list of points that already exist: the same definition, and everything stays in
 * device memory — no copy to the host, no host sort, no synchronisation; asynchronous on the context's stream.
 *   Occupied points: point i of d_occupied_uv (n_occupied (x, y) pairs, float32) is read only where d_occupied_flags[i] != 0 (NULL flags:
 *   every point counts; n_occupied 0: none, both pointers may be NULL).  It stamps the pixel (clamp((int)floorf(x + 0.5f), 0, W - 1),
 *   clamp((int)floorf(y + 0.5f), 0, H - 1)), which may lie in the 11-pixel border band.  A candidate with a stamp within Chebyshev distance
 *   reach = max(min_distance, 1) - 1 is BLOCKED: it does not survive and it does not compete, so it suppresses nobody.  The candidates that
 *   are not blocked follow the window-maximum rule among themselves.
 *   Output: d_uv_out, [max_count][2] float32, 8-byte aligned: the strongest min(S, max_count) of the S survivors as (col, row), by response
 *   descending then pixel index ascending, and zeros behind them; d_count_out, one int32: min(S, max_count).  With no occupied point the rows
 *   are ftk_harris_detect's.  The order in which the survivors were appended to the device's list does not reach the output: a survivor's row
 *   is the number of survivors with a greater 64-bit key (keys carry the pixel index, so they are unique), counted on the device.
 *   Survivors are pairwise at Chebyshev distance >= d = max(min_distance, 1), so S <= ceil(H / d) * ceil(W / d); the list is sized by that
 *   bound and cannot overflow.  A call whose bound exceeds FTK_HARRIS_DEVICE_MAX_SURVIVORS is refused before any launch (FTK_E_UNSUPPORTED).
 *   An image below 23 x 23 has no valid centre: count 0, rows zero.  Uses the context's scratch block (it may grow: not promised capturable).
 */
#define FTK_HARRIS_DEVICE_MAX_SURVIVORS 65536
#define FTK_HARRIS_RANK_TILE 256
int ftk_harris_detect_device(ftk_context *ctx, const ftk_pyramid *image, int32_t level, int32_t max_count, int32_t min_distance, float min_response,
                             const float *d_occupied_uv, const uint8_t *d_occupied_flags, int32_t n_occupied, float *d_uv_out, int32_t *d_count_out);

/* ---- the track table (KltVideoTracker) ------------------------------------------ */

/*
 * A fixed-capacity table of tracks in device memory, n_slots = 1 .. FTK_TRACK_TABLE_MAX_SLOTS slots that never move: d_ids int64 [n] (-1 =
 * empty), d_points / d_prev_points float32 [n][2] (current / previous frame, 8-byte aligned), d_status uint8 [n] (TrackStatus; an empty slot
 * has a status > FTK_TRACKED, so ftk_klt_track_device over all n slots skips it), d_age int32 [n] (frames tracked since detection),
 * d_n_live int32 [1], d_next_id int64 [1].  Both entries are asynchronous on the context's stream and read nothing back.
 *
 * ftk_track_table_retire_device — after the frame's tracker call(s), one launch.  d_tracked_uv / d_tracked_status are the results of
 * ftk_klt_track_device with ref_uv = cur_uv_in = d_points (separate buffers, not the table's).  A slot stays live iff its id >= 0 and its
 * tracked status is FTK_TRACKED; with the forward-backward check (d_back_uv / d_back_status, both or neither: the results of a second call in
 * the opposite direction started from the tracked points) it additionally needs a backward status FTK_TRACKED and
 * fmaf(dy, dy, dx * dx) <= t * t in float32, d = backward result - the slot's point before the forward call, t = fb_threshold (>= 0) — else
 * its status becomes FTK_LARGE_RESIDUAL.  A live slot gets prev_points <- its old point, points <- tracked, age += 1.  Any other slot that held
 * a track gets id <- -1, the status and the point the tracker left; a slot that was empty is not touched.  d_free (int32 [n]) receives the
 * indices of all empty slots in ASCENDING slot order (a scan, not an atomic append), d_n_free (int32 [1]) their number, d_n_live n - that.
 *
 * ftk_track_table_fill_device — masked detection on `image` (as ftk_harris_detect_device, the slots with id >= 0 as occupied points) fused
 * with the fill: the survivor of rank r < n_free goes to slot d_free[r] with id = next_id + r, points = prev_points = (col, row), status
 * FTK_NOT_TRACKED, age 0; then next_id and n_live grow by min(n_free, S).  d_free / d_n_free as retire wrote them (for an empty table:
 * 0 .. n - 1 and n).  Refusals as ftk_harris_detect_device.
 */
#define FTK_TRACK_TABLE_MAX_SLOTS 65536
#define FTK_TRACK_TABLE_BLOCK 1024
int ftk_track_table_retire_device(ftk_context *ctx, int32_t n_slots, int64_t *d_ids, float *d_points, float *d_prev_points, uint8_t *d_status,
                                  int32_t *d_age, int32_t *d_n_live, const float *d_tracked_uv, const uint8_t *d_tracked_status,
                                  const float *d_back_uv, const uint8_t *d_back_status, float fb_threshold, int32_t *d_free, int32_t *d_n_free);
int ftk_track_table_fill_device(ftk_context *ctx, const ftk_pyramid *image, int32_t level, int32_t min_distance, float min_response, int32_t n_slots,
                                int64_t *d_ids, float *d_points, float *d_prev_points, uint8_t *d_status, int32_t *d_age, int32_t *d_n_live,
                                int64_t *d_next_id, const int32_t *d_free, const int32_t *d_n_free);

/* ---- two-view outlier rejection (EpipolarRansac) -------------------------------- */

/*
 * RANSAC on the fundamental matrix over n correspondences d_ref_uv[i] -> d_cur_uv[i] (float32 [n][2], (u, v) pixels, 8-byte aligned), all on
 * the device.  The PARTICIPANTS are the points with d_status[i] == FTK_TRACKED, in ascending index order (a scan, not an atomic append); M,
 * their number, stays on the device.  DESIGN.md 5.20 states every float operation and its order; in short, all in float32 without contraction:
 *   coordinates are normalised by the image alone: cx = 0.5f (W - 1), cy = 0.5f (H - 1), s = 2.0f / (float)(W + H), xn = (x - cx) s, and the
 *   threshold (pixels, >= 0) becomes tn = threshold s;
 *   hypothesis h = 0 .. hypotheses - 1 draws 8 distinct participants with a stated 32-bit integer mix of (seed, h, draw, attempt), at most 16
 *   attempts per draw, else h is invalid; the 8 x 9 constraint matrix is reduced by Gaussian elimination with complete pivoting (largest |a|,
 *   ties to the lowest row, then column), the null vector read off by back substitution and scaled to unit Frobenius norm; a zero or
 *   non-finite pivot, or a non-finite F, makes h invalid.  No rank-2 projection, no refit on the inliers;
 *   participant i is an inlier of h iff num^2 <= tn^2 den, den > 0, both sides finite (the Sampson test without the division); the score of h
 *   is its inlier count, -1 when invalid.  The greatest count wins, the lowest h among equal counts.
 * Outputs: d_best int32 [1] (-1: none), d_n_inliers int32 [1], d_F float32 [9] (row-major, pixel units, x_cur^T F x_ref = 0; zeros when there
 * is none), and d_status rewritten in place: a participant that is not an inlier of the winner becomes FTK_LARGE_RESIDUAL, nothing else
 * changes.  With M < 8 or every hypothesis invalid no status changes, best = -1, n_inliers = M, F = 0.  d_counts (int32 [hypotheses]) and
 * d_models (float32 [hypotheses][9], the normalised F of every hypothesis, zeros when invalid) may be NULL.
 * d_workspace: ftk_epipolar_workspace_bytes(n, hypotheses) bytes, 16-byte aligned, no initialisation needed.  n = 1 .. FTK_TRACK_TABLE_MAX_SLOTS
 * and hypotheses = 1 .. FTK_EPIPOLAR_MAX_HYPOTHESES, anything beyond is FTK_E_UNSUPPORTED before any launch.  Four launches on `stream` (a
 * hipStream_t; NULL is the null stream) of fixed shape; no host read, no synchronisation, no allocation: capturable at any time.  Integer
 * counts and integer atomics only: the result does not depend on the schedule.  The pose and the landmarks of the points this leaves TRACKED:
 * ftk_two_view_pose_device below.
 */
#define FTK_EPIPOLAR_MAX_HYPOTHESES 4096
#define FTK_EPIPOLAR_SAMPLE 8
#define FTK_EPIPOLAR_MAX_ATTEMPTS 16
#define FTK_EPIPOLAR_SCORE_TILE 256
int ftk_epipolar_workspace_bytes(int32_t n, int32_t hypotheses, int64_t *bytes);
int ftk_epipolar_ransac_device(ftk_context *ctx, void *stream, const float *d_ref_uv, const float *d_cur_uv, uint8_t *d_status, int32_t n,
                               int32_t image_rows, int32_t image_cols, float threshold, int32_t hypotheses, uint32_t seed, void *d_workspace,
                               int32_t *d_best, int32_t *d_n_inliers, float *d_F, int32_t *d_counts, float *d_models);

/*
 * The same with a choice of model.  mode FTK_TWO_VIEW_FUNDAMENTAL is ftk_epipolar_ransac_device's computation, bit for bit.
 * FTK_TWO_VIEW_HOMOGRAPHY fits x_cur ~ H x_ref instead: hypothesis h draws 4 distinct participants with the same sampler (M < 4: every h is
 * invalid), each draw gives two rows of the 8 x 9 DLT system, [x1 y1 1 0 0 0 -(x2 x1) -(x2 y1) -x2] and [0 0 0 x1 y1 1 -(y2 x1) -(y2 y1) -y2],
 * which the same elimination reduces; participant i is an inlier iff ex^2 + ey^2 <= tn^2 w^2 with w = (H6 x1 + H7 y1) + H8 != 0,
 * ex = px - x2 w, ey = py - y2 w, both sides finite (the one-sided transfer error in the current image without the division; no symmetric
 * error, no orientation test, no refit).  FTK_TWO_VIEW_AUTO runs both on the same participants and seed (one scan) and chooses the
 * homography iff it has a winner and (the fundamental matrix has none, or 1000 n_H >= prefer_homography_permille n_F, in int64); otherwise
 * the fundamental matrix if it has a winner; otherwise nothing changes and model = -1.  Only the chosen model's non-inliers become
 * FTK_LARGE_RESIDUAL.
 * Outputs: d_model int32 [1] (-1, 0 or 1), d_best / d_n_inliers int32 [2] (slot 0 the fundamental matrix, slot 1 the homography), d_F and
 * d_H float32 [9] (row-major, pixel units, x_cur ~ H x_ref; zeros when there is none), d_counts int32 [2][hypotheses] and d_models float32
 * [2][hypotheses][9] (may be NULL).  The slot of a model that did not run, or has no winner, holds best = -1, n_inliers = M and a zero
 * matrix; every count of a model that did not run is -1 and its hypotheses are zeros.
 * d_workspace: ftk_two_view_workspace_bytes(n, hypotheses, mode) bytes, 16-byte aligned, no initialisation needed.  The limits are the
 * fundamental route's; a mode outside 0 .. 2 or prefer_homography_permille outside 0 .. 1000 is FTK_E_INVALID_ARGUMENT before any launch.
 * Four launches (six with FTK_TWO_VIEW_AUTO) of fixed shape on `stream`; no host read, no synchronisation, no allocation: capturable.
 * F and H are for rejecting outliers; the pose and the landmarks of the points this leaves TRACKED: ftk_two_view_pose_device below.
 */
#define FTK_TWO_VIEW_FUNDAMENTAL 0
#define FTK_TWO_VIEW_HOMOGRAPHY 1
#define FTK_TWO_VIEW_AUTO 2
#define FTK_TWO_VIEW_HOMOGRAPHY_SAMPLE 4
int ftk_two_view_workspace_bytes(int32_t n, int32_t hypotheses, int32_t mode, int64_t *bytes);
int ftk_two_view_ransac_device(ftk_context *ctx, void *stream, const float *d_ref_uv, const float *d_cur_uv, uint8_t *d_status, int32_t n,
                               int32_t image_rows, int32_t image_cols, float threshold, int32_t hypotheses, uint32_t seed, int32_t mode,
                               int32_t prefer_homography_permille, void *d_workspace, int32_t *d_model, int32_t *d_best, int32_t *d_n_inliers,
                               float *d_F, float *d_H, int32_t *d_counts, float *d_models);

/* ---- relative pose and landmarks from two-view inliers (TwoViewPose) ------------ */

/*
 * What follows the two filters above: the refit of the essential matrix on ALL participants (d_status[i] == FTK_TRACKED, ascending index
 * order, the scan of the filters), its decomposition, the cheirality vote and the triangulation, all on the device.  DESIGN.md 5.29 states
 * every float operation and its order; in short, all in float32 without contraction, `/` and sqrtf correctly rounded:
 *   calibrated coordinates x = (u - cx) / fx, y = (v - cy) / fy, each view with its own camera (fx, fy, cx, cy); a participant with a
 *   non-finite calibrated coordinate contributes nothing to any sum and ends as FTK_LARGE_RESIDUAL;
 *   the 45 distinct entries of A = sum r r^T, r = [x2 x1, x2 y1, x2, y2 x1, y2 y1, y2, x1, y1, 1], are summed in a fixed tree: tiles of
 *   FTK_POSE_TILE participants (a position beyond M is +0), within a tile p[j] += p[j + stride] for stride 128 .. 1, tile totals in ascending
 *   order from +0.  No float atomics: the bits do not depend on the schedule;
 *   the null vector of A by cyclic Jacobi (pairs in row-major order, FTK_POSE_JACOBI_SWEEPS sweeps, no early exit), smallest eigenvalue,
 *   ties to the lowest column; the same Jacobi on E^T E gives U, V; Ehat = u1 v1^T + u2 v2^T; candidates c = 0 .. 3:
 *   R = U W V^T (c < 2) or U W^T V^T, t = u3 (c even) or -u3, with u3 = u1 x u2, v3 = v1 x v2 (det R > 0 by construction);
 *   n_front[c] counts the participants whose two-ray (midpoint) depths z1, z2 of z2 x2 = z1 R x1 + t are finite and > 0; the greatest
 *   count wins, the lowest c among equals.
 * Outputs: d_pose float32 [7] = q_rc (w, x, y, z), p_rc in ftk_direct_track's convention (x_cur ~ q_rc^-1 (X_ref - p_rc)), |p_rc| = baseline;
 * d_points float32 [n][3], z1 (x1, y1, 1) scaled to the baseline for a participant with z1, z2 > 0 and a reprojection error in the current
 * image of at most `threshold` pixels ((fx (X - x2 Z))^2 + (fy (Y - y2 Z))^2 <= threshold^2 Z^2, both sides finite), zeros elsewhere;
 * d_E float32 [9] Ehat; d_n_front int32 [4]; d_valid int32 [1] (1 / -1); d_n_points int32 [1]; d_status rewritten in place: every other
 * participant becomes FTK_LARGE_RESIDUAL.  INVALID (M < 8, a second-smallest eigenvalue of A not above 2^-20 of the largest: the points do not determine
 * E, a non-finite entry of Ehat, R, t or the pose, a winning count of 0): no
 * status changes, valid = -1, pose = (1, 0, 0, 0, 0, 0, 0), E = 0, points = 0, n_points = 0.
 * d_workspace: ftk_two_view_pose_workspace_bytes(n) bytes, 16-byte aligned, no initialisation needed.  n = 1 .. FTK_TRACK_TABLE_MAX_SLOTS
 * (beyond: FTK_E_UNSUPPORTED); fx, fy finite and > 0, cx, cy finite, threshold >= 0 with threshold^2 finite in float32 (up to about 1.8e19),
 * baseline finite and > 0, else
 * FTK_E_INVALID_ARGUMENT, all before any launch.  Five launches of fixed shape on `stream`; no host read, no synchronisation, no
 * allocation: capturable.
 */
#define FTK_POSE_JACOBI_SWEEPS 7
#define FTK_POSE_TILE 256
int ftk_two_view_pose_workspace_bytes(int32_t n, int64_t *bytes);
int ftk_two_view_pose_device(ftk_context *ctx, void *stream, const float *d_ref_uv, const float *d_cur_uv, uint8_t *d_status, int32_t n, float fx,
                             float fy, float cx, float cy, float fx_cur, float fy_cur, float cx_cur, float cy_cur, float threshold, float baseline,
                             void *d_workspace, float *d_pose, float *d_points, float *d_E, int32_t *d_n_front, int32_t *d_valid, int32_t *d_n_points);

/* ---- camera pose from landmarks and their pixels (PnpRansac) --------------------- */

/*
 * What every frame after the second asks: given landmarks d_landmarks float32 [n][3] (in the frame the points of TwoViewPose are in) and
 * the pixels d_uv float32 [n][2] where they are seen now, the pose of the camera, all on the device.  DESIGN.md 5.30 states every float
 * operation and its order (float32, no contraction, `/` and sqrtf correctly rounded); the result is a pure function of the inputs and
 * the seed.  In short:
 *   a point takes part iff d_status[i] == FTK_TRACKED, its five numbers are finite and its landmark is not exactly (0, 0, 0) (how
 *   TwoViewPose writes "no landmark"); nothing else of a point that is not TRACKED is read.  The participants are listed in ascending
 *   index order with x = (u - cx) / fx, y = (v - cy) / fy;
 *   hypothesis h draws FTK_PNP_SAMPLE = 6 distinct participants by the filters' sampler (same generator, seed mixing and
 *   FTK_EPIPOLAR_MAX_ATTEMPTS), centres their landmarks on the sample mean and divides by the mean absolute deviation, builds the DLT
 *   system of the 3 x 4 projection (two rows per point, the twelfth row dropped: 11 x 12) and takes its null vector by the filters'
 *   elimination with complete pivoting.  The conditioning is folded back, the sign fixed so that the six depths are positive.  Invalid:
 *   a zero pivot, anything non-finite, depths of both signs.  A model is P = [A | b], FTK_PNP_MODEL_FLOATS = 12 floats row-major;
 *   a participant is an inlier of camera coordinates (c0, c1, c2) iff c2 > 0 and (c0 - x c2)^2 + ((c1 - y c2) fy / fx)^2 <=
 *   (threshold / fx)^2 c2^2, both sides finite: a reprojection error of at most `threshold` pixels, without the division.  Integer counts;
 *   the highest count wins, the lowest h among equals;
 *   the winner's pose: R the nearest rotation to A through the cyclic Jacobi of A^T A (FTK_POSE_JACOBI_SWEEPS sweeps; det A < 0: the term
 *   of the smallest eigenvalue changes sign; det A = 0 or an eigenvalue <= 0: invalid), t = b / s with s the mean singular value;
 *   refine_iterations Gauss-Newton steps on the reprojection error.  The first step is taken over the inliers of the model that won (those
 *   in front of the camera under the pose: the nearest rotation of a six-point model of noisy pixels can be pixels away from the model
 *   itself), every later step over the inliers of the current pose.  Each step: the 21 + 6 sums in TwoViewPose's tree
 *   (tiles of FTK_POSE_TILE, then the tile totals in order), an LDL^T without pivoting, a first-order quaternion step with
 *   renormalisation.  A step with fewer than 6 inliers, a pivot that is not > 0, or a non-finite update ends the refit; the pose before
 *   it stands.
 * Outputs: d_pose float32 [7] = q_rc (w >= 0, x, y, z), p_rc in ftk_direct_track's convention (x_cur ~ q_rc^-1 (X - p_rc)); d_n_inliers,
 * d_best (the winning hypothesis), d_valid (1 / -1) int32 [1] each; d_counts int32 [hypotheses] (-1: invalid) and d_models float32
 * [hypotheses][12] when not null.  d_status is rewritten in place: a participant that is no inlier of the final pose becomes
 * FTK_LARGE_RESIDUAL; no other point is touched.  INVALID (fewer than 6 participants, no valid hypothesis, a singular or non-finite
 * pose; in particular landmarks of one plane, for which the six-point DLT has no unique solution): no status changes, valid = -1,
 * best = -1, n_inliers = 0, pose = (1, 0, 0, 0, 0, 0, 0).
 * d_workspace: ftk_pnp_ransac_workspace_bytes(n, hypotheses, refine_iterations) bytes, 16-byte aligned, no initialisation needed.
 * n = 1 .. FTK_TRACK_TABLE_MAX_SLOTS, hypotheses = 1 .. FTK_EPIPOLAR_MAX_HYPOTHESES, refine_iterations = 0 ..
 * FTK_PNP_MAX_REFINE_ITERATIONS (beyond: FTK_E_UNSUPPORTED); fx, fy finite and > 0, cx, cy finite, threshold >= 0 with threshold^2
 * finite in float32, else FTK_E_INVALID_ARGUMENT, all before any launch.  5 + 2 refine_iterations launches of fixed shape on `stream`;
 * no host read, no synchronisation, no allocation: capturable.
 */
#define FTK_PNP_SAMPLE 6
#define FTK_PNP_MODEL_FLOATS 12
#define FTK_PNP_MAX_REFINE_ITERATIONS 16
int ftk_pnp_ransac_workspace_bytes(int32_t n, int32_t hypotheses, int32_t refine_iterations, int64_t *bytes);
int ftk_pnp_ransac_device(ftk_context *ctx, void *stream, const float *d_landmarks, const float *d_uv, uint8_t *d_status, int32_t n, float fx,
                          float fy, float cx, float cy, float threshold, int32_t hypotheses, int32_t refine_iterations, uint32_t seed,
                          void *d_workspace, float *d_pose, int32_t *d_n_inliers, int32_t *d_best, int32_t *d_valid, int32_t *d_counts,
                          float *d_models);

/* ftk_pnp_ransac_sampled_device: ftk_pnp_ransac_device with a choice of the minimal solver behind the hypotheses.
 * sample = FTK_PNP_SAMPLE_DLT6: exactly ftk_pnp_ransac_device (which is this call with that value).  sample = FTK_PNP_SAMPLE_P3P:
 * hypothesis h draws FTK_PNP_P3P_SAMPLE = 4 distinct participants by the same sampler; the first three go to a P3P solver (Grunert's
 * quartic in s2 / s0 - 1, factored by Ferrari's resolvent cubic, whose root comes from a fixed number of Newton steps; one Newton step
 * on the three distance equations per root; float32, `+ - * /` and sqrtf alone), which returns up to four poses (R, t), x_cam = R X + t;
 * of those that put all four sample points in front of the camera, the one with the smallest (c0 - x c2)^2 + ((c1 - y c2) fy / fx)^2 at
 * the fourth point wins, the first produced among equals.  The model is [R | t], row-major, in the slot of a DLT model; invalid: a draw
 * that fails, coincident or collinear sample landmarks, two equal bearings, no solution with four positive depths, anything non-finite.
 * Every other stage is ftk_pnp_ransac_device's; a call needs 4 participants instead of 6 (a refit step still needs 6 rows: with 4 or 5
 * participants the pose is the winner's), and landmarks of one plane give a pose.  The workspace is ftk_pnp_ransac_workspace_bytes's,
 * the launches are 5 + 2 refine_iterations.  Another value of sample: FTK_E_INVALID_ARGUMENT before any launch.
 */
#define FTK_PNP_SAMPLE_DLT6 0
#define FTK_PNP_SAMPLE_P3P 1
#define FTK_PNP_P3P_SAMPLE 4
int ftk_pnp_ransac_sampled_device(ftk_context *ctx, void *stream, const float *d_landmarks, const float *d_uv, uint8_t *d_status, int32_t n,
                                  float fx, float fy, float cx, float cy, float threshold, int32_t hypotheses, int32_t refine_iterations,
                                  uint32_t seed, int32_t sample, void *d_workspace, float *d_pose, int32_t *d_n_inliers, int32_t *d_best,
                                  int32_t *d_valid, int32_t *d_counts, float *d_models);

/* ---- the landmark table beside a track table (TrackOdometry) --------------------- */

/*
 * What turns the single-shot pieces above into a per-frame front end: a table of n slots beside a track table (d_ids int64 [n], -1 = empty;
 * d_points float32 [n][2]; KltVideoTracker's or MatchVideoTracker's) that says which slot's landmark belongs to which track and gives a
 * landmark to a track born after the first pair.  The state is the caller's device arrays: d_owner int64 [n] (the id the slot's state
 * belongs to, -1: none), d_landmarks float32 [n][3] (world frame, exactly (0, 0, 0): no landmark, which is ftk_pnp_ransac_device's own
 * rule, so the array goes into it unchanged), d_anchor_uv float32 [n][2], d_anchor_pose float32 [n][7] (q_rc, p_rc of the anchor
 * observation), d_anchor_frame int32 [n] (negative: no anchor), d_counters int32 [FTK_LANDMARK_TABLE_COUNTERS] (indices below) and d_pose
 * float32 [7].  DESIGN.md 5.31 states every float operation and its order (float32, no contraction, `/` correctly rounded); every output
 * is a pure function of the inputs.  A frame is begin, the pose (ftk_pnp_ransac_device in the steady state), end.
 *
 * ftk_landmark_table_begin_device, before the pose is known.  Per slot: if d_ids[s] != d_owner[s] the slot changed hands: owner <- id, the
 * landmark zeroed, anchor_frame <- -1.  d_pnp_status[s] <- FTK_TRACKED iff id >= 0 and the landmark is not (0, 0, 0), d_anchor_status[s] <-
 * FTK_TRACKED iff id >= 0 and anchor_frame >= 0 (the participants of a two-view bootstrap on d_anchor_uv), else FTK_NOT_TRACKED.
 * The counters N_NEW, N_ANCHORED, N_LANDMARKS and N_DROPPED are zeroed: end adds to them, so end follows begin.
 *
 * ftk_landmark_table_end_device, after it.  d_pose_in float32 [7] / d_valid_in int32 [1]: the pose of this frame and its validity
 * (ftk_pnp_ransac_device's outputs, or ftk_two_view_pose_device's in the bootstrap); d_model_in int32 [1] or null: ftk_two_view_ransac_device's
 * chosen model, anything but 0 counts as invalid (a homography is no pose).  Invalid (valid_in != 1): VALID <- -1, LOST += 1 and no slot
 * changes.  Otherwise VALID <- 1, LOST <- 0, d_pose <- pose_in, and for every live slot (id >= 0):
 *   a (steady mode) d_status_in[s] == FTK_LARGE_RESIDUAL: the landmark is zeroed, the anchor dropped, N_DROPPED counts it; on to b;
 *   b (steady mode) no landmark and no anchor: anchor_uv <- points[s], anchor_pose <- pose_in, anchor_frame <- frame;
 *   c no landmark and an anchor that this call did not write: with x = (u - cx) / fx, y = (v - cy) / fy, the world rays a = R_a (x_a, y_a, 1),
 *     b = R_c (x_c, y_c, 1) (R of a quaternion by ftk_pnp_ransac_device's nine expressions) and t = p_a - p_c, the depths of z2 b = z1 a + t
 *     by ftk_two_view_pose_device's 2 x 2 normal equations.  Any non-finite input: the attempt fails.  (a.b)^2 > min_parallax_cos2
 *     ((a.a) (b.b)): it WAITS, nothing changes.  A depth not finite or <= 0: it fails.  X = ((p_a + z1 a) + (p_c + z2 b)) * 0.5 per
 *     component; not finite, exactly (0, 0, 0), or no inlier of both views by ftk_pnp_ransac_device's rule on R^T (X - p) with `threshold`:
 *     it fails.  Success: the landmark is written, N_NEW counts it.  Failure in steady mode: the slot is anchored again by b's writes; in
 *     bootstrap mode nothing changes.
 * N_ANCHORED counts the live slots that had an anchor when the call began, N_LANDMARKS those that hold a landmark when it ends (both
 * also when the pose is invalid).  Counts are ballots, one integer atomic add per workgroup of FTK_LANDMARK_TABLE_BLOCK slots and counter.
 * n = 1 .. FTK_TRACK_TABLE_MAX_SLOTS (beyond: FTK_E_UNSUPPORTED); frame >= 0, mode one of the two, fx, fy finite and > 0, cx, cy finite,
 * threshold >= 0 with threshold^2 finite in float32, min_parallax_cos2 in 0 .. 1 (the squared cosine of the parallax floor, computed by
 * the caller: no trigonometry runs on the device), else FTK_E_INVALID_ARGUMENT, all before any launch.  One launch of fixed shape each on
 * `stream`; no host read, no synchronisation, no allocation: capturable.
 */
#define FTK_LANDMARK_TABLE_BLOCK 256
#define FTK_LANDMARK_TABLE_COUNTERS 8
#define FTK_LANDMARK_TABLE_VALID 0
#define FTK_LANDMARK_TABLE_N_NEW 1
#define FTK_LANDMARK_TABLE_N_ANCHORED 2
#define FTK_LANDMARK_TABLE_N_LANDMARKS 3
#define FTK_LANDMARK_TABLE_N_DROPPED 4
#define FTK_LANDMARK_TABLE_LOST 5
#define FTK_LANDMARK_TABLE_STEADY 0
#define FTK_LANDMARK_TABLE_BOOTSTRAP 1
int ftk_landmark_table_begin_device(ftk_context *ctx, void *stream, const int64_t *d_ids, int32_t n, int64_t *d_owner, float *d_landmarks,
                                    int32_t *d_anchor_frame, uint8_t *d_pnp_status, uint8_t *d_anchor_status, int32_t *d_counters);
int ftk_landmark_table_end_device(ftk_context *ctx, void *stream, const int64_t *d_ids, const float *d_points, int32_t n, const uint8_t *d_status_in,
                                  const float *d_pose_in, const int32_t *d_valid_in, const int32_t *d_model_in, int32_t frame, int32_t mode, float fx,
                                  float fy, float cx, float cy, float threshold, float min_parallax_cos2, float *d_landmarks, float *d_anchor_uv,
                                  float *d_anchor_pose, int32_t *d_anchor_frame, int32_t *d_counters, float *d_pose);

/*
 * ftk_keypoint_decode_device — a SuperPoint-style network's head tensors to keypoints, scores and descriptors, all in device memory
 * (KeypointDecoder).  The networks are not part of this library; this is the weight-free arithmetic behind them.
 *   d_semi: float32 [65][cell_rows][cell_cols], the detector head's logits, channel 64 the dustbin.  The image is H = 8 cell_rows by
 *   W = 8 cell_cols.  Per cell: m = the maximum (x_0, then `if (x_k > m) m = x_k` ascending), e_k = exp_c(x_k - m),
 *   sum = e_0 + e_1 + ... + e_64 ascending, score_k = e_k / sum at pixel (8 cy + k / 8, 8 cx + k % 8) for k < 64.  A pixel is a candidate
 *   iff score > min_score and it lies at least `border` pixels from every image edge; its key is sortable(score) << 32 | ~pixel index.
 *   Suppression and selection are ftk_harris_detect_device's on that key plane (d_occupied_uv / d_occupied_flags / n_occupied as there):
 *   row r < max_keypoints of d_uv receives (col, row) of the survivor of rank r, d_scores[r] its score, d_count[0] = min(S, max_keypoints);
 *   rows behind the count are zeros.
 *   d_desc: float32, `channels` channels over the cell grid, element (c, cy, cx) at d_desc[c desc_stride_c + cy desc_stride_y +
 *   cx desc_stride_x] (strides in elements, >= 0).  Row r of d_descriptors [max_keypoints][channels] is the bilinear sample at
 *   xc = min(max((x - 3.5) * 0.125, 0), cell_cols - 1), yc likewise, v_c = ((w00 d00 + w01 d01) + w10 d10) + w11 d11, divided by
 *   max(sqrt(n2), 1e-12) where n2 sums v_c^2 per lane of 64 (fmaf, channels l, l + 64, ... ascending) and then over six rounds
 *   p_l + p_(l xor off), off = 32 .. 1.  Non-finite values propagate.
 *   d_heatmap: float32 [H][W] of every pixel's score, or NULL.
 * d_workspace: ftk_keypoint_decode_workspace_bytes(cell_rows, cell_cols, min_distance, n_occupied) bytes, 16-byte aligned, no
 * initialisation needed.  Limits: H, W <= 65 536; ceil(H / d) ceil(W / d) <= FTK_HARRIS_DEVICE_MAX_SURVIVORS with d = max(min_distance, 1)
 * (FTK_E_UNSUPPORTED); 1 <= max_keypoints <= FTK_KEYPOINT_DECODE_MAX_KEYPOINTS; 1 <= channels <= FTK_KEYPOINT_DECODE_MAX_CHANNELS;
 * min_score finite; border >= 0.  Everything is refused before any launch.  7 launches (10 with occupied points) of fixed shape on
 * `stream`; no host read, no synchronisation, no allocation: capturable.
 */
#define FTK_KEYPOINT_DECODE_CELL 8
#define FTK_KEYPOINT_DECODE_MAX_KEYPOINTS 65536
#define FTK_KEYPOINT_DECODE_MAX_CHANNELS 1024
int ftk_keypoint_decode_workspace_bytes(int32_t cell_rows, int32_t cell_cols, int32_t min_distance, int32_t n_occupied, int64_t *bytes);
int ftk_keypoint_decode_device(ftk_context *ctx, void *stream, const float *d_semi, int32_t cell_rows, int32_t cell_cols, const float *d_desc,
                               int32_t channels, int64_t desc_stride_c, int64_t desc_stride_y, int64_t desc_stride_x, int32_t max_keypoints,
                               float min_score, int32_t min_distance, int32_t border, const float *d_occupied_uv, const uint8_t *d_occupied_flags,
                               int32_t n_occupied, void *d_workspace, float *d_uv, float *d_scores, float *d_descriptors, int32_t *d_count,
                               float *d_heatmap);

/*
 * ftk_match_assignment_device — LightGlue's assignment head: two descriptor sets to the log-assignment tensor that
 * ftk_nn_match_scores_device reads, all in device memory (MatchAssignment).  It replaces the tail of the network run at
 * nn_feature_matcher.cpp:130-131 (session_.Run), which is upstream LightGlue's MatchAssignment.forward; the transformer layers before it
 * are not part of this library.
 *   d_desc0 [rows0][dim], d_desc1 [rows1][dim]: float32, dense rows.  d_weights: float32 [dim + 1][dim], rows 0 .. dim - 1 final_proj.weight
 *   and row dim matchability.weight; d_bias: float32 [dim + 1] likewise; both NULL: no projection and no matchability, every descriptor
 *   element is multiplied by `scale` (finite, > 0; ignored with weights).  d_count0 / d_count1: int32 [1] device words or NULL: rows
 *   i < n0 = clamp(count0, 0, rows0) and columns j < n1 = clamp(count1, 0, rows1) are valid (NULL: all).
 *   d_scores: [rows0 + 1] rows of row_stride floats (0: rows1 + 1), of which rows1 + 1 are written: entry (i, j) of the valid block is
 *   ((sim - lse_row_i) + (sim - lse_col_j)) + (ls(z0_i) + ls(z1_j)), the dustbin column ls(-z0_i), the dustbin row ls(-z1_j), the
 *   corner +0; without weights there is no ls term and the dustbins are -inf; every entry of an invalid row or column is -inf.  The
 *   arithmetic is DESIGN.md 5.23's to the bit.  Non-finite values propagate; the inputs are never written.
 * d_workspace: ftk_match_assignment_workspace_bytes(rows0, rows1, dim, with_weights) bytes, 16-byte aligned, no initialisation needed.
 * Limits: 1 <= rows0, rows1 <= FTK_MATCH_ASSIGNMENT_MAX_ROWS; 1 <= dim <= FTK_MATCH_ASSIGNMENT_MAX_DIM; row_stride 0 or >= rows1 + 1.
 * Everything is refused before any launch.  4 launches (3 without weights) of fixed shape on `stream`; no host read, no
 * synchronisation, no allocation: capturable.
 */
#define FTK_MATCH_ASSIGNMENT_MAX_ROWS 4096
#define FTK_MATCH_ASSIGNMENT_MAX_DIM 1024
int ftk_match_assignment_workspace_bytes(int32_t rows0, int32_t rows1, int32_t dim, int32_t with_weights, int64_t *bytes);
int ftk_match_assignment_device(ftk_context *ctx, void *stream, const float *d_desc0, int32_t rows0, const float *d_desc1, int32_t rows1, int32_t dim,
                                const float *d_weights, const float *d_bias, float scale, const int32_t *d_count0, const int32_t *d_count1,
                                void *d_workspace, float *d_scores, int64_t row_stride);

/*
 * ftk_transformer_layer_device — one of LightGlue's transformer layers (TransformerLayer): the self block on each
 * descriptor set, then the cross block in both directions, all in device memory.  ftk_attention_device and ftk_linear_device are two
 * of its kernels alone.
 *   d_desc0 [rows0][dim], d_desc1 [rows1][dim]: float32, dense rows; head a is columns a * dh .. a * dh + dh - 1, dh = dim / heads.
 *   d_enc0 [2][rows0][dh], d_enc1 [2][rows1][dh]: the rotary encoding's cos and sin planes, repeat-interleaved as upstream caches them.
 *   d_weights: the layer's tensors packed as DESIGN.md 5.24 states (TransformerLayer.from_state_dict packs them): per block the input
 *   Linear (self: q | k | v rows, 3 dim; cross: to_qk | to_v, 2 dim) and its bias, the output Linear and its bias, ffn.0 [2 dim][2 dim]
 *   and its bias, LayerNorm's weight and bias [2 dim], ffn.3 [dim][2 dim] and its bias; the self block first.
 *   d_count0 / d_count1: int32 [1] device words or NULL: keys at or behind clamp(count, 0, rows) take part in no softmax (NULL: all).
 *   d_out0 [rows0][dim], d_out1 [rows1][dim]: the layer's result; they may not overlap the inputs.
 * ftk_attention_device: out [rows_q][heads * head_dim] = softmax((q pre)(k pre)^T post) v per head over the first clamp(count, 0,
 * rows_k) keys; no valid key gives +0.  ftk_linear_device: out [rows][out_dim] = x [rows][in_dim] weight^T + bias.
 * d_workspace: ftk_transformer_layer_workspace_bytes(rows0, rows1, dim, heads) bytes, 16-byte aligned, no initialisation needed.
 * Limits: 1 <= rows <= FTK_TRANSFORMER_MAX_ROWS per side; 1 <= dim <= FTK_TRANSFORMER_MAX_DIM; heads divides dim; dh even and in
 * 2 .. FTK_TRANSFORMER_MAX_HEAD_DIM; scales finite and > 0.  Everything is refused before any launch.  12 launches of fixed shape
 * (attention, linear: 1) on `stream`; no host read, no synchronisation, no allocation: capturable.  The arithmetic is DESIGN.md 5.24's
 * to the bit.  Non-finite values propagate; the inputs are never written.
 */
#define FTK_TRANSFORMER_MAX_ROWS 4096
#define FTK_TRANSFORMER_MAX_DIM 1024
#define FTK_TRANSFORMER_MAX_HEAD_DIM 128
int ftk_transformer_layer_workspace_bytes(int32_t rows0, int32_t rows1, int32_t dim, int32_t heads, int64_t *bytes);
int ftk_attention_device(ftk_context *ctx, void *stream, const float *d_q, int32_t rows_q, const float *d_k, const float *d_v, int32_t rows_k,
                         int32_t heads, int32_t head_dim, const int32_t *d_count, float pre_scale, float post_scale, float *d_out);
int ftk_linear_device(ftk_context *ctx, void *stream, const float *d_x, int32_t rows, int32_t in_dim, const float *d_weight, const float *d_bias,
                      int32_t out_dim, float *d_out);
int ftk_transformer_layer_device(ftk_context *ctx, void *stream, const float *d_desc0, int32_t rows0, const float *d_desc1, int32_t rows1, int32_t dim,
                                 int32_t heads, const float *d_enc0, const float *d_enc1, const float *d_weights, const int32_t *d_count0,
                                 const int32_t *d_count1, void *d_workspace, float *d_out0, float *d_out1);

/*
 * LightGlue's adaptive depth and width (LightGlue.match_adaptive): the steps that stop the network once enough points
 * are confident and that remove points which are confidently unmatchable, all in device memory.  A pass owns two halves of a
 * ping-pong pair of descriptors [rows][dim], rotary encodings [2][rows][dh] and index maps int32 [rows] per side, conf and mt
 * float32 [rows0 + rows1], layers int32 [rows] per side (zeroed by the caller) and d_state, int32 [FTK_LIGHTGLUE_STATE_WORDS]:
 * the live counts of both sides, the sticky stop flag, the stop layer (initialised by the caller to clamp(count), 0, L - 1).
 *   ftk_transformer_layer_adaptive_device: ftk_transformer_layer_device in place on d_desc0 / d_desc1, with the live counts (required)
 *   as the counts; every workgroup returns before its first load when *d_gate != 0 or when all of its rows lie at or behind their
 *   set's live count.  Rows at or behind the live count are unspecified afterwards.
 *   ftk_lightglue_confidence_device: conf = sigmoid_c(token(x)) and mt = sigmoid_c(matchability(x)) of every live row, each the fmaf
 *   chain over the columns ascending from its bias (d_live0 / d_live1 / d_gate may be NULL: all rows, never gated).  1 launch.
 *   ftk_lightglue_adapt_step_device: layer i's stop test and pruning (5.26 steps 3 and 4), then the stable gather of the kept rows of
 *   the `in` half to the front of the `out` half (the identity when stopped or not pruning).  d_count0 / d_count1: the pass's input
 *   counts or NULL.  threshold: t_i; depth_confidence / width_confidence <= 0: off.  2 launches.
 *   ftk_lightglue_finish_device: selects log_assignment.{stop layer} out of d_head_w [L][dim + 1][dim] and d_head_b [L][dim + 1], runs
 *   ftk_match_assignment_device and ftk_nn_match_scores_device on the compacted sets with the live counts (d_scores: [rows0 + 1][rows1
 *   + 1], compacted layout) and maps the result back: d_match_index [rows0] and d_status [rows0] in original indices, -1 and
 *   FTK_STATUS_LARGE_RESIDUAL for every row without a match; d_layers0 / d_layers1 receive stop layer + 1 for the rows that stayed.
 * d_workspace: ftk_lightglue_adaptive_workspace_bytes(rows0, rows1, dim, heads) bytes, 16-byte aligned, no initialisation needed; it
 * contains the layer's and the head's workspaces.  Limits: ftk_transformer_layer_device's, and at most FTK_LIGHTGLUE_MAX_LAYERS
 * layers.  Everything is refused before any launch; launches of fixed shape on `stream`; no host read, no synchronisation.
 */
#define FTK_LIGHTGLUE_MAX_LAYERS 64
#define FTK_LIGHTGLUE_STATE_WORDS 4
int ftk_lightglue_adaptive_workspace_bytes(int32_t rows0, int32_t rows1, int32_t dim, int32_t heads, int64_t *bytes);
int ftk_transformer_layer_adaptive_device(ftk_context *ctx, void *stream, float *d_desc0, int32_t rows0, float *d_desc1, int32_t rows1, int32_t dim,
                                          int32_t heads, const float *d_enc0, const float *d_enc1, const float *d_weights, const int32_t *d_live0,
                                          const int32_t *d_live1, const int32_t *d_gate, void *d_workspace);
int ftk_lightglue_confidence_device(ftk_context *ctx, void *stream, const float *d_desc0, int32_t rows0, const float *d_desc1, int32_t rows1, int32_t dim,
                                    const float *d_token_w, const float *d_token_b, const float *d_match_w, const float *d_match_b,
                                    const int32_t *d_live0, const int32_t *d_live1, const int32_t *d_gate, float *d_conf, float *d_mt);
int ftk_lightglue_adapt_step_device(ftk_context *ctx, void *stream, int32_t rows0, int32_t rows1, int32_t dim, int32_t heads, int32_t layer,
                                    const float *d_conf, const float *d_mt, const int32_t *d_count0, const int32_t *d_count1, int32_t *d_state,
                                    float threshold, float depth_confidence, float width_confidence, int32_t min_keypoints, const float *d_desc_in0,
                                    const float *d_desc_in1, const float *d_enc_in0, const float *d_enc_in1, const int32_t *d_ind_in0,
                                    const int32_t *d_ind_in1, float *d_desc_out0, float *d_desc_out1, float *d_enc_out0, float *d_enc_out1,
                                    int32_t *d_ind_out0, int32_t *d_ind_out1, int32_t *d_layers0, int32_t *d_layers1, void *d_workspace);
int ftk_lightglue_finish_device(ftk_context *ctx, void *stream, const float *d_desc0, int32_t rows0, const float *d_desc1, int32_t rows1, int32_t dim,
                                int32_t heads, int32_t n_layers, const float *d_head_w, const float *d_head_b, const int32_t *d_state,
                                const int32_t *d_ind0, const int32_t *d_ind1, float min_score, void *d_workspace, float *d_scores,
                                int32_t *d_match_index, uint8_t *d_status, int32_t *d_layers0, int32_t *d_layers1);

/* ---- the landmark table (MatchVideoTracker) -------------------------------------- */

/*
 * A fixed-capacity table of landmarks in device memory for tracking with learned features over a frame sequence.  It extends the step at
 * nn_feature_matcher.cpp:187-215 (the mutual-best matches of one pair) to a sequence: the matcher is asked about the TABLE, the last
 * seen position and descriptor of every live track, not about the previous frame's detections, so a landmark hidden for a few frames
 * is found again under its identity.  n_slots = 1 .. FTK_MATCH_TABLE_MAX_SLOTS slots that never move (the matchers' row limit):
 * d_ids int64 [n] (-1 = empty), d_points / d_prev_points float32 [n][2] (8-byte aligned), d_descriptors float32 [n][dim], dim = 1 ..
 * FTK_MATCH_TABLE_MAX_DIM, d_status uint8 [n], d_age int32 [n] (frames matched since admission), d_lost int32 [n] (frames since the slot
 * was last matched), d_n_live int32 [1], d_next_id int64 [1].
 *
 * ftk_match_table_query_device — the table as a matcher's reference set.  The live slots (id >= 0) in ASCENDING slot order (a scan, not
 * an atomic append) become rows 0 .. nq - 1 of d_q_uv [n][2] (8-byte aligned), d_q_desc [n][dim] and d_q_slot int32 [n] (the row's
 * slot); d_q_count [1] = nq.  Rows at or behind nq are +0 in d_q_uv and d_q_desc and -1 in d_q_slot.  The table is not written.
 *
 * ftk_match_table_update_device — one frame's results into the table.  d_q_slot / d_q_count as the query wrote them; d_match_index
 * int32 [n] and d_match_status uint8 [n] as ftk_nn_match_scores_device or ftk_lightglue_finish_device wrote them for the query rows
 * against the current set d_cur_uv [rows_cur][2] (8-byte aligned), d_cur_desc [rows_cur][dim], rows_cur = 1 .. FTK_MATCH_TABLE_MAX_SLOTS;
 * d_cur_count int32 [1] or NULL (all rows); max_lost >= 0.  With nq = clamp(q_count, 0, n) and nk = clamp(cur_count, 0, rows_cur):
 *   1. row r < nq NAMES j = match_index[r] iff 0 <= j < nk; it is a HIT iff it names j, match_status[r] == FTK_TRACKED and no lower hit
 *      row names the same j (an integer atomicMin per j: a pure function of the inputs).  A current row named by any row is CLAIMED,
 *      hit or not: a match the geometric filter rejected does not come back as a new track on the same keypoint.
 *   2. for r < nq and s = q_slot[r], a slot live before the call: a hit gets prev_points[s] <- points[s], points[s] <- cur_uv[j],
 *      descriptors[s] <- cur_desc[j] (replaced, not averaged), age += 1, lost <- 0, status FTK_TRACKED; any other gets lost += 1, status
 *      FTK_LARGE_RESIDUAL and, if lost > max_lost, id <- -1 (its other fields stay).  A slot that was empty before the call is not touched.
 *   3. the unclaimed current rows j < nk in ascending j and the empty slots after step 2 (the ones just retired included) in ascending
 *      slot order: for rank r < min(#unclaimed, #empty) the r-th row goes to the r-th slot with id next_id + r, points = prev_points =
 *      cur_uv[j], its descriptor, age 0, lost 0, status FTK_NOT_TRACKED; then next_id grows by the number admitted and n_live is the
 *      live count.
 * d_cur_slot int32 [rows_cur], or NULL: the slot each current row now belongs to (hit or admitted), else -1.
 * d_workspace: ftk_match_table_workspace_bytes(n_slots, rows_cur, dim) bytes, 16-byte aligned, no initialisation needed.  No argument may
 * alias another: equal pointers are refused.  Everything is refused (FTK_E_INVALID_ARGUMENT) before any launch.  2 launches each of
 * fixed shape on `stream` (one workgroup of FTK_TRACK_TABLE_BLOCK threads scans up to four flags per thread, then one wave per
 * descriptor row moves it, 16 bytes per lane when dim % 4 == 0 and the descriptor bases are 16-byte aligned); no host read, no
 * synchronisation, no allocation: capturable.  Integer logic and copies only.
 */
#define FTK_MATCH_TABLE_MAX_SLOTS 4096
#define FTK_MATCH_TABLE_MAX_DIM 1024
int ftk_match_table_workspace_bytes(int32_t n_slots, int32_t rows_cur, int32_t dim, int64_t *bytes);
int ftk_match_table_query_device(ftk_context *ctx, void *stream, int32_t n_slots, int32_t dim, const int64_t *d_ids, const float *d_points,
                                 const float *d_descriptors, float *d_q_uv, float *d_q_desc, int32_t *d_q_slot, int32_t *d_q_count);
int ftk_match_table_update_device(ftk_context *ctx, void *stream, int32_t n_slots, int32_t dim, int64_t *d_ids, float *d_points, float *d_prev_points,
                                  float *d_descriptors, uint8_t *d_status, int32_t *d_age, int32_t *d_lost, int32_t *d_n_live, int64_t *d_next_id,
                                  const int32_t *d_q_slot, const int32_t *d_q_count, const int32_t *d_match_index, const uint8_t *d_match_status,
                                  const float *d_cur_uv, const float *d_cur_desc, int32_t rows_cur, const int32_t *d_cur_count, int32_t max_lost,
                                  void *d_workspace, int32_t *d_cur_slot);

/* ---- diagnostics ---------------------------------------------------------------------------- */

/*
 * Solves n independent 6x6 systems A x = b with the device's Eigen-compatible pivoted LDLT — the
 * primitive inside the affine trackers (affine_klt.cpp:103, affine_klt_fast.cpp:39 `H.ldlt().solve(b)`)
 * and the direct method (direct_method_tracker.cpp:170) — so that tests can compare it with the oracle
 * on matrices a tracker would rarely produce (ties, zero pivots, NaN).  a: n x 36 row-major symmetric,
 * b: n x 6, x: n x 6; host buffers.
 */
int ftk_ldlt6_solve(ftk_context *ctx, const float *a, const float *b, float *x, int32_t n);

/* ---- direct method ---------------------------------------------- */

/* DirectMethodOptions, src/direct_method_tracker/direct_method_tracker.h:20-28 */
typedef struct ftk_direct_options {
    uint32_t max_track_points;   /* kMaxTrackPointsNumber (500)  */
    uint32_t max_iteration;      /* kMaxIteration         (15)   */
    int32_t half_rows;           /* kPatchRowHalfSize     (6)    */
    int32_t half_cols;           /* kPatchColHalfSize     (6)    */
    float max_converge_step;     /* kMaxConvergeStep      (1e-6) */
    float max_converge_residual; /* kMaxConvergeResidual  (2.0; the reference never reads it) */
    int32_t method;              /* kMethod (FTK_METHOD_DIRECT); kInverse / kFast are empty stubs in the reference and no-ops here */
} ftk_direct_options;
void ftk_default_direct_options(ftk_direct_options *opt);

/*
 * Replaces DirectMethod::TrackFeatures, camera-frame overload (direct_method_tracker.cpp:35-86) with
 * TrackSingleLevel -> TrackAllFeaturesDirect (:88-106, :115-192): photometric Gauss-Newton on ONE pose
 * (q_rc, p_rc) over all features jointly, coarse to fine.  K = {fx, fy, cx, cy}; p_c_in_ref = n x 3 points in
 * the reference camera frame; cur_uv in/out (the caller applies ":42-44 sizes differ -> cur = ref");
 * q_rc = (w, x, y, z) and p_rc in/out; status in/out with status_valid = 0 meaning "was not sized n"
 * (reset to kTracked, :73-75).  iterations (optional) = Gauss-Newton iterations over all levels.
 * The sums of the normal equations keep the scalar loop's order (feature by feature, pixel by pixel),
 * so pose, pixels and iteration counts are those of the scalar code.  The world-frame overload
 * (:8-33) is host-side quaternion algebra around this call and lives in the C++ class.
 * Any number of tracked features: up to 3072 their per-iteration projections live in LDS, above that in a
 * context-owned device buffer (same arithmetic, same order of the sums).
 */
int ftk_direct_track(ftk_context *ctx, const ftk_direct_options *opt, const ftk_pyramid *ref, const ftk_pyramid *cur, const float *K,
                     const float *p_c_in_ref, const float *ref_uv, float *cur_uv, int32_t n, float *q_rc_wxyz, float *p_rc, uint8_t *status,
                     int status_valid, uint32_t *iterations);

/* A batch of independent pose problems in ONE launch (one workgroup each), buffers device-resident.
 * d_pose = 7 floats: q_rc (w, x, y, z) then p_rc.  All problems share the options and the pyramid depth. */
typedef struct ftk_direct_problem {
    const ftk_pyramid *ref;
    const ftk_pyramid *cur;
    float K[4];
    const float *d_p_c_in_ref;
    const float *d_ref_uv;
    float *d_cur_uv;
    int32_t n;
    float *d_pose;
    uint8_t *d_status;
    int32_t status_valid;
    uint32_t *d_iterations; /* may be NULL */
} ftk_direct_problem;
int ftk_direct_track_batch_device(ftk_context *ctx, const ftk_direct_options *opt, const ftk_direct_problem *problems, int32_t n_problems);

/* ---- dense optical flow (Farneback) ------------------------------------------------------------ */

/* DenseOpticalFlow::Options, src/dense_optical_flow_tracker/dense_optical_flow.h:15-20 (same defaults).  k_moments = {k2, k4, k22}
 * of the Gaussian kernel, read ONLY when half_patch == 0: the reference then keeps the object's previous values
 * (dense_optical_flow.cpp:95-98 returns before :119-131), which are 0 for a fresh object; the classes above pass what their
 * object holds.  Larger half patches recompute them.  half_patch may be at most 255 here (the reference has no bound). */
typedef struct ftk_dense_flow_options {
    int32_t max_iteration;     /* kMaxIteration     (10)   */
    int32_t half_patch;        /* kHalfPatchSize    (2)    */
    float max_converge_step;   /* kMaxConvergeStep  (1e-6) */
    float max_delta_flow_step; /* kMaxDeltaFlowStep (1.0)  */
    float k_moments[3];        /* k2, k4, k22 for half_patch == 0 (0, 0, 0) */
} ftk_dense_flow_options;
#define FTK_DENSE_MAX_HALF_PATCH 255
void ftk_default_dense_flow_options(ftk_dense_flow_options *opt);

/* InitializeGaussianKernel (dense_optical_flow.cpp:87-134) on the host, no device needed: the library's single definition of the
 * table.  weights_out (optional): (2 half_patch + 1)^2 floats, row-major; k_out (optional): {k2, k4, k22}, left as passed for
 * half_patch == 0 (the reference's quirk).  FTK_E_INVALID_ARGUMENT for half_patch < 0 (the reference's `return false`) or above
 * FTK_DENSE_MAX_HALF_PATCH. */
int ftk_dense_flow_gaussian(int32_t half_patch, float *weights_out, float *k_out);

/*
 * Replaces DenseOpticalFlow::Track(ImagePyramid, ImagePyramid, flow_rc) (dense_optical_flow.cpp:35-85): coarse to fine from zero
 * flow at the coarsest level; per level the moment images of both images (:136-189), the per-pixel Gauss-Newton refinement
 * (:191-245) and the 3x3 median (:334-371), then the smoothed flow upsampled to the next level (:66-77).  flow_r / flow_c receive
 * level 0's ref size (rows x cols, row-major: row and column components of the flow).  Both pyramids need the same level count
 * (>= 1; the reference returns false otherwise — the classes above check).  half_patch < 0 gives zero flow and FTK_OK (the
 * reference ignores the per-level `false`).  Host buffers, synchronous.
 */
int ftk_dense_flow(ftk_context *ctx, const ftk_dense_flow_options *opt, const ftk_pyramid *ref_pyr, const ftk_pyramid *cur_pyr, float *flow_r,
                   float *flow_c);
/* The same on device buffers (d_flow_r / d_flow_c: level 0's ref size), stream-ordered on the context's stream, no host
 * synchronisation, capturable.  Workspace (moment images, flow planes, the Gaussian table) belongs to the context and grows only on
 * calls outside a stream capture: a captured call whose shape or half patch needs more fails with FTK_E_UNSUPPORTED — make one
 * uncaptured call of the same shape first. */
int ftk_dense_flow_device(ftk_context *ctx, const ftk_dense_flow_options *opt, const ftk_pyramid *ref_pyr, const ftk_pyramid *cur_pyr, float *d_flow_r,
                          float *d_flow_c);
/* Replaces DenseOpticalFlow::Track(GrayImage, GrayImage, flow_rc) (:7-33) on level `level` of both pyramids (ref and cur may differ in
 * size).  flow_r / flow_c: host buffers of the ref level's size, in/out; flow_valid bit 0: flow_r holds a ref-sized initial guess
 * (otherwise it is reset to zero, :18-20), bit 1 the same for flow_c (:21-23).  half_patch < 0 fails with FTK_E_INVALID_ARGUMENT
 * and leaves the flow untouched (the reference's `return false`). */
int ftk_dense_flow_level(ftk_context *ctx, const ftk_dense_flow_options *opt, const ftk_pyramid *ref_pyr, const ftk_pyramid *cur_pyr, int32_t level,
                         float *flow_r, float *flow_c, int32_t flow_valid);

/* ---- RAFT correlation pyramid (src/nn_optical_flow_tracker/raft/correlation_volumes.py) ------------------------ */

/*
 * CorrelationPyramid (correlation_volumes.py:19-83) on caller-provided memory: the library holds no workspace, so both device entries
 * are stream-ordered, never synchronise and can be captured in a graph at any time.  Feature maps are contiguous float32 [B][C][H][W];
 * the volume is ONE buffer of ftk_corr_pyramid_layout's size, level l at element level_offsets[l], laid out [B*H*W][level_h[l]][level_w[l]]
 * (the reference's [B*H*W, 1, H_l, W_l] tensors).  Both device entries enqueue on `stream` (a hipStream_t; NULL is the null stream),
 * not on the context's own stream, so a caller's current stream orders them; the context selects the device and records errors.
 */
#define FTK_CORR_MAX_LEVELS 16
#define FTK_CORR_MAX_RADIUS 64
/* Host only, no device needed.  *elements: floats of the whole volume, 4 * B * H * W * sum_l H_l * W_l bytes; level_offsets (elements),
 * level_h, level_w (each optional, `levels` entries).  H_l = H_{l-1} / 2 and W_l = W_{l-1} / 2 rounded down (avg_pool2d, :27-34).
 * FTK_E_INVALID_ARGUMENT for non-positive sizes, levels outside 1 .. FTK_CORR_MAX_LEVELS, a level with H_l or W_l == 0 (the reference
 * raises in avg_pool2d) or a size that overflows int64. */
int ftk_corr_pyramid_layout(int32_t B, int32_t H, int32_t W, int32_t levels, int64_t *elements, int64_t *level_offsets, int32_t *level_h,
                            int32_t *level_w);
/* __init__ (:20-34) and ComputeCorrelation (:36-46): level 0 = f0^T f1 / sqrt(C) per batch item (an fmaf chain over the channels in
 * ascending order from +0, divided by (float)sqrt((double)C)), then levels - 1 2x2 average pools.  d_volume: the layout's size. */
int ftk_corr_pyramid_build_device(ftk_context *ctx, void *stream, const float *d_fmap0, const float *d_fmap1, int32_t B, int32_t C, int32_t H,
                                  int32_t W, int32_t levels, float *d_volume);
/* __call__ (:48-77) and the model's concatenation (model.py:87-88): for every pixel and level the (2r+1)^2 bilinear window around
 * d_coords / 2^l (d_coords: [B][2][H][W], x then y).  per_level == 0: d_out is [B][levels * (2r+1)^2][H][W], the tensor model.py:88
 * builds; per_level != 0: d_out holds `levels` consecutive blocks [B][H][W][(2r+1)^2], the list __call__ returns.  radius 0 .. FTK_CORR_MAX_RADIUS. */
int ftk_corr_pyramid_lookup_device(ftk_context *ctx, void *stream, const float *d_volume, int32_t B, int32_t H, int32_t W, int32_t levels,
                                   int32_t radius, const float *d_coords, float *d_out, int32_t per_level);

/* ---- RAFT on-demand correlation: the lookups of the pyramid above without its volume ------------------------ */

/*
 * The same windows as ftk_corr_pyramid_lookup_device, with no correlation value ever stored: the workspace holds fmap0 transposed to
 * [B][H*W][C] (element 0) and fmap1 pooled through the levels with the pyramid's pool formula, level l channel-last as
 * [B][level_h[l]][level_w[l]][C] at element level_offsets[l]; a lookup evaluates the correlation of a query pixel with a level position
 * as the fmaf chain over the channels (ascending, from +0) of fmap0[b, c, p] * fmap1_l[b, c, y2, x2], divided by (float)sqrt((double)C),
 * zero outside the level, and samples it exactly as the pyramid's lookup does.  Level 0 is bit-identical to the pyramid's; levels >= 1
 * are the same quantity with other roundings (the pool is linear).  Any C >= 1; limits FTK_CORR_MAX_LEVELS and FTK_CORR_MAX_RADIUS.
 * The library holds no workspace and allocates nothing; both device entries enqueue on `stream` and can be captured in a graph.
 */
/* Host only.  *elements = B * C * (H * W + sum_l H_l * W_l) floats; level_offsets (elements), level_h, level_w as for
 * ftk_corr_pyramid_layout (each optional, `levels` entries), and its level rules and errors. */
int ftk_corr_ondemand_layout(int32_t B, int32_t C, int32_t H, int32_t W, int32_t levels, int64_t *elements, int64_t *level_offsets, int32_t *level_h,
                             int32_t *level_w);
/* Once per image pair: transposes d_fmap0 and d_fmap1 (contiguous float32 [B][C][H][W]) and pools d_fmap1 into d_workspace (the layout's
 * size; a 16-byte aligned one with C % 4 == 0 lets the lookup load 16 bytes at a time).  1 + (levels - 1) launches. */
int ftk_corr_ondemand_prepare_device(ftk_context *ctx, void *stream, const float *d_fmap0, const float *d_fmap1, int32_t B, int32_t C, int32_t H,
                                     int32_t W, int32_t levels, float *d_workspace);
/* d_coords and d_out as for ftk_corr_pyramid_lookup_device (both output forms), from the prepared workspace alone.  One launch. */
int ftk_corr_ondemand_lookup_device(ftk_context *ctx, void *stream, const float *d_workspace, int32_t B, int32_t C, int32_t H, int32_t W,
                                    int32_t levels, int32_t radius, const float *d_coords, float *d_out, int32_t per_level);

/* ---- RAFT convex flow upsampling (src/nn_optical_flow_tracker/raft/model.py) ------------------------ */

/* Coarse pixels along x that one workgroup of the kernel owns: shapes just below, at and above a multiple of it are the ones a test
 * of the entry below should cover. */
#define FTK_FLOW_UPSAMPLE_TILE 32
/* Replaces Raft.UpsampleFlow(flow, mask_scale * mask) (model.py:48-64, the scaling is update_block.py:66): per fine pixel (8y + i, 8x + j)
 * the softmax over the 9 logits mask[b][k * 64 + i * 8 + j][y][x] * mask_scale, k = 0 .. 8, applied to 8 * flow of the zero-padded
 * 3 x 3 neighbourhood of coarse pixel (y, x), in the operation order DESIGN.md 5.12 fixes.  d_flow: [B][2][H][W], d_mask: [B][576][H][W],
 * d_out: [B][2][8H][8W], all contiguous float32 on the context's device.  One launch on `stream` (a hipStream_t; NULL is the null
 * stream), no allocation, no synchronisation: capturable at any time.  FTK_E_INVALID_ARGUMENT, before any launch, for a null pointer,
 * a non-positive size, a non-finite mask_scale or a mask whose byte count overflows int64. */
int ftk_flow_upsample_device(ftk_context *ctx, void *stream, const float *d_flow, const float *d_mask, int32_t B, int32_t H, int32_t W,
                             float mask_scale, float *d_out);

/* ---- Sparse tracking from RAFT's coarse flow ------------------------ */

/* Feature points that one workgroup of the kernel owns: point counts just below, at and above a multiple of it are the ones a test of
 * the entry below should cover. */
#define FTK_FLOW_POINTS_TILE 64
/* Tracks N feature points per batch entry through the flow that Raft.UpsampleFlow(flow, mask_scale * mask) (model.py:48-64) would give,
 * without storing it: d_points [B][N][2] (u = x, v = y, image pixels) -> d_cur_points [B][N][2], d_status [B][N] (uint8, TrackStatus) and,
 * when it is not NULL, d_fb_error2 [B][N].  Per point, in the operation order DESIGN.md 5.17 fixes:
 *   inside(p) is 0 <= p.u <= image_cols - 1 and 0 <= p.v <= image_rows - 1 in float32 (NaN fails); a reference point that is not inside
 *   is FTK_OUTSIDE with cur = ref;
 *   S(p) is the bilinear sample at p of the fine flow, whose four values are the floats ftk_flow_upsample_device writes, the right and
 *   lower neighbours clamped to the grid's last column and row; cur = ref + S(ref): non-finite is FTK_NUMERIC_ERROR with cur = ref, not
 *   inside is FTK_OUTSIDE with cur as computed;
 *   with the backward pair (d_flow_back, d_mask_back: both or neither), a point that is still inside gets e2 = |cur + S_back(cur) - ref|^2,
 *   and FTK_LARGE_RESIDUAL unless e2 <= fb_threshold^2 (a NaN e2 is a large residual); otherwise FTK_TRACKED.
 * d_fb_error2 is e2 where the check ran and 0 elsewhere.  1 <= image_rows <= 8H and 1 <= image_cols <= 8W: the image may be smaller than
 * the grid (RAFT's encoders round sizes up), and a pixel of the grid outside the image is outside.  d_flow, d_flow_back: [B][2][H][W];
 * d_mask, d_mask_back: [B][576][H][W]; all contiguous float32 on the context's device.  One launch on `stream` (a hipStream_t; NULL is
 * the null stream), no allocation, no synchronisation: capturable at any time.  N = 0 is FTK_OK with no launch, and the three point
 * buffers may then be NULL.
 * FTK_E_INVALID_ARGUMENT, before any launch, for a null required pointer, a non-positive B, H or W or a negative N, 8H or 8W above 2^24
 * (float32 coordinates name every fine pixel up to there), image_rows or image_cols out of range, a non-finite mask_scale, a negative
 * or NaN fb_threshold, half a backward pair, or a mask whose byte count overflows int64. */
int ftk_flow_track_points_device(ftk_context *ctx, void *stream, const float *d_flow, const float *d_mask, const float *d_flow_back,
                                 const float *d_mask_back, int32_t B, int32_t H, int32_t W, int32_t N, int32_t image_rows, int32_t image_cols,
                                 float mask_scale, float fb_threshold, const float *d_points, float *d_cur_points, uint8_t *d_status,
                                 float *d_fb_error2);

/* ---- The warm start of RAFT on video ------------------------ */

/* Targets that one workgroup of the kernel owns, and sources of one LDS tile: pixel counts just below, at and above a multiple of it
 * are the ones a test of the entry below should cover. */
#define FTK_FLOW_WARM_TILE 256
/* The search is all targets against all sources: H * W is held to this. */
#define FTK_FLOW_WARM_MAX_PIXELS (1 << 20)
#define FTK_FLOW_WARM_MAX_SPLITS 32
/* Host only: the number of source ranges ("splits") the entry below should be called with at these sizes, 1 .. FTK_FLOW_WARM_MAX_SPLITS,
 * chosen so that the scan fills the chip; FTK_E_INVALID_ARGUMENT for a non-positive size or H * W above FTK_FLOW_WARM_MAX_PIXELS. */
int ftk_flow_warm_splits(int32_t B, int32_t H, int32_t W, int32_t *splits);
/* Replaces upstream RAFT's forward_interpolate (core/utils/utils.py: scipy.interpolate.griddata(method="nearest") on the host, per batch
 * entry): the coarse flow d_flow [B][2][H][W] (channel 0 = x) pushed forward along itself into d_out [B][2][H][W], both contiguous float32
 * on the context's device and distinct.  In float32, in the operation order DESIGN.md 5.18 fixes: source pixel s = y W + x lands at
 * x1 = (float)x + flow[b][0][y][x], y1 = (float)y + flow[b][1][y][x] and is valid iff x1 > 0 && x1 < (float)W && y1 > 0 && y1 < (float)H
 * (a NaN or infinite landing is not); target (tx, ty) takes both components of the valid source with the least
 * d2 = fmaf(ey, ey, ex * ex), ex = (float)tx - x1, ey = (float)ty - y1, the least s among equal d2, as copies of its two input floats;
 * a batch entry without a valid source is all +0.  Batch entries are independent.
 * `splits` = 1: one launch, d_workspace may be NULL.  2 .. FTK_FLOW_WARM_MAX_SPLITS: the sources are scanned in that many ranges by as
 * many times the workgroups, and a second launch combines them through d_workspace, splits * B * H * W 64-bit words that need no
 * initialisation.  The result does not depend on `splits`.  On `stream` (a hipStream_t; NULL is the null stream), no allocation, no
 * synchronisation: capturable at any time.
 * FTK_E_INVALID_ARGUMENT, before any launch, for a null pointer (the workspace with splits > 1 too), d_out == d_flow, a non-positive
 * size, H * W above FTK_FLOW_WARM_MAX_PIXELS or splits out of range; a grid beyond 2^31 - 1 workgroups is FTK_E_HIP. */
int ftk_flow_warm_device(ftk_context *ctx, void *stream, const float *d_flow, int32_t B, int32_t H, int32_t W, int32_t splits,
                         uint64_t *d_workspace, float *d_out);

/* ---- RAFT separable ConvGRU (src/nn_optical_flow_tracker/raft/gru.py:46-76) ------------------------ */

/*
 * SepConvGru.forward (gru.py:59-76) as two kernels per pass, each a 1 x ks (horizontal) or ks x 1 (vertical) convolution as an
 * implicit GEMM on the f32-input matrix cores with the activation and the element-wise tail in its epilogue.  The input of a
 * convolution is the channel concatenation of 1 .. FTK_SEP_CONV_GRU_MAX_PARTS tensors of x, read in place, then h (gates) or r * h
 * (blend): no concatenation is ever stored.  Everything is contiguous float32 [B][channels][H][W] on the context's device.
 * Limits: kernel_size 3 or 5; 1 <= h_channels <= FTK_SEP_CONV_GRU_MAX_H_CHANNELS; x_channels >= 1 and x_channels + h_channels <=
 * FTK_SEP_CONV_GRU_MAX_IN_CHANNELS; any B, H, W >= 1.  A size outside them is FTK_E_UNSUPPORTED and launches nothing.
 *
 * Packed weights: the weight matrix [M][K], K = kernel_size * C_in in torch's own order k = c * kernel_size + t (M = 2 h_channels for
 * the gates: the rows of z, then those of r; M = h_channels for q), as [ceil(M / 32)][k_steps][64] floats: entry (tile, s, lane) is
 * W[32 tile + lane % 32][2 s + lane / 32]; k_steps = ceil(C_in / FTK_SEP_CONV_GRU_CHUNK) * FTK_SEP_CONV_GRU_CHUNK * kernel_size / 2;
 * a k >= K is packed as -0.0f, a row >= M as +0.0f.  The bias is [M].
 */
#define FTK_SEP_CONV_GRU_MAX_PARTS 3
#define FTK_SEP_CONV_GRU_MAX_H_CHANNELS 1024
#define FTK_SEP_CONV_GRU_MAX_IN_CHANNELS 4096
#define FTK_SEP_CONV_GRU_CHUNK 16
typedef struct ftk_gru_part {
    const float *data; /* [B][channels][H][W] */
    int32_t channels;
} ftk_gru_part;
/* Host only, no device needed: floats of the packed matrix of out_channels rows over in_channels = x_channels + h_channels. */
int ftk_sep_conv_gru_packed_elements(int32_t out_channels, int32_t in_channels, int32_t kernel_size, int64_t *elements);
/* gru.py:59-76, lines 63-66 (vertical == 0) / 70-73 (vertical != 0): d_z = sigmoid_c(conv_z(x | h)), d_rh = sigmoid_c(conv_r(x | h)) * h.
 * d_weights: the packed stacked z | r matrix, d_bias: [2 h_channels].  One launch on `stream` (a hipStream_t), no allocation, no
 * synchronisation: capturable. */
int ftk_sep_conv_gru_gates_device(ftk_context *ctx, void *stream, const ftk_gru_part *x_parts, int32_t n_parts, const float *d_h, const float *d_weights,
                                  const float *d_bias, int32_t h_channels, int32_t kernel_size, int32_t vertical, int32_t B, int32_t H, int32_t W, float *d_z,
                                  float *d_rh);
/* gru.py:59-76, lines 66-68 / 73-75: d_out = (1 - z) * h + z * tanh_c(conv_q(x | rh)), every operation one float32 rounding.
 * d_weights: the packed q matrix, d_bias: [h_channels].  d_out must not alias d_h, d_z or d_rh.  One launch on `stream`. */
int ftk_sep_conv_gru_blend_device(ftk_context *ctx, void *stream, const ftk_gru_part *x_parts, int32_t n_parts, const float *d_rh, const float *d_z,
                                  const float *d_h, const float *d_weights, const float *d_bias, int32_t h_channels, int32_t kernel_size, int32_t vertical,
                                  int32_t B, int32_t H, int32_t W, float *d_out);

/* ---- RAFT UpdateBlock's stock layers (src/nn_optical_flow_tracker/raft/update_block.py:4-67) ------------------------ */

/*
 * The nine convolutions around the GRU (MotionEncoder: update_block.py:20-35, FlowHead: :7-9, the mask head: :56-60) are one thing: a
 * stride-1 square convolution of kernel_size 1, 3 or 7 with zero padding kernel_size / 2, a bias, an optional ReLU and an output scale,
 * run as an implicit GEMM on the f32-input matrix cores.  The input is the channel concatenation of 1 .. FTK_CONV2D_MAX_PARTS tensors
 * read in place (no concatenation is ever stored); everything is contiguous float32 [B][channels][H][W] on the context's device.
 * Per output element: acc = bias[co]; for k = (c * kernel_size + ty) * kernel_size + tx ascending, acc = fmaf(W[co][k], in[c][y + ty -
 * pad][x + tx - pad], acc), a tap outside the image being a multiplied +0; then v = (acc < 0) ? +0 : acc if relu; then out =
 * out_scale * v, one rounded multiply.
 * Limits: kernel_size 1, 3 or 7; 1 <= out_channels <= FTK_CONV2D_MAX_OUT_CHANNELS; 1 <= in_channels <= FTK_CONV2D_MAX_IN_CHANNELS; any
 * B, H, W >= 1.  A size outside them is FTK_E_UNSUPPORTED and launches nothing.
 *
 * Packed weights: torch's own [M][K], K = C_in * kernel_size^2, as [ceil(M / 32)][k_steps][64] floats: entry (tile, s, lane) is
 * W[32 tile + lane % 32][2 s + lane / 32]; k_steps = ceil(C_in / chunk) * chunk * kernel_size^2 / 2 with chunk = FTK_CONV2D_CHUNK_1, _3
 * or _7 by kernel size; a k >= K is packed as -0.0f, a row >= M as +0.0f.  The bias is [M].
 */
#define FTK_CONV2D_MAX_PARTS 3
#define FTK_CONV2D_MAX_OUT_CHANNELS 1024
#define FTK_CONV2D_MAX_IN_CHANNELS 4096
#define FTK_CONV2D_CHUNK_1 32
#define FTK_CONV2D_CHUNK_3 8
#define FTK_CONV2D_CHUNK_7 2
/* Host only, no device needed: floats of the packed matrix of out_channels rows over in_channels. */
int ftk_conv2d_packed_elements(int32_t out_channels, int32_t in_channels, int32_t kernel_size, int64_t *elements);
/* One layer of update_block.py: a Conv2d and, with relu != 0, the ReLU after it: correlation_conv (:21-24, kernel sizes 1 and 3),
 * flow_conv (:27-30, 7 and 3), out_conv (:33-34, whose input, :39's cat, is parts = {temp_correlation, temp_flow}), FlowHead (:7-9, :11-13)
 * and the mask head (:57-59), whose last layer takes out_scale = 0.25f in place of :66's pass over the mask; out_scale is 1 elsewhere.
 * parts: the input's tensors (ftk_gru_part: a device pointer and its channel count).  d_out: [B][out_channels][H][W], not aliasing an
 * input.  One launch on `stream` (a hipStream_t), no allocation, no synchronisation: capturable. */
int ftk_conv2d_device(ftk_context *ctx, void *stream, const ftk_gru_part *parts, int32_t n_parts, const float *d_weights, const float *d_bias,
                      int32_t out_channels, int32_t kernel_size, int32_t relu, float out_scale, int32_t B, int32_t H, int32_t W, float *d_out);

/* ---- RAFT's encoders (src/nn_optical_flow_tracker/raft/encoder.py:4-68) ------------------------------------------- */

/*
 * The layers of FeatureEncoder / ContextEncoder are the layer above with three additions.  BatchNorm (eval mode) is no addition: the
 * caller folds it into the weights and the bias once (s = gamma / sqrtf(var + eps), w' = w * s, b' = beta - mean * s).
 *  - stride 1 or 2 (2: kernel sizes 1 and 3 only): the input is [B][in_channels][H][W], the output [B][out_channels][ceil(H / stride)]
 *    [ceil(W / stride)], the tap of output (y, x) is in[c][stride * y + ty - pad][stride * x + tx - pad], outside the image a multiplied +0.
 *  - d_residual (may be NULL): a dense tensor of the output's shape; v = acc + residual[co][y][x], one rounded add, BEFORE the ReLU
 *    (encoder.py:21-22); then ReLU and out_scale as above.
 *  - normalise != 0: every in-image input value x is read as 2.0f * (x / 255.0f) - 1.0f (model.py:70-71: one rounded division, an exact
 *    doubling, one rounded subtraction); the zero padding stays +0, which is why this is no change of the weights.
 * Limits as ftk_conv2d_device; any other stride, or stride 2 with kernel_size 7, is FTK_E_UNSUPPORTED and launches nothing.  The packed
 * weights are ftk_conv2d_device's (the stride changes neither the layout nor the chunk).  stride 1 with no residual and normalise == 0
 * is ftk_conv2d_device itself.
 * Replaces, per call: encoder.py:16-18 (conv1, bn1, ReLU: stride as the block's, relu); :21's shortcut (:12-13: 1 x 1, the block's
 * stride, its BatchNorm, no ReLU); :19-22 (conv2, bn2, the add of the shortcut as d_residual, ReLU); :30-31 (conv_in, 7 x 7, normalise);
 * :46-47 (conv_out).  d_out must not alias an input or the residual.  One launch on `stream`, no allocation, no synchronisation: capturable.
 */
int ftk_conv2d_strided_device(ftk_context *ctx, void *stream, const ftk_gru_part *parts, int32_t n_parts, const float *d_weights, const float *d_bias,
                              int32_t out_channels, int32_t kernel_size, int32_t stride, int32_t relu, float out_scale, const float *d_residual,
                              int32_t normalise, int32_t B, int32_t H, int32_t W, float *d_out);

/* ---- SuperPoint's VGG and descriptor head --------------------------------------------------------------------- */

/*
 * ftk_conv2d_device's layer (kernel_size 1 or 3) with a 2 x 2 max-pool of stride 2 in its epilogue: SuperPoint's conv1b, conv2b and conv3b
 * with the ReLU and the pool after them, in one launch that never stores the tensor before the pool.  d_out: [B][out_channels][H / 2][W / 2]
 * (floored: a last odd row or column is computed and dropped, as by torch's max_pool2d(2, 2)).  Per output element, with acc the chain of
 * ftk_conv2d_device: v = (acc < 0) ? +0 : acc if relu, else acc; pick(m, x) = (x > m || x != x) ? x : m; out = pick(pick(v00, v01),
 * pick(v10, v11)) over the window's (row, column) offsets: torch's scan, a NaN propagates and among equal maxima (+-0 included) the first
 * of (0,0), (0,1), (1,0), (1,1) wins.  There is no out_scale.  Packed weights, parts and limits as ftk_conv2d_device, and H, W >= 2
 * (FTK_E_INVALID_ARGUMENT); kernel_size 7 is FTK_E_UNSUPPORTED; neither launches anything.  One launch on `stream`, no allocation, no
 * synchronisation: capturable.
 */
int ftk_conv2d_pool_device(ftk_context *ctx, void *stream, const ftk_gru_part *parts, int32_t n_parts, const float *d_weights, const float *d_bias,
                           int32_t out_channels, int32_t kernel_size, int32_t relu, int32_t B, int32_t H, int32_t W, float *d_out);
/*
 * The L2 normalisation of a dense descriptor map over its channels, with the change of layout ftk_keypoint_decode_device reads fastest:
 * d_in [channels][cell_rows][cell_cols] to d_out [cell_rows][cell_cols][channels] (strides 1, cell_cols * channels, channels there).  Per
 * cell: n2 = fmaf(x_c, x_c, n2) over ascending c from +0; den = fmaxf(sqrtf(n2), 1e-12f); y_c = x_c / den (torch's F.normalize(dim = 1)
 * with this summation order; square root and division correctly rounded).  1 <= channels <= FTK_KEYPOINT_DECODE_MAX_CHANNELS,
 * cell_rows, cell_cols >= 1 (FTK_E_INVALID_ARGUMENT).  d_out must not alias d_in.  One launch on `stream`, no allocation, no
 * synchronisation: capturable.
 */
int ftk_channel_normalise_device(ftk_context *ctx, void *stream, const float *d_in, int32_t channels, int32_t cell_rows, int32_t cell_cols, float *d_out);

/* ---- features sharded over the GPUs of one node ------------------------ */

/*
 * The reference has no parallelism of any kind; what shards is the independence of its units: every feature's
 * computation reads the two pyramids and its own (ref_uv, cur_uv, status) only (basic_klt.cpp:13-54, affine_klt.cpp:12-56,
 * lssd_klt.cpp:13-58), every reference descriptor's scan is its own (descriptor_matcher.h:67-76).  One process per GPU;
 * rank r of `world` works on the contiguous block ftk_shard_bounds(n, world, r) with both pyramids (or all candidates)
 * replicated, and ONE all-gather of the packed result shards — RCCL ncclAllGather over xGMI, issued from this library on the
 * context's stream right behind the kernel — gives every rank the complete result in the original order, identical to the
 * single-GPU result.  kMaxTrackPointsNumber stays a cap on the GLOBAL feature index (basic_klt.cpp:9).
 *
 * Bootstrap: rank 0 calls ftk_comm_unique_id and hands the 128 bytes to the other ranks by any means (a file, MPI,
 * torch.distributed ...); every rank then calls ftk_comm_create.  RCCL is bound at run time (dlopen): without it these
 * calls fail with FTK_E_UNSUPPORTED and everything else keeps working.  world == 1 with a NULL id needs no RCCL at all.
 */
typedef struct ftk_comm ftk_comm;
#define FTK_UNIQUE_ID_BYTES 128
/* [begin, end) of rank's block: the first n % world ranks hold one unit more. */
void ftk_shard_bounds(int32_t n, int32_t world, int32_t rank, int32_t *begin, int32_t *end);
/* Bytes of ONE rank's packed tracker shard: ceil(n / world) * (8 B (u, v) + 1 B status), rounded up to 16 B. */
size_t ftk_klt_shard_bytes(int32_t n, int32_t world);
int ftk_comm_unique_id(void *id_out /* FTK_UNIQUE_ID_BYTES */);
int ftk_comm_create(ftk_context *ctx, int32_t rank, int32_t world, const void *unique_id, ftk_comm **out);
void ftk_comm_destroy(ftk_comm *comm);
int ftk_comm_rank(const ftk_comm *comm);
int ftk_comm_world(const ftk_comm *comm);

/*
 * ftk_klt_track_device over the ranks of `comm`.  Every rank passes the SAME full-length device buffers (n features);
 * on return (asynchronously, stream-ordered) every rank's d_cur_uv_out / d_status_out hold all n results.
 * Launches: the tracker kernel on this rank's block, ncclAllGather of the packed shards, one scatter kernel.
 * d_iters (optional, n entries) receives only this rank's block.
 * Failure symmetry: a rank whose tracker launch fails still takes part in the collective with a POISONED shard (every byte
 * 0xFF: status 255, NaN coordinates) and returns its error, so its peers finish instead of blocking; the host-buffer form below
 * turns a poisoned block into FTK_E_HIP on every rank, the device form leaves it visible in the data.  (A rank that cannot even
 * allocate its exchange buffers cannot contribute: destroy the communicator's process group in that case.)
 * HIP-graph capture: the exchange buffers grow on demand (hipFree / hipMalloc, which a capture does not allow), so make ONE eager
 * call with the largest n before capturing any.
 */
int ftk_klt_track_sharded_device(ftk_context *ctx, ftk_comm *comm, int model, const ftk_klt_options *opt, const ftk_pyramid *ref,
                                 const ftk_pyramid *cur, const float *d_ref_uv, const float *d_cur_uv_in, float *d_cur_uv_out,
                                 const uint8_t *d_status_in, uint8_t *d_status_out, int32_t n, const float *prior, int consider_luminance,
                                 int single_level, uint32_t *d_iters);
/* Host-buffer form (synchronous; cur_uv / status in/out as in ftk_klt_track): what the C++ OpticalFlow classes call when the
 * process is one rank of several.  iters (optional) is filled for this rank's block only, 0 elsewhere. */
int ftk_klt_track_sharded(ftk_context *ctx, ftk_comm *comm, int model, const ftk_klt_options *opt, const ftk_pyramid *ref, const ftk_pyramid *cur,
                          const float *ref_uv, float *cur_uv, uint8_t *status, int32_t n, const float *prior, int consider_luminance, int single_level,
                          uint32_t *iters);
/* The two halves of the call above for callers that bring their own collective (e.g. torch.distributed): rank's block
 * tracked into its packed shard (ftk_klt_shard_bytes(n, world) bytes), and the scatter of `world` gathered shards. */
int ftk_klt_track_shard_device(ftk_context *ctx, int32_t rank, int32_t world, int model, const ftk_klt_options *opt, const ftk_pyramid *ref,
                               const ftk_pyramid *cur, const float *d_ref_uv, const float *d_cur_uv_in, const uint8_t *d_status_in, int32_t n,
                               const float *prior, int consider_luminance, int single_level, void *d_packed_shard, uint32_t *d_iters);
int ftk_klt_unpack_shards_device(ftk_context *ctx, const void *d_gathered, int32_t n, int32_t world, float *d_cur_uv_out, uint8_t *d_status_out);
/* ftk_hamming_match_device with the reference rows sharded over the ranks (candidates replicated); d_index_pairs (n_ref
 * entries, in/out as in the single-GPU call) is complete on every rank afterwards. */
int ftk_hamming_match_sharded_device(ftk_context *ctx, ftk_comm *comm, const uint32_t *d_ref_words, int32_t n_ref, const uint32_t *d_cur_words,
                                     int32_t n_cur, int32_t n_words, int32_t n_bits, float max_distance, const float *d_pred_uv,
                                     const float *d_cur_uv, int32_t max_col_distance, int32_t max_row_distance, int32_t *d_index_pairs);

/* ---- descriptor matcher ------------------------------------------------------------------ */

/*
 * Replaces DescriptorMatcher<BriefType>::ForceMatch (descriptor_matcher.h:55-79) and
 * ::NearbyMatch (:90-124) for the per-bit Hamming distance of
 * test/test_descriptor_matcher_brief.cpp:33-45.  Descriptors are bit-packed: n_words uint32
 * per descriptor (any n_words >= 1: widths other than 1, 2, 4, 8, 16 words are zero-padded on the device
 * or take a generic scan — same indices), bit i of the descriptor in bit (i % 32) of word i / 32, unused
 * high bits 0.
 * n_bits == 0 reproduces ComputeDistance's "empty descriptor" answer (kMaxInt32).
 * 256- and 512-bit descriptors (n_words 8 / 16) are compared on the matrix cores (the distances are exact integers out of
 * int8 MFMAs: same indices as the popcount scans that serve the other widths).  Device descriptor pointers are read with 16-byte
 * loads: pass 16-byte-aligned arrays (any hipMalloc'ed buffer, and any row offset into one when n_words is a multiple of 4).
 * pred_uv == NULL selects ForceMatch; otherwise NearbyMatch with the window test
 * |pred.u - cur.u| > max_col_distance || |pred.v - cur.v| > max_row_distance -> skip.
 * index_pairs is in/out (n_ref entries): written only where a candidate beats the threshold,
 * exactly like the reference, whose caller-visible reset to -1 happens only on a size mismatch
 * (descriptor_matcher.h:60-62) and therefore lives in the host-side class.
 * Returns FTK_OK with *matched_ok = 0 when n_cur == 0 (the reference's `return false`).
 */
int ftk_hamming_match(ftk_context *ctx, const uint32_t *ref_words, int32_t n_ref, const uint32_t *cur_words, int32_t n_cur, int32_t n_words,
                      int32_t n_bits, float max_distance, const float *pred_uv, const float *cur_uv, int32_t max_col_distance,
                      int32_t max_row_distance, int32_t *index_pairs, int *matched_ok);

/* Device-resident, asynchronous variant.  d_workspace must hold n_ref uint64 (packed
 * (distance, index) keys); pass NULL to let the context allocate and cache one. */
int ftk_hamming_match_device(ftk_context *ctx, const uint32_t *d_ref_words, int32_t n_ref, const uint32_t *d_cur_words, int32_t n_cur,
                             int32_t n_words, int32_t n_bits, float max_distance, const float *d_pred_uv, const float *d_cur_uv,
                             int32_t max_col_distance, int32_t max_row_distance, int32_t *d_index_pairs, uint64_t *d_workspace);

/*
 * Float descriptors.  Replaces DescriptorMatcher<T>::ForceMatch
 * (descriptor_matcher.h:55-79) / ::NearbyMatch (:90-124) for the cosine distance the reference's
 * SuperPoint / DISK callers define (test/test_descriptor_matcher_superpoint.cpp:32-34,
 * test_descriptor_matcher_disk.cpp:32-34):
 *     0.5f - ref.dot(cur) / ref.norm() / cur.norm() * 0.5f
 * Descriptors are row-major float[n][dim] (256 for SuperPoint, 128 for DISK; any dim <= 4096).
 * The all-pairs contraction runs on the matrix cores in fp16 only to shortlist the pairs that can
 * decide a row; every deciding comparison is made on the distance evaluated in fp32 in Eigen's
 * reduction order, so index_pairs is what the scalar loop returns (ties -> lowest index, strict
 * threshold).  pred_uv == NULL selects ForceMatch.  index_pairs in/out and *matched_ok as in
 * ftk_hamming_match.  NearbyMatch (both matchers): blocks of (reference rows x candidates) whose
 * bounding boxes lie farther apart than the window are skipped — same indices for any order of the
 * features, less time when they are in spatial order (a detector scanning the image).
 */
int ftk_cosine_match(ftk_context *ctx, const float *ref_desc, int32_t n_ref, const float *cur_desc, int32_t n_cur, int32_t dim, float max_distance,
                     const float *pred_uv, const float *cur_uv, int32_t max_col_distance, int32_t max_row_distance, int32_t *index_pairs,
                     int *matched_ok);
/* Device-resident, asynchronous variant (workspace cached in the context). */
int ftk_cosine_match_device(ftk_context *ctx, const float *d_ref_desc, int32_t n_ref, const float *d_cur_desc, int32_t n_cur, int32_t dim,
                            float max_distance, const float *d_pred_uv, const float *d_cur_uv, int32_t max_col_distance,
                            int32_t max_row_distance, int32_t *d_index_pairs);

/* Replaces DescriptorMatcher::FillMatchedPixelByPairIndices (descriptor_matcher.h:135-157).
 * Pure index -> pixel gather on host buffers (O(n_ref), not worth a launch); status is in/out. */
int ftk_fill_matched_pixels(const int32_t *index_pairs, int32_t n_ref, const float *cur_uv, int32_t n_cur, float *matched_uv, uint8_t *status);

/* ---- NNFeatureMatcher: what Match does after the network ----------------------------------- */

/*
 * Replaces the score-matrix branch of NNFeatureMatcher::Match (nn_feature_matcher.cpp:177-215: kLightglueFor*ScoreMat) — not the
 * network in front of it.  scores: float32, logically [batch][n_ref][n_cur], element (b, i, j) at
 * scores[b * batch_stride + i * row_stride + j] (strides in elements; column stride 1; row_stride >= n_cur; pass the
 * [:, :-1, :-1] view of LightGlue's log-assignment tensor to leave its dustbin row and column out).  Per batch item:
 *   col_best[j] = first argmax over i of column j and row_best[i] = first argmax over j of row i, both by the reference's loop
 *   (:188-199, :201-210: start at index 0, replace on a strict >) — so ties go to the lowest index, -0 and +0 tie, a NaN at index 0
 *   keeps its column / row, a NaN elsewhere never wins, all -inf gives 0;
 *   row i is matched iff NOT (row maximum < min_score) (:211: a NaN maximum or a NaN min_score passes) and
 *   col_best[row_best[i]] == i (:212);
 *   match_index[b * n_ref + i] = row_best[i] if matched, else -1; status[...] = FTK_TRACKED if matched, else FTK_LARGE_RESIDUAL
 *   (:156, :214).
 * Bit-identical to the scalar loops for every input: only comparisons are involved.  The matrix is read once.
 * Device entry: asynchronous on `stream` (a hipStream_t; NULL = the legacy default stream), 16-byte loads when d_scores is 16-byte
 * aligned and both strides are multiples of 4, 4-byte loads otherwise (same results).  The context keeps
 * batch * (n_ref + n_cur) + 1 8-byte words of key workspace, left empty by every call; it grows only outside a stream capture
 * (FTK_E_UNSUPPORTED inside one: make one call of the size, or larger, on this context before capturing).  Calls on one context
 * share that workspace: issue them on one stream at a time.  Limits: batch <= 65535, batch * (n_ref + n_cur) < 2^31.
 * n_ref == 0 (or batch == 0) writes nothing and returns FTK_OK — the host entry with *matched_ok = 0, the reference's `return false`
 * (:92).  n_cur == 0 with n_ref > 0 is FTK_E_INVALID_ARGUMENT: the reference would read scores(0) of an empty row (a departure
 * from undefined behaviour).
 */
int ftk_nn_match_scores_device(ftk_context *ctx, void *stream, const float *d_scores, int32_t batch, int32_t n_ref, int32_t n_cur, int64_t row_stride,
                               int64_t batch_stride, float min_score, int32_t *d_match_index, uint8_t *d_status);
/* Host arrays in and out, synchronous; *matched_ok as in ftk_hamming_match. */
int ftk_nn_match_scores(ftk_context *ctx, const float *scores, int32_t batch, int32_t n_ref, int32_t n_cur, int64_t row_stride, int64_t batch_stride,
                        float min_score, int32_t *match_index, uint8_t *status, int *matched_ok);

/*
 * Replaces the match-list branch (nn_feature_matcher.cpp:158-174: kLightglueFor*Matches).  matches: int64 [n_matches][2] rows of
 * (idx_ref, idx_cur).  Row k is applied iff 0 <= idx_ref < min(n_ref, n_cur) and 0 <= idx_cur < n_cur: the reference bounds idx_ref
 * by the size of matched_pixel_uv_cur (n_cur entries, :169) and then writes status[idx_ref] (n_ref entries, :172), so the
 * intersection is the largest range in which it is defined (a departure from undefined behaviour).  Of several applied rows with
 * one idx_ref the one with the largest k wins, as in the sequential loop.  Outputs as above (one batch item).  n_matches < 2^31 - 1.
 */
int ftk_nn_match_list_device(ftk_context *ctx, void *stream, const int64_t *d_matches, int32_t n_matches, int32_t n_ref, int32_t n_cur,
                             int32_t *d_match_index, uint8_t *d_status);
int ftk_nn_match_list(ftk_context *ctx, const int64_t *matches, int32_t n_matches, int32_t n_ref, int32_t n_cur, int32_t *match_index, uint8_t *status,
                      int *matched_ok);

/*
 * The pixel fill of both branches on the device (:157, :171, :213).  matched_uv has n_CUR entries of (u, v), as the reference's
 * `matched_pixel_uv_cur = pixel_uv_cur`: entry t becomes cur_uv[match_index[t]] where t < n_ref and 0 <= match_index[t] < n_cur,
 * and cur_uv[t] otherwise.  In score mode the reference writes matched_pixel_uv_cur[idx_ref] without a bounds test, which is
 * undefined for idx_ref >= n_cur: here such a row keeps its match_index and status and its pixel is not written (a departure from
 * undefined behaviour).  d_matched_uv must not alias d_cur_uv.
 */
int ftk_nn_fill_pixels_device(ftk_context *ctx, void *stream, const int32_t *d_match_index, int32_t n_ref, const float *d_cur_uv, int32_t n_cur,
                              float *d_matched_uv);

#ifdef __cplusplus
}
#endif
#endif /* FTK_H_ */
