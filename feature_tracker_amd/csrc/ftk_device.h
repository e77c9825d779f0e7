// ftk_device.h — structures shared between the host-side C ABI (the ftk_*.cpp files) and the gfx950
// kernels (klt_kernels.hip, matcher_kernels.hip, pyramid_kernels.hip).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/ftk.h"

namespace ftk {

constexpr int kWave = 64;  // lanes of a wavefront

// Floats per pixel group (4 pixels x 24 sums + one float4 of padding) of the non-fast affine variants' product layout
// (klt_kernels.hip affine_all_terms); the host sizes KltParams::terms_floats with it.
constexpr int kAffineTermsGroupFloats = 4 * 24 + 4;
constexpr int kAffineTermsRoundGroups = 4;  // groups are allocated in whole prefetch rounds of the chain (klt_kernels.hip FTK_CHAIN_ROUND)

struct DevImage {
    const uint8_t *data;
    int32_t rows;
    int32_t cols;
};

// Kernel argument block of one KLT launch (passed by value: ~450 B of SGPR-loadable constants).
struct KltParams {
    DevImage ref[FTK_MAX_LEVELS];
    DevImage cur[FTK_MAX_LEVELS];
    int32_t n_levels;      // levels actually walked (1 in single-level mode)
    int32_t single_level;  // TrackSingleLevel semantics
    const float *ref_uv;
    const float *cur_uv_in;
    float *cur_uv_out;
    const uint8_t *status_in;
    uint8_t *status_out;
    uint32_t *iters;       // may be null
    const int32_t *order;  // may be null: launch slot -> feature index (a permutation of [0, n) made by an earlier launch's sort block)
    uint32_t *sched_iters; // may be null: iteration counts kept by the context for the launch order of later calls
    // Position-keyed slot swaps (klt_order.h klt_resolve_feature), all null / 0 when off: a coarse grid over the level-0 image in
    // which every feature leaves its iteration count, tagged with the call number; one claim word per launch slot; this call's number
    uint32_t *sched_grid;
    uint32_t *sched_claim;
    uint32_t *sched_flags;  // [2]: (call number << 1 | "the counts that call sorted had no tail"), written by the sort block of a launch
    uint32_t sched_call;
    // the call's longest feature, reported for the next call's wave policy (klt_order.h tail_report; null: not reported)
    uint32_t *tail_dev;
    uint32_t *tail_host;
    uint32_t tail_call;
    int32_t long_tail;          // host-side note: this variant's recent calls had a feature of many iterations (klt_plan.cpp; nothing reads it back)
    const uint32_t *sort_iters;  // may be null: the previous call's counts; one extra workgroup (block 0) sorts them ...
    int32_t *sort_order_out;     // ... into this permutation, longest first (klt_order.h, klt_order_block)
    const float *sort_ref_uv;    // reference positions the sort block may use for the spatial (tile) order: ref_uv, or null when this
                                 // launch's outputs overwrite them (in-place position buffer: the two passes of the sort would disagree)
    int32_t n;             // features in the buffers
    uint32_t n_track;      // min(n, kMaxTrackPointsNumber)
    uint32_t max_iteration;
    uint32_t max_large_step;
    int32_t half_rows, half_cols;
    float converge;
    float prior[4];
    int32_t consider_luminance;
    // derived patch geometry
    int32_t patch_rows, patch_cols, P, Ppad;  // Ppad = P rounded up to a multiple of 16
    int32_t ex_rows, ex_cols, E;
    int32_t a0_floats;  // size of the first LDS array: max(E padded, axis tables)
    uint32_t magic_pc;   // ceil(2^32 / patch_cols): row = umulhi(p, magic_pc)
    uint32_t magic_pc20; // ceil(2^20 / patch_cols) when P * patch_cols < 2^20 (row = (p * magic_pc20) >> 20 on the 24-bit multiplier), else 0
    uint32_t magic_exc;  // ceil(2^32 / ex_cols)
    // LDS image windows (16-bit pixel pairs): reference footprint and current footprint + margin
    int32_t rwin_rows, rwin_cols;
    int32_t cwin_rows, cwin_cols, cwin_margin;
    uint32_t magic_rwc, magic_cwc;  // division by window cols
    uint32_t magic_rwq, magic_cwq;  // division by window cols / 4
    int32_t waves_per_feature;  // workgroup = 64 * waves_per_feature lanes
    int32_t px_floats;          // per-pixel floats behind a0 in the generic kernel's LDS carve: 3, 4 (one float4 record: non-fast affine) or 6 (chunked LSSD)
    int32_t quad_chain;         // chunked one-wave LSSD levels: 1 = the exact-order sums through the DPP network (klt_chain.h "quad chain": fewer
                                // instructions on a lone feature's critical path), 0 = one lane per sum (fewer LDS bytes and plain adds: better when
                                // the launch oversubscribes the chip — config 4: 136 against 141 us, with luminance 255 against 285)
    int32_t terms_floats;       // floats of the generic kernel's `terms` LDS region: K * Ppad, or the 64-pixel ring of a chunked variant
    int32_t lssd_chunked;       // LSSD fast, one wave per feature, no luminance scaling: chunked sweep / chain (klt_kernels.hip)
    int32_t features_per_group; // > 1 (only with waves_per_feature == 1): that many one-wave features share a workgroup, without
                                // meeting at a barrier (lifts the 16-workgroups-per-CU cap on resident one-wave features)
    int32_t group_lds_stride;   // bytes between the LDS carves of the features of a group (klt_plan)
    // pipelined Basic-KLT inverse kernel (klt_basic_kernels.hip); pb_enabled = 0 selects the generic kernel
    int32_t pb_enabled;
    int32_t pb_rwin_rows, pb_rwin_cols;  // reference window incl. the rounding row / column: 2h+5 (cols padded to 4)
    int32_t pb_cap_r, pb_cap_c;          // lattice node capacity per axis: len + 2 + provable maximum of extras
    int32_t fk_enabled;                  // the one-wave `fast` kernels (klt_fast_kernels.hip); 0 selects the generic kernel
    // Patches whose per-pixel arrays exceed a workgroup's 160 KB of LDS (the reference has no patch-size ceiling: optical_flow.h:24-25
    // takes any int32 half size): the generic kernel with its product rows, extended patch, per-pixel records and flags in a
    // per-workgroup slice of device memory instead (L2-resident at these sizes); sums, counts and — where they fit — the image
    // windows stay in LDS.  Same code, same arithmetic; only the address space of those arrays differs (klt_kernels.hip SPILL).
    int32_t spill;
    float *spill_base;                   // spill_stride_floats floats per workgroup (launch slot)
    uint32_t spill_stride_floats;
    int32_t tree;                        // 0: sums in the reference's order (the contract); 1: throughput mode — the same per-pixel products, summed
                                         // by per-lane partials + a cross-lane butterfly (ftk_set_reduction_mode; reported, never the default)
    int32_t scale_recip;                 // 1: n_levels - 1 <= 30, so the coarsest level's 2^-(n_levels - 1) is a normal float and a kernel may multiply by
                                         // it where it would divide by 2^(n_levels - 1) (klt_basic_kernels.hip; set by klt_plan_call)
    int32_t pb_rwin_pitch, pb_cwin_pitch;  // the pipelined kernel keeps its windows as plain BYTES: row pitch in bytes (klt_byte_pitch), a power of two
};

// ceil(2^32 / d): row = umulhi(index, magic)
__host__ __device__ constexpr uint32_t klt_div_magic(int32_t d) { return d <= 1 ? 0u : (uint32_t)(((1ull << 32) + (uint64_t)d - 1) / (uint64_t)d); }

// Byte windows of the pipelined Basic kernel (klt_basic_kernels.hip).  Byte (r, c) of a window is img[clamp(r_lo + r)][clamp(c_lo + c)];
// the 2x2 neighbourhood of element (r, c), c < cols, is bytes c, c + 1 of rows r, r + 1, so a row holds cols + 1 bytes that are read.
// The pitch is that rounded up to a multiple of 8 (a row is staged in 8-byte units) and then to a power of two (unit -> row and
// position are a shift and a mask).  The windows live in the regions carved for 16-bit pairs, 2 * pad4(rows * cols) bytes.  The power of
// two always fits them: cols is a multiple of 4 and >= 8, and with 2^k <= cols < 2^(k + 1) the pitch is at most 2^(k + 1) <= 2 * cols.
// (klt_byte_windows_ok states it as a check: a static_assert of the compile-time geometries, a condition of the form in the plan.)
__host__ __device__ constexpr int32_t klt_byte_window_room(int32_t rows, int32_t cols) { return 2 * ((rows * cols + 3) & ~3); }
__host__ __device__ constexpr int32_t klt_byte_pitch(int32_t cols) {
    const int32_t pitch8 = (cols + 1 + 7) & ~7;
    int32_t pow2 = 8;
    while (pow2 < pitch8) {
        pow2 *= 2;
    }
    return pow2;
}
// Image byte offset of 8-byte unit idx of a window relative to the window's origin: row idx >> shift, position idx & mask, with
// shift = log2(pitch / 8).  The one place that says where a unit comes from (klt_stage.h issue_octets; klt_plan_cli prints it).
__host__ __device__ constexpr uint32_t klt_byte_unit_offset(uint32_t idx, int shift, uint32_t im_cols) {
    return (idx >> shift) * im_cols + 8u * (idx & ((1u << shift) - 1u));
}
__host__ __device__ constexpr int klt_byte_units_shift(int32_t pitch) {
    int shift = 0;
    while ((8 << shift) < pitch) {
        ++shift;
    }
    return shift;
}
// The staging rule of a byte window: every 8-byte unit of every row — bytes [c_lo, c_lo + pitch) of image rows [r_lo, r_lo + wrows) —
// lies inside the level's rows * cols bytes AND inside its own image row.  (r_lo <= rows - wrows has no sum that could overflow.)
__host__ __device__ constexpr bool klt_byte_window_inside(int32_t im_rows, int32_t im_cols, int32_t r_lo, int32_t c_lo, int32_t wrows, int32_t pitch) {
    return r_lo >= 0 && c_lo >= 0 && r_lo <= im_rows - wrows && c_lo <= im_cols - pitch;
}

// Everything in KltParams that follows from (half_rows, half_cols) ALONE.  One definition for the host (klt_plan) and
// for the kernels' compile-time specialisations (klt_basic_kernels.hip instantiates the pipelined kernel for the common patch
// sizes: the geometry then folds into immediates instead of living in ~40 SGPRs, most of them spilled to vector lanes).
__host__ __device__ constexpr void klt_fill_geometry(KltParams &p) {
    p.patch_rows = 2 * p.half_rows + 1;
    p.patch_cols = 2 * p.half_cols + 1;
    p.P = p.patch_rows * p.patch_cols;
    p.Ppad = (p.P + 15) & ~15;  // (a multiple of 16 since round 5: the quad chains add 16 terms per step, klt_chain.h; the padding holds exact zeros)
    p.ex_rows = p.patch_rows + 2;
    p.ex_cols = p.patch_cols + 2;
    p.E = p.ex_rows * p.ex_cols;
    const int32_t epad = (p.E + 3) & ~3, tables = 12 * (p.patch_rows + p.patch_cols);
    p.a0_floats = epad > tables ? epad : tables;
    p.magic_pc = klt_div_magic(p.patch_cols);
    // the same division on the full-rate 24-bit multiplier when it is exact over the whole patch: x * (M * d - 2^20) < 2^20 for all x < P
    p.magic_pc20 = (p.patch_cols > 1 && (long long)p.P * p.patch_cols < (1ll << 20) && p.P < (1 << 12))
                       ? (uint32_t)(((1u << 20) + (uint32_t)p.patch_cols - 1) / (uint32_t)p.patch_cols) : 0u;
    p.magic_exc = klt_div_magic(p.ex_cols);
    p.rwin_rows = p.patch_rows + 3;
    p.rwin_cols = (p.patch_cols + 3 + 3) & ~3;  // pixel-pair columns, rounded up to a multiple of 4 (8-byte LDS stores)
    p.cwin_margin = 2;
    p.cwin_rows = p.rwin_rows + 2 * p.cwin_margin;
    p.cwin_cols = (p.patch_cols + 3 + 2 * p.cwin_margin + 3) & ~3;
    p.magic_rwc = klt_div_magic(p.rwin_cols);
    p.magic_cwc = klt_div_magic(p.cwin_cols);
    p.magic_rwq = klt_div_magic(p.rwin_cols / 4);
    p.magic_cwq = klt_div_magic(p.cwin_cols / 4);
    p.pb_rwin_rows = p.patch_rows + 4;
    p.pb_rwin_cols = (p.patch_cols + 4 + 3) & ~3;
    p.pb_rwin_pitch = klt_byte_pitch(p.pb_rwin_cols);
    p.pb_cwin_pitch = klt_byte_pitch(p.cwin_cols);
    // lattice extras per axis: a unit step crosses at most log2(len + 2) + 3 binade boundaries, two nodes each
    int bits_r = 0, bits_c = 0;
    while ((1 << bits_r) < p.patch_rows + 2) {
        ++bits_r;
    }
    while ((1 << bits_c) < p.patch_cols + 2) {
        ++bits_c;
    }
    p.pb_cap_r = p.patch_rows + 2 + 2 * (bits_r + 3);
    p.pb_cap_c = p.patch_cols + 2 + 2 * (bits_c + 3);
}

// What the pipelined kernel needs of its byte windows: a power-of-two pitch that covers cols + 1 bytes, inside the carved region.
__host__ __device__ constexpr bool klt_byte_window_ok(int32_t rows, int32_t cols, int32_t pitch) {
    return pitch >= cols + 1 && (pitch & (pitch - 1)) == 0 && pitch % 8 == 0 && rows * pitch <= klt_byte_window_room(rows, cols);
}
__host__ __device__ constexpr bool klt_byte_windows_ok(const KltParams &p) {
    return klt_byte_window_ok(p.pb_rwin_rows, p.pb_rwin_cols, p.pb_rwin_pitch) && klt_byte_window_ok(p.cwin_rows, p.cwin_cols, p.pb_cwin_pitch);
}

// (the trackers' launch plan, per-form LDS sizes, kernel pickers and klt_launch: klt_plan.h)
// Launch order of THIS call from the position table the last call wrote (klt_kernels.hip): order[slot] = feature, predicted-longest
// first.  last_table: 2^16 words; pred: n bytes; hist_and_cursor: kSchedOrderWords (klt_sched.h) words (zeroed here).
hipError_t klt_position_order_launch(const float *ref_uv, int32_t n, const uint32_t *last_table, uint32_t last_call, uint8_t *pred, uint32_t *hist_and_cursor,
                                     int32_t *order, hipStream_t stream);
// Lane-parallel 6x6 LDLT (klt_ldlt.h) on n systems, one wave each: the test hook behind ftk_ldlt6_solve.
hipError_t ldlt6_launch(const float *d_a, const float *d_b, float *d_x, int n, hipStream_t stream);

// Reference descriptors a thread of the register-tiled Hamming scan keeps in registers (a 256-thread workgroup covers
// 256 * kMatchRefs reference rows); the host sizes its grid and its NearbyMatch boxes with the same number.
constexpr int kMatchBlock = 256;  // threads of every Hamming-matcher workgroup except the matrix-core scan's one wave
constexpr int kMatchRefs = 2;
constexpr int kMatchRowsPerBlock = kMatchBlock * kMatchRefs;
constexpr int kMfmaRows = 64;  // reference rows per workgroup of the matrix-core scan: ONE wave (nothing is shared, so nothing is
                               // gained by larger groups, and single waves pack the SIMDs' two slots evenly)
constexpr int kMfmaTile = 32;  // candidates per tile of the matrix-core scan (one v_mfma_i32_32x32x32_i8)
constexpr int kMfmaMaxTilesPerSplit = 1024;  // the position field of the matrix-core scan's running keys
// The one-launch form (hamming_match_small_kernel) up to n_ref * n_cur * n_words = kSmallMatchWork while a row's walk stays at or below
// n_cur * n_words = kSmallMatchRowWork; the packed key holds the candidate in 20 bits, kSmallNoIndex = "none"
constexpr long long kSmallMatchWork = 32ll << 20;
constexpr int kSmallMatchRowWork = 24576;
constexpr int kSmallNoIndex = 0xFFFFF;

struct MatchParams {
    const uint32_t *ref_words;
    const uint32_t *cur_words;
    const float *pred_uv;  // null => ForceMatch
    const float *cur_uv;
    int32_t *index_pairs;
    unsigned long long *keys;  // workspace: n_ref packed (distance << 32 | index)
    int32_t n_ref, n_cur, n_words, n_bits;
    float max_distance;
    float max_col, max_row;
    int32_t cur_per_block;  // candidates scanned by one workgroup
    int32_t keys_clean;     // keys already hold "no match" (context-owned workspace: the epilogue leaves it that way)
    int32_t matrix_cores;   // 1: the scan on the matrix cores (hamming_match_mfma_kernel; n_words 8 / 16)
    float4 *boxes;          // NearbyMatch, optional: ceil(n_ref / 512) prediction boxes, then one candidate box per split
                            // ({u min, u max, v min, v max}; hamming_box_kernel fills them, the scan leaves early on them)
};
struct HammingPlan;
hipError_t match_launch(const HammingPlan &plan, const MatchParams &p, hipStream_t stream);

// Float-descriptor (cosine distance) matcher: float_matcher_kernels.hip.
constexpr int kCosineCandCap = 64;       // candidates kept per ref row before the row falls back to the exact scan
constexpr int kCosineIrregularCap = 64;  // cur rows with a zero / non-finite / extreme norm kept in the side list
constexpr int kCosineTile = 128;  // rows of one operand tile of the chunked kernel (cur: MFMA rows, ref: MFMA columns)
constexpr int kRrTile = 64;       // cur rows per step of the register-stationary kernel (and per NearbyMatch tile box)
constexpr int kRrRows = 512;      // ref rows per workgroup of the register-stationary kernel
// Candidates per row up to which a call runs as ONE exact launch (cosine_match_small_kernel: a wave walks its row's candidates
// alone, so its time grows with n_cur); measured against the multi-launch pipeline per shape
constexpr int kCosineSmallCurNearby = 2048;  // 300 x 300 x 256 NearbyMatch 48.7 -> 10.7 us, 1 000 x 1 000 47.4 -> 21.3, 2 000 x 2 000 54.6 -> 40.3 (3 000 candidates: even)
constexpr int kCosineSmallCurForce = 384;    // ForceMatch computes every pair exactly: 100 x 100 x 256 35.4 -> 14.8 us, 300 x 300 40.3 -> 32.1, 600 x 600 41.6 -> 59.2 (not taken)
constexpr int kCosineSmallRefMax = 4096;
// Shortlist margin on the distance (band 2 * margin on the approximate cosine): the error budget in the header of
// float_matcher_kernels.hip.  Constant up to dim_pad 256 (the register-stationary kernel compiles it in); cosine_plan lets it grow
// with dim_pad above that, where the accumulation terms of the budget would otherwise use up the slack.
constexpr float kCosineMargin = 1.5e-3f;
constexpr float kCosineMarginPerK = 1.75e-7f;  // added per descriptor component beyond 256
struct CosineParams {
    const float *ref, *cur;   // [n][dim] fp32 descriptors, row-major
    const float *pred_uv;     // null => ForceMatch
    const float *cur_uv;
    int32_t *index_pairs;
    // workspace (see ftk_cosine_workspace_bytes)
    _Float16 *ref_h, *cur_h;  // unit-length fp16 copies, [n_pad][dim_pad], zero padded
    float *ref_norm, *cur_norm, *cur_bias;
    float4 *cur_info;         // {bias, u, v, 0} per (padded) cur row: what cosine_gemm_rr_kernel streams beside the tile
    float4 *tile_box;         // NearbyMatch: {u min, u max, v min, v max} of every 64-row cur tile (cosine_tile_box_kernel); null: not used
    uint8_t *ref_irregular;
    uint32_t *row_max, *cand_count;
    int32_t *cand;            // [n_ref_pad][kCosineCandCap]
    float *cand_score;        // approximate score of each entry; non-null selects the single-walk contraction (ref-stationary only)
    uint32_t *irregular_count;
    int32_t *irregular_list;  // [kCosineIrregularCap]
    void *clear_begin;        // row_max | cand_count | irregular_count, contiguous: zeroed by one memset per call
    size_t clear_bytes;
    int32_t n_ref, n_cur, dim, n_ref_pad, n_cur_pad, dim_pad;
    int32_t tiles_per_split;  // cur tiles (128 rows) walked by one workgroup of the chunked kernel
    int32_t ref_stationary;   // dim_pad <= 256: cosine_gemm_rr_kernel (ref fragments in registers; n_ref_pad % 512 == 0,
                              // n_cur_pad % 64 == 0, `splits` workgroups share the cur tiles evenly); 0: the chunked kernel
    int32_t splits;
    float max_distance, max_col, max_row;
    float margin;             // CosinePlan::margin
};
size_t cosine_rr_lds_bytes(int dim_pad);
struct CosinePlan;
hipError_t cosine_match_launch(const CosinePlan &plan, const CosineParams &p, hipStream_t stream);

// DirectMethod (direct_kernels.hip): one workgroup per pose problem; all problems of a launch share
// the pyramid depth and the options.
struct DirectProblem {
    DevImage ref[FTK_MAX_LEVELS];
    DevImage cur[FTK_MAX_LEVELS];
    float K[4];             // fx, fy, cx, cy at full resolution
    const float *p_ref;     // n x 3: points in the reference camera frame
    const float *ref_uv;    // n x 2
    float *cur_uv;          // n x 2, in/out
    float *pose;            // 7: q_rc (w, x, y, z), p_rc — in/out
    uint8_t *status;        // n, in/out
    uint32_t *iterations;   // optional: Gauss-Newton iterations over all levels
    int32_t n;
    int32_t status_valid;   // 0: reset every status to kTracked first (direct_method_tracker.cpp:73-75)
    float4 *feat;           // null: the per-feature projection table lives in LDS; else n_track entries of device memory (large problems)
};
constexpr uint32_t kDirectLdsFeatures = 768;  // tracked features whose per-feature table (64 B each) still fits in LDS beside the ring
constexpr int kDmWaves = 8;                   // waves of a direct-method workgroup
struct DirectParams {
    const DirectProblem *problems;  // device memory, one per workgroup
    int32_t tree;                   // throughput mode (ftk_set_reduction_mode): butterfly sums instead of the scalar loop's order
    int32_t n_levels;
    uint32_t max_track_points, max_iteration;
    int32_t half_rows, half_cols, patch_rows, patch_cols;
    float converge;
    int32_t method;
    // ONE problem spread over the chip (direct_kernels.hip direct_track_spread_kernel): `spread` producer workgroups beside the
    // consumer, hand-offs through `spread_ws` (direct_spread_ws_bytes; its first direct_spread_clear_bytes zeroed before the launch)
    int32_t spread;
    uint32_t *spread_ws;
    uint32_t spread_ws_words;  // words between the workspaces of consecutive problems
    int32_t spread_poison;     // tests only (FTK_DIRECT_SPREAD_POISON=1): the consumer behaves as if its first wait had run out — the
                               // launch ends at once with header word 1 set and a NaN pose, as a launch that was not co-resident would
};
size_t direct_lds_bytes(uint32_t max_features);
size_t direct_spread_ws_bytes(uint32_t n_track, int32_t patch_rows, int32_t patch_cols);
size_t direct_spread_clear_bytes(uint32_t n_track, int32_t patch_rows, int32_t patch_cols);
int direct_spread_resident_groups(uint32_t max_features, int device);  // workgroups of the spread kernel the device holds at once (0: unknown)
struct DirectPlan;
hipError_t direct_track_launch(const DirectPlan &plan, const DirectParams &p, hipStream_t stream);

struct BriefParams {
    DevImage img;
    const float *uv;
    uint32_t *words;        // n * n_words, bit i of a descriptor in bit (i % 32) of word i / 32
    const int8_t *pattern;  // 4 offsets per bit, device memory
    int32_t n, n_bits, n_words, half;
};
hipError_t brief_launch(const BriefParams &p, hipStream_t stream);

struct HarrisParams {
    DevImage img;
    short *gx, *gy;                  // rows*cols each
    float *response;                 // rows*cols or null
    unsigned long long *key, *tmp, *wmax;  // rows*cols each (tmp / wmax unused when list is null)
    unsigned long long *list;        // survivors (keys), capacity entries; null = response only
    unsigned *count;
    unsigned capacity;
    int32_t min_distance;
    float min_response;
};
hipError_t harris_launch(const HarrisParams &p, hipStream_t stream);
// Points that already exist (masked detection): point i counts where flags[i] != 0 (flags null: everywhere) and
// ids[i] >= 0 (ids null: everywhere); plane / dilated: rows*cols bytes each of workspace.  n == 0: no masking, no workspace.
struct HarrisOccupied {
    const float *uv;
    const uint8_t *flags;
    const long long *ids;
    int32_t n;
    uint8_t *plane, *dilated;
};
// harris_launch's passes with the occupied points' neighbourhoods taken out of the candidates first; p.list must be set, and
// p.capacity entries suffice when it is the plan's bound (track_table_plan.h).
hipError_t harris_masked_launch(const HarrisParams &p, const HarrisOccupied &o, hipStream_t stream);
// The passes of harris_masked_launch behind the response: any plane of sortable 64-bit keys (score bits << 32 | ~pixel index, 0: no
// candidate) to the list of its survivors (DESIGN.md 5.19's rules).  The keypoint decoder's key plane goes through it too (5.22).
struct KeyPlaneSelectParams {
    int32_t rows, cols, reach;
    unsigned long long *key, *tmp, *wmax;  // rows*cols each
    unsigned long long *list;              // capacity entries
    unsigned *count;
    unsigned capacity;
};
hipError_t key_plane_select_launch(const KeyPlaneSelectParams &p, const HarrisOccupied &o, hipStream_t stream);

// The track table (track_table_kernels.hip, KltVideoTracker): fixed slots, torch-owned.
struct TrackTable {
    long long *ids;        // [n] -1 = empty
    float *points;         // [n][2]
    float *prev_points;    // [n][2]
    uint8_t *status;       // [n]
    int32_t *age;          // [n]
    int32_t *n_live;       // [1]
    long long *next_id;    // [1]
    int32_t n;
};
struct TrackRetireParams {
    TrackTable t;
    const float *tracked_uv;        // [n][2] the forward call's results
    const uint8_t *tracked_status;  // [n]
    const float *back_uv;           // both or neither: the backward call's results
    const uint8_t *back_status;
    float fb_threshold;
    int32_t *free_slots;            // [n] out: the empty slots in ascending order
    int32_t *n_free;                // [1] out
    int32_t per_thread;             // the plan's retire_per_thread
};
struct HarrisRankParams {
    const unsigned long long *list;  // the survivors' keys in any order
    const unsigned *count;           // how many (device word)
    unsigned capacity;
    int32_t cols;
    float *uv_out;                   // detection: [max_count][2], zeroed before the launch; null: fill the table
    int32_t *count_out;
    int32_t max_count;
    float *score_out;                // detection: [max_count] the float the key's upper 32 bits carry, or null
    TrackTable t;                    // fill
    const int32_t *free_slots;
    const int32_t *n_free;
};
struct TrackTablePlan;
hipError_t track_table_retire_launch(const TrackTablePlan &plan, const TrackRetireParams &p, hipStream_t stream);
// Ranks the survivors (rank = survivors with a greater key) and writes rows (uv_out) or table slots; in fill mode a second, one-thread
// launch advances next_id and n_live.
hipError_t harris_rank_launch(const TrackTablePlan &plan, const HarrisRankParams &p, hipStream_t stream);
hipError_t harris_rank_launch(uint32_t rank_blocks, const HarrisRankParams &p, hipStream_t stream);  // the same with the grid alone

// Dense optical flow (dense_flow_kernels.hip, DenseOpticalFlow).  Moments: two float4 per pixel, {S0, Sr, Sc, Src} then {Srr, Scc, 0, 0},
// row-major at the image's own size; flow planes row-major at the ref level's size.
struct DenseMomentsParams {
    DevImage img[2];       // ref, cur of one level
    float4 *mom[2];        // their moment images
    const float *weights;  // (2 half + 1)^2 normalised Gaussian weights, row-major (ftk_dense_flow_gaussian)
    int32_t half;
};
struct DenseFlowParams {
    const float4 *mom_ref;
    const float4 *mom_cur;
    int32_t ref_rows, ref_cols, cur_rows, cur_cols;
    float k2, k4, k22;
    int32_t max_iteration;
    float converge;  // kMaxConvergeStep
    float max_step;  // kMaxDeltaFlowStep
    int32_t init;    // 0: zero flow; 1: init_r / init_c at ref size where flow_valid's bit is set (may alias out_*); 2: upsample init_* (init_rows x init_cols)
    int32_t flow_valid;
    const float *init_r;
    const float *init_c;
    int32_t init_rows, init_cols;
    float *out_r;
    float *out_c;
};
struct DenseMedianParams {
    const float *in_r;
    const float *in_c;
    float *out_r;
    float *out_c;
    int32_t rows, cols;
};
int dense_lds_half();  // largest half patch the moments kernel stages in LDS (above: global reads, same arithmetic)
hipError_t dense_moments_launch(const DenseMomentsParams &p, hipStream_t stream);
hipError_t dense_flow_launch(const DenseFlowParams &p, hipStream_t stream);
hipError_t dense_median_launch(const DenseMedianParams &p, hipStream_t stream);

// RAFT correlation pyramid (raft_corr_kernels.hip, CorrelationPyramid).  One volume buffer: level l at element level_offset[l], laid out
// [B * H * W][level_h[l]][level_w[l]] (ftk_corr_pyramid_layout).
constexpr int kCorrMaxLevels = 16;
struct CorrBuildParams {
    const float *f0;  // [B][C][H][W]
    const float *f1;
    float *volume;
    int32_t B, C, H, W;
    float divisor;  // (float)sqrt((double)C)
    int32_t fused;  // pooled levels the build's epilogue writes (0 .. corr_fused_levels())
    int64_t level_offset[4];
    int32_t level_h[4], level_w[4];
};
struct CorrLookupParams {
    const float *volume;
    const float *coords;  // [B][2][H][W]: x, y
    float *out;           // [B][levels * K][H][W], or per_level: levels blocks of [B][H][W][K]
    int32_t B, H, W, levels, radius, per_level;
    int64_t level_offset[kCorrMaxLevels];
    int32_t level_h[kCorrMaxLevels], level_w[kCorrMaxLevels];
};
int corr_fused_levels();
hipError_t corr_build_launch(const CorrBuildParams &p, hipStream_t stream);
hipError_t corr_pool_launch(const float *src, float *dst, int64_t slabs, int hin, int win, int hout, int wout, hipStream_t stream);
hipError_t corr_lookup_launch(const CorrLookupParams &p, hipStream_t stream);

// RAFT's on-demand correlation (raft_corr_ondemand_kernels.hip, OnDemandCorrelation): no volume.  One workspace: fmap0
// transposed to [B][H * W][C] at element 0, fmap1's level l channel-last as [B][level_h[l]][level_w[l]][C] at level_offset[l]
// (ftk_corr_ondemand_layout).  The grids are raft_corr_ondemand_plan's (raft_corr_ondemand_plan.h).
struct CorrOdTransposeParams {
    const float *f0;  // [B][C][H * W]
    const float *f1;
    float *out0;      // [B][H * W][C]
    float *out1;
    int32_t B, C;
    int64_t HW;
};
struct CorrOdPoolParams {
    const float *src;  // [B][hin][win][C]
    float *dst;        // [B][hin / 2][win / 2][C]
    int32_t B, C, hin, win;
};
struct CorrOdLookupParams {
    const float *workspace;
    const float *coords;  // [B][2][H][W]: x, y
    float *out;           // [B][levels * K][H][W], or per_level: levels blocks of [B][H][W][K]
    int32_t B, C, H, W, levels, radius, per_level;
    int32_t lattice_side;  // 2r + 2, or 0: every corner directly
    int32_t vector;        // 16-byte loads in the channel chain
    float divisor;         // (float)sqrt((double)C)
    int64_t level_offset[kCorrMaxLevels];
    int32_t level_h[kCorrMaxLevels], level_w[kCorrMaxLevels];
};
hipError_t corr_od_transpose_launch(const CorrOdTransposeParams &p, dim3 grid, dim3 block, hipStream_t stream);
hipError_t corr_od_pool_launch(const CorrOdPoolParams &p, int64_t blocks, hipStream_t stream);
hipError_t corr_od_lookup_launch(const CorrOdLookupParams &p, dim3 grid, dim3 block, hipStream_t stream);

// RAFT's convex flow upsampling (raft_upsample_kernels.hip, Raft.UpsampleFlow): one launch.
constexpr int kFlowUpsampleTile = 32;  // coarse pixels per workgroup along x (FTK_FLOW_UPSAMPLE_TILE)
struct FlowUpsampleParams {
    const float *flow;  // [B][2][H][W]
    const float *mask;  // [B][576][H][W]
    float *out;         // [B][2][8H][8W]
    int32_t B, H, W;
    float mask_scale;
};
// hipErrorInvalidValue when the grid would not fit in 2^31 - 1 workgroups
hipError_t flow_upsample_launch(const FlowUpsampleParams &p, hipStream_t stream);

// Sparse tracking from RAFT's coarse flow (raft_points_kernels.hip): one launch.
constexpr int kFlowPointsTile = 64;  // points per workgroup (FTK_FLOW_POINTS_TILE)
struct FlowPointsParams {
    const float *flow;       // [B][2][H][W]
    const float *mask;       // [B][576][H][W]
    const float *flow_back;  // both or neither: the backward pair of the forward-backward check
    const float *mask_back;
    const float *points;     // [B][N][2] (u = x, v = y)
    float *cur_points;       // [B][N][2]
    uint8_t *status;         // [B][N]
    float *fb_error2;        // [B][N] or null
    int32_t B, H, W, N, image_rows, image_cols;
    float mask_scale, fb_threshold;
};
// hipErrorInvalidValue when the grid would not fit in 2^31 - 1 workgroups
hipError_t flow_track_points_launch(const FlowPointsParams &p, hipStream_t stream);

// The warm start of RAFT on video (raft_warm_kernels.hip, upstream RAFT's forward_interpolate): a scan launch, and with
// more than one split of the sources a gather launch.
constexpr int kFlowWarmTile = 256;               // targets per workgroup and sources per LDS tile (FTK_FLOW_WARM_TILE)
constexpr int kFlowWarmMaxSplits = 32;           // FTK_FLOW_WARM_MAX_SPLITS
constexpr int kFlowWarmMaxPixels = 1 << 20;      // FTK_FLOW_WARM_MAX_PIXELS: the search is exhaustive
constexpr int kFlowWarmFillGroups = 1024;        // the automatic split count aims at this many workgroups: four per compute unit
struct FlowWarmParams {
    const float *flow;              // [B][2][H][W]
    unsigned long long *workspace;  // [splits][B][H * W] keys, or null with one split
    float *out;                     // [B][2][H][W]
    int32_t B, H, W, splits;
    int32_t split_sources;          // sources per split, whole tiles: set by the launch function
};
// The split count ftk_flow_warm_splits reports: ceil(kFlowWarmFillGroups / (B * tiles)) held to 1 .. min(tiles, kFlowWarmMaxSplits).
int flow_warm_auto_splits(int32_t B, int32_t H, int32_t W);
// hipErrorInvalidValue when the grid would not fit in 2^31 - 1 workgroups
hipError_t flow_warm_launch(const FlowWarmParams &p, hipStream_t stream);

// RAFT's separable ConvGRU (raft_gru_kernels.hip, SepConvGru.forward, gru.py:59-76): per pass a gates launch and a
// candidate + blend launch, each an implicit GEMM on the f32-input matrix cores.
// One tensor of an input that is a channel concatenation read in place (the GRU's and conv2d_kernel's segment lists).
struct ChannelSegment {
    const float *data;  // [B][channels][H][W]
    int32_t channels;
};
struct SepConvGruParams {
    ChannelSegment seg[4];    // the input's channel segments in order: the x parts, then h (gates) or r * h (candidate)
    int32_t n_seg;
    const float *weights;  // packed [m_tiles][k_steps][64] (sep_conv_gru_plan.h)
    const float *bias;     // [out_channels]
    const float *h;        // [B][h_channels][H][W]
    float *z;              // gates: written; candidate: read
    float *rh;             // gates: written
    float *out;            // candidate: the new hidden state
    int32_t h_channels, in_channels, B, H, W;
};
struct SepConvGruPlan;
hipError_t sep_conv_gru_launch(const SepConvGruPlan &plan, const SepConvGruParams &p, int kernel_size, int vertical, int gates, hipStream_t stream);

// The stock layers of RAFT's UpdateBlock (raft_conv_kernels.hip, update_block.py:4-67): a stride-1, zero-padded square
// convolution with bias, an optional ReLU and an output scale, as one implicit GEMM on the f32-input matrix cores.
struct ConvParams {
    ChannelSegment seg[3];  // the input's channel segments in order
    int32_t n_seg;
    const float *weights;   // packed [m_tiles][k_steps][64] (raft_conv_plan.h)
    const float *bias;      // [out_channels]
    float *out;             // [B][out_channels][H][W]
    float out_scale;        // the epilogue's last multiply (1: none)
    int32_t out_channels, in_channels, B, H, W;
};
struct ConvPlan;
hipError_t raft_conv_launch(const ConvPlan &plan, const ConvParams &p, int kernel_size, int relu, hipStream_t stream);
// SuperPoint's VGG: the same layer (kernel sizes 1 and 3) with a 2 x 2 max-pool in its epilogue; p.out is [B][out_channels]
// [H / 2][W / 2], p.out_scale is not read.  `plan` is a plan of pool = 1.
hipError_t raft_conv_pool_launch(const ConvPlan &plan, const ConvParams &p, int kernel_size, int relu, hipStream_t stream);
// RAFT's encoders (encoder.py:4-68): the same layer with a stride of 1 or 2 (base.H, base.W the input's sizes), a residual
// added before the ReLU and the image normalisation of model.py:70-71 at the fetch.  Stride 1 with neither is raft_conv_launch itself.
struct ConvStridedParams {
    ConvParams base;
    const float *residual;  // [B][out_channels][OH][OW] or nullptr
    int32_t OH, OW;         // ceil(H / stride) x ceil(W / stride): the plan's out_h, out_w
    int32_t normalise;      // != 0: an in-image input value x is read as 2 (x / 255) - 1
};
hipError_t raft_conv_strided_launch(const ConvPlan &plan, const ConvStridedParams &p, int kernel_size, int relu, hipStream_t stream);

// SuperPoint's dense descriptor map (superpoint_kernels.hip): x [D][cells] to y [cells][D], every cell divided by
// fmaxf(sqrtf(sum of squares over ascending c, an fmaf chain from +0), 1e-12f).  hipErrorInvalidValue when D or cells is not positive or
// the grid (64 cells per workgroup) would not fit in 2^31 - 1 workgroups.
hipError_t channel_normalise_launch(const float *x, float *y, int32_t D, int64_t cells, hipStream_t stream);

// NNFeatureMatcher's post-processing (nn_match_kernels.hip): mutual-best matching of a score matrix, or a match list.
// Keys (unsigned 64-bit, merged with atomicMax, 0 = empty): score mode (order-preserving map of the score << 32 | ~index), so the
// greatest score wins and, among equal scores, the lowest index; list mode ((k + 1) << 32 | idx_cur), so the last row wins.
constexpr int kNnBlock = 256;     // threads of every workgroup of this file
constexpr int kNnTileCols = 256;  // columns of a tile: one 16-byte load per lane of a wave covers a 1 KB row segment
constexpr int kNnTileRowsMin = 16, kNnTileRowsMax = 128;  // rows of a tile (a multiple of 16: four waves x four loads in flight each)
constexpr int kNnMaxBatch = 65535;                        // grid.y
struct NnMatchParams {
    const float *scores;              // [B][n_ref][n_cur] through row_stride / batch_stride (elements), unit column stride
    int64_t row_stride, batch_stride;
    int32_t batch, n_ref, n_cur;
    int32_t tile_rows, col_tiles;
    float min_score;
    unsigned long long *row_key;      // [B][n_ref]
    unsigned long long *col_key;      // [B][n_cur]
    unsigned int *done;               // workgroups of the epilogue that have finished (the last one empties col_key)
    int32_t *match_index;             // [B][n_ref]
    uint8_t *status;                  // [B][n_ref]
};
struct NnMatchPlan;
hipError_t nn_match_scores_launch(const NnMatchPlan &plan, const NnMatchParams &p, hipStream_t stream);
// List mode: row_key holds n_ref entries (empty before and after).
hipError_t nn_match_list_launch(const long long *matches, int32_t n_matches, int32_t n_ref, int32_t n_cur, unsigned long long *row_key,
                                int32_t *match_index, uint8_t *status, hipStream_t stream);
hipError_t nn_fill_pixels_launch(const int32_t *match_index, int32_t n_ref, const float *cur_uv, int32_t n_cur, float *matched_uv, hipStream_t stream);
hipError_t nn_match_warm(hipStream_t stream);

// Scatter of the all-gathered packed tracker shards into (cur_uv, status) in global feature order (ftk_comm.cpp).
hipError_t unpack_klt_shards_launch(const uint8_t *d_gathered, int32_t n, int32_t world, int32_t cap, int64_t shard_bytes, float *d_uv_out,
                                    uint8_t *d_status_out, hipStream_t stream);
hipError_t pyramid_downsample_launch(const uint8_t *src, int32_t src_rows, int32_t src_cols, uint8_t *dst, hipStream_t stream);
// Levels 1 .. n_levels - 1 from level 0 (dst[l] = level l, l >= 1): one fused launch (pyramid_fused_kernel), deeper levels one by one.
// level0_keep (n_levels >= 2): `level0` is a device-visible source outside the pyramid (pinned host memory) and the same launch
// stores it as the pyramid's level 0.
hipError_t pyramid_build_levels_launch(const uint8_t *level0, int32_t rows, int32_t cols, uint8_t *const *dst, int32_t n_levels, hipStream_t stream,
                                       uint8_t *level0_keep = nullptr);
hipError_t extract_patch_launch(DevImage ref, float u, float v, int32_t ex_rows, int32_t ex_cols, float *d_patch, uint8_t *d_valid,
                                uint32_t *d_count, hipStream_t stream);

hipError_t klt_fast_warm(hipStream_t stream);

// One empty launch per translation unit: loads its code object (ftk_warmup).
hipError_t klt_warm(hipStream_t stream);
hipError_t klt_basic_warm(hipStream_t stream);
hipError_t matcher_warm(hipStream_t stream);
hipError_t cosine_warm(hipStream_t stream);
hipError_t direct_warm(hipStream_t stream);
hipError_t pyramid_warm(hipStream_t stream);
hipError_t feature_warm(hipStream_t stream);
hipError_t dense_warm(hipStream_t stream);

}  // namespace ftk
