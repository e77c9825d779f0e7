// match_plan.h — the launch plans of the Hamming matcher, the cosine matcher and the direct method, as klt_plan.h is the trackers':
// pure functions of values (no context, no environment, no HIP call; tests/test_match_plan_cpu.py walks them without a device).
// The entry points (ftk_match.cpp, ftk_direct.cpp, ftk_nn.cpp) parse the FTK_* overrides, plan, hold the buffers the plan asks for; the launchers carry it out.
#pragma once

#include <limits.h>

#include "ftk_device.h"

namespace ftk {

constexpr int kPlanNotSet = INT_MIN;  // an override that is not in the environment, or an input not known yet

// ---- Hamming matcher (matcher_kernels.hip) ----
struct HammingPlanInput {
    int32_t n_ref, n_cur, n_words, n_bits;  // n_ref, n_cur, n_words >= 1; 0 <= n_bits <= 32 n_words
    int nearby;       // prediction windows given (NearbyMatch)
    int keys_given;   // the caller supplied the keys workspace
    int small;        // FTK_MATCH_SMALL (atoi; 0: never the one-launch form), or kPlanNotSet
    int kernel;       // FTK_MATCH_KERNEL: 1 "mfma", 0 any other value, or kPlanNotSet
};
enum class HammingForm { Small, Plain, Popcount, MatrixCores, Generic };
struct HammingPlan {
    HammingForm form;
    int32_t dev_words;  // the width the kernels read (hamming_device_words; the device entry zero-pads narrower descriptors to it first)
    int32_t cur_per_block, keys_clean, matrix_cores;
    size_t n_boxes;     // NearbyMatch boxes held for the call (0: none)
    // box_grid.x / epilogue_grid.x 0: no such launch; the box and epilogue blocks are kMatchBlock
    dim3 box_grid, scan_grid, scan_block, epilogue_grid;
};
// The register-tiled scans exist for 1, 2, 4, 8 and 16 words: narrower widths are zero-padded to the next of them (equal pad bits in
// both sets: same distances); wider descriptors take the generic scan at their own width.
int32_t hamming_device_words(int32_t n_words);
HammingPlan hamming_plan(const HammingPlanInput &in);

// ---- cosine matcher (float_matcher_kernels.hip) ----
struct CosinePlanInput {
    int32_t n_ref, n_cur, dim;  // n_ref, n_cur >= 1; 1 <= dim <= 4096
    int nearby;
    int aligned16;               // both descriptor pointers are 16-byte aligned
    int small, chunked, splits;  // FTK_COSINE_SMALL / _CHUNKED / _SPLITS (atoi), or kPlanNotSet
};
enum class CosineForm { Small, RegisterStationary, Chunked };
struct CosinePlan {
    CosineForm form;
    int32_t dim_pad, n_ref_pad, n_cur_pad, splits, tiles_per_split;
    // shortlist margin on the distance: kCosineMargin up to dim_pad 256, + kCosineMarginPerK per component beyond (the error budget in
    // float_matcher_kernels.hip, which grows with the width); both contraction forms and the recheck's admission cut use it
    float margin;
    // workspace: byte offsets of the regions (256-byte aligned); [row_max, clear_end) is zeroed by one memset per call
    size_t ref_h, cur_h, ref_norm, cur_norm, cur_bias, cur_info, tile_box, ref_irregular, row_max, cand_count, irregular_count, clear_end,
        cand, cand_score, irregular_list, ws_bytes;
    bool use_tile_box;
    int32_t ref_stationary;         // dim_pad <= 256 and not forced chunked (also the small form's note); uses the cand_score region
    bool packet_prep;               // cosine_prep_pair_kernel (else cosine_prep_kernel); block 256
    dim3 prep_grid, box_grid;       // x 0: no such launch; box: cosine_tile_box_kernel, block 64
    dim3 grid, block;               // the small kernel, the register-stationary kernel or each of the chunked pair
    size_t lds;
    dim3 recheck_grid;              // block 256; x 0: no recheck
};
CosinePlan cosine_plan(const CosinePlanInput &in);

// ---- direct method (direct_kernels.hip) ----
struct DirectPlanInput {
    int32_t n_problems;
    uint32_t max_features;  // tracked features of the largest problem
    int32_t patch_rows, patch_cols;
    int method, tree;
    int spread_allowed;        // 0: the re-run of a poisoned spread launch
    int resident;              // spread workgroups the device holds at once, or kPlanNotSet (not asked yet)
    int capturing;             // the stream is being captured (1 / 0), or kPlanNotSet (not asked yet)
    size_t spread_bytes_held;  // the context's spread workspace
    int spread, resident_cap, poison;  // FTK_DIRECT_SPREAD / _RESIDENT / _POISON (atoi), or kPlanNotSet
    long long min_terms;               // FTK_DIRECT_SPREAD_MIN_TERMS (atoll), or kPlanNotSet
};
struct DirectPlan {
    bool ask_resident, ask_capturing;  // that input decides: fill it in and plan again
    bool feat_in_global;
    size_t feat_bytes;     // per problem, when the feature table lives in device memory
    int32_t producers;     // spread over the chip: producer workgroups per problem (0: one workgroup per problem)
    size_t ws_stride, clear_bytes;  // spread workspace per problem and its head zeroed before the launch
    int32_t poison;
    dim3 grid, block;
    size_t lds;
};
DirectPlan direct_plan(const DirectPlanInput &in);

// ---- NNFeatureMatcher post-processing (nn_match_kernels.hip) ----
struct NnMatchPlanInput {
    int32_t batch, n_ref, n_cur;        // all >= 1
    long long row_stride, batch_stride;  // elements
    int aligned16;                       // the base pointer is 16-byte aligned
};
struct NnMatchPlan {
    bool ok;             // false: the problem does not fit a launch (batch > kNnMaxBatch, or 2^31 tiles / key indices); nothing else is set
    int32_t vec4;        // 16-byte loads (aligned base, row and batch strides multiples of 4 elements), else 4-byte loads
    int32_t tile_rows;   // a multiple of kNnTileRowsMin up to kNnTileRowsMax; tile columns are kNnTileCols
    int32_t row_tiles, col_tiles;
    size_t key_count;    // workspace, in 8-byte words: batch * n_ref row keys, batch * n_cur column keys, one counter word
    dim3 grid, block;    // the pass: x = row_tiles * col_tiles (column tile fastest), y = batch
    dim3 epilogue_grid;  // block kNnBlock, one thread per (batch item, reference row)
};
NnMatchPlan nn_match_plan(const NnMatchPlanInput &in);

}  // namespace ftk
