// match_assignment_plan.h — the launch plan and workspace layout of LightGlue's assignment head (match_assignment_kernels.hip,
// DESIGN.md 5.23), as keypoint_decode_plan.h is the keypoint decoder's: a pure function of values (no context, no environment, no HIP
// call; tests/test_match_assignment_args_cpu.py walks it without a device through host/build/match_assignment_plan_cli).
// ftk_match_assignment.cpp plans, the launcher carries the plan out.
#pragma once

#include "ftk_device.h"
#include "ftk_layout.h"

namespace ftk {

constexpr int kAssignMaxRows = 4096;     // FTK_MATCH_ASSIGNMENT_MAX_ROWS: M, N
constexpr int kAssignMaxDim = 1024;      // FTK_MATCH_ASSIGNMENT_MAX_DIM: D
constexpr int kAssignGemmWaves = 4;      // waves of a GEMM workgroup, each with its own 32 rows
constexpr int kAssignGemmTileRows = 32 * kAssignGemmWaves;
constexpr int kAssignGemmTileCols = 128;  // 4 MFMA column tiles per wave
constexpr int kAssignNormThreads = 64;   // one wave per row, or per block of columns
constexpr int kAssignNormCols = 16;      // columns of a column block: a 64-row tile is 16 loads of 4 rows x 16 columns
constexpr int kAssignNormLdsStride = kAssignNormCols + 1;  // floats between the LDS rows of a tile: a transposed read is conflict-free
constexpr int kAssignFinishThreads = 256;  // columns of a finish workgroup
constexpr int kAssignFinishRows = 8;     // rows of a finish workgroup

struct MatchAssignmentPlanInput {
    int32_t rows0, rows1;   // M, N
    int32_t dim;            // D
    int32_t with_weights;   // 0: descriptors as they are, times scale
    int64_t row_stride;     // floats between rows of the output; 0: N + 1
    int32_t aligned16;      // every descriptor / weight pointer is 16-byte aligned
};
enum class MatchAssignmentRefusal { None, Rows, Dim, Stride };
struct MatchAssignmentPlan {
    MatchAssignmentRefusal refused;  // not None: nothing else is set
    int64_t row_stride;
    int32_t vec;                     // rows are read four channels at a time (D % 4 == 0 and aligned pointers); the same bits either way
    uint32_t project_grid_x, project_grid_y;  // workgroups of kAssignGemmWaves waves: 128-row tiles of the M + N rows, 128-column tiles of
                                              // the D + 1 outputs (0: no projection)
    uint32_t sim_grid_x, sim_grid_y;          // 128-row tiles of M, 128-column tiles of N
    uint32_t norm_row_blocks, norm_col_blocks;  // workgroups of one wave: one per row, then one per kAssignNormCols columns
    size_t norm_lds;
    uint32_t finish_grid_x, finish_grid_y;    // kAssignFinishThreads columns of N + 1, kAssignFinishRows rows of M + 1
    int32_t launches;                // projection (with weights), similarity, normalisers, finish: 4 or 3
    // the workspace (ftk_layout.h), in this order: projected descriptors [M + N][D] and z [M + N] (with weights, count 0 without), the row
    // and column normalisers [M], [N], and (with weights) ls(z), ls(-z) per row [2][M] and per column [2][N]
    ftk_slot16<float> md, z, lse_row, lse_col, ls0, ls1;
    size_t bytes;
};
const char *match_assignment_refusal_name(MatchAssignmentRefusal r);
MatchAssignmentPlan match_assignment_plan(const MatchAssignmentPlanInput &in);

struct MatchAssignmentParams {
    const float *desc0, *desc1;     // [M][D], [N][D]
    int32_t rows0, rows1, dim;
    const float *weights, *bias;    // [D + 1][D] (row D: matchability), [D + 1]; null: no projection
    float q;                        // (float)sqrt(sqrt((double)D))
    float scale;                    // per side, without weights
    const int32_t *count0, *count1;  // device words or null
    float *md, *z;                  // workspace (with weights)
    float *lse_row, *lse_col, *ls0, *ls1;
    float *scores;                  // [M + 1] rows of row_stride floats
    int64_t row_stride;
};
// One call: the launches of the plan, in stream order.
hipError_t match_assignment_launch(const MatchAssignmentPlan &plan, const MatchAssignmentParams &p, hipStream_t stream);

}  // namespace ftk
