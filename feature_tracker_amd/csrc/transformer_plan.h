// transformer_plan.h — the launch plan and workspace layout of LightGlue's transformer layer (transformer_kernels.hip),
// as match_assignment_plan.h is the assignment head's: a pure function of values (no context, no environment, no HIP call;
// tests/test_transformer_args_cpu.py walks it without a device through host/build/transformer_plan_cli).  ftk_transformer.cpp plans,
// the launchers carry the plan out: every grid they launch is a field of the plan.
#pragma once

#include "ftk_device.h"
#include "ftk_layout.h"

namespace ftk {

constexpr int kTransformerMaxRows = 4096;   // FTK_TRANSFORMER_MAX_ROWS: M, N
constexpr int kTransformerMaxDim = 1024;    // FTK_TRANSFORMER_MAX_DIM: D
constexpr int kTransformerMaxHeadDim = 128;  // FTK_TRANSFORMER_MAX_HEAD_DIM: dh
constexpr int kLinearWaves = 4;             // waves of a linear workgroup, each with its own 32 rows
constexpr int kLinearTileRows = 32 * kLinearWaves;
constexpr int kLinearTileCols = 128;        // 4 MFMA column tiles per wave (mfma_tile_gemm.h)
constexpr int kAttnThreads = 64;            // one wave per attention workgroup: 32 query rows of one head
constexpr int kAttnKeyTile = 128;           // keys per step of a sweep
constexpr int kAttnLdsStride = 33;          // floats between the LDS rows of a 32 x 32 tile of p: the A-operand read is conflict-free
constexpr int kAttnFillWaves = 256;         // below this many waves a head's output columns are split 32 per wave
constexpr int kNormThreads = 64;            // layernorm_gelu_kernel: one wave per row

struct TransformerPlanInput {
    int32_t rows0, rows1;  // M, N
    int32_t dim;           // D
    int32_t heads;         // h
    int32_t aligned16;     // every tensor pointer is 16-byte aligned
};
enum class TransformerRefusal { None, Rows, Dim, Heads, HeadDim };
struct TransformerPlan {
    TransformerRefusal refused;  // not None: nothing else is set
    int32_t head_dim;            // dh = D / h
    int32_t vec_linear;          // Linear rows are read four channels at a time (D % 4 == 0 and aligned pointers); the same bits either way
    int32_t vec_attn;            // the same for a head's dh channels (dh % 4 == 0 too)
    uint32_t linear_grid_x;      // 128-row tiles of the M + N rows
    uint32_t grid_y_d, grid_y_2d, grid_y_3d;  // 128-column tiles of D, 2 D and 3 D outputs
    int32_t attn_out_tiles;      // 32-column tiles of a head's output one wave accumulates: 1, 2 or 4
    uint32_t attn_grid_x, attn_grid_y, attn_grid_z;  // 32-row tiles of max(M, N); heads x column splits; the two sets or directions
    uint32_t norm_blocks;        // M + N
    int32_t launches;            // 12: per block qkv, attention, out, ffn.0, LayerNorm + GELU, ffn.3
    // the workspace (ftk_layout.h), in this order, R = M + N: the q | k | v planes [3][R][D], the attention output [R][D], the message
    // [R][D], the hidden rows [R][2 D], the self block's result [R][D]
    ftk_slot16<float> qkv, ctx, msg, hidden, x1;
    size_t bytes;
    // the packed weights, float offsets: per block w_in, b_in, w_out, b_out, w_ffn0, b_ffn0, gamma, beta, w_ffn3, b_ffn3
    size_t w_self[10], w_cross[10], weight_floats;
};
// The Linear entry alone (LightGlue's input_proj): limits, then one launch of linear_kernel.
struct LinearPlan {
    TransformerRefusal refused;  // None, Rows or Dim
    int32_t vec;
    uint32_t grid_x, grid_y;     // 128-row tiles, 128-column tiles of the outputs
};
LinearPlan linear_plan(int32_t rows, int32_t in_dim, int32_t out_dim, int32_t aligned16);
const char *transformer_refusal_name(TransformerRefusal r);
TransformerPlan transformer_plan(const TransformerPlanInput &in);
// The attention entry alone: the same limits on (rows_q, rows_k, h * dh, h) and the attention part of the plan.
TransformerPlan attention_plan(int32_t rows_q, int32_t rows_k, int32_t heads, int32_t head_dim, int32_t aligned16);

enum LinearEpilogue { kLinearPlain = 0, kLinearResidual = 1, kLinearRotary = 2 };

// y[i][o] = epilogue(bias[o] + sum_c [a | b][i][c] w[o][c]) for the rows of both sets
struct LinearParams {
    const float *a0, *a1;      // segment A: rows below rows0 from a0, the others from a1 (row - rows0); ka floats a row
    const float *b;            // segment B [rows][kb] or null
    int32_t rows0, rows, ka, kb;
    const float *w, *bias;     // [outs][ka + kb], [outs]
    int32_t outs;
    int32_t epilogue;
    const float *x0, *x1;      // residual: [rows0][outs], [rows - rows0][outs]
    const float *enc0, *enc1;  // rotary: [2][rows0][dh], [2][rows - rows0][dh]
    int32_t head_dim;
    int32_t rotary_outs;       // outputs below this are rotated
    float *out0, *out1;        // rows below rows0, the others; plane o / plane_cols at plane_stride floats, plane_cols floats a row
    int32_t plane_cols;
    int64_t plane_stride;
    // the adaptive pass, all null otherwise: a wave returns before its first load when *gate != 0 or when all of its
    // rows lie at or behind their set's live count
    const int32_t *gate, *live0, *live1;
};
// One launch on the plan's grid (grid_y: the 128-column tiles of p.outs).
hipError_t linear_launch(const LinearParams &p, bool vec, uint32_t grid_x, uint32_t grid_y, hipStream_t stream);

// One problem of an attention launch (blockIdx.z)
struct AttentionProblem {
    const float *q, *k, *v;    // [rows_q][dim], [rows_k][dim], [rows_k][dim]
    float *out;                // [rows_q][dim]
    int32_t rows_q, rows_k;
    const int32_t *count;      // of the keys; device word or null
    const int32_t *live_q;     // of the queries, read only with a gate; device word or null
};
struct AttentionParams {
    AttentionProblem prob[2];
    int32_t dim, head_dim;
    float pre, post;
    const int32_t *gate;       // the adaptive pass or null: a workgroup returns when *gate != 0 or its queries lie at or behind live_q
};
hipError_t attention_launch(const TransformerPlan &plan, const AttentionParams &p, hipStream_t stream);

struct NormParams {
    float *rows;               // [n_rows][cols], in place
    int32_t n_rows, cols;
    const float *gamma, *beta;
    const int32_t *gate, *live0, *live1;  // the adaptive pass or null, as LinearParams'; rows below rows0 belong to the first set
    int32_t rows0;
};
hipError_t layernorm_gelu_launch(const NormParams &p, uint32_t blocks, hipStream_t stream);

}  // namespace ftk
