// ftk_transformer.cpp — LightGlue's transformer layer behind the C ABI (include/ftk.h): attention alone, a Linear alone,
// and the whole layer (self block on both sets, cross block in both directions) over device arrays, in a workspace the caller owns;
// nothing is copied to the host, nothing synchronises and nothing is allocated.
#include <cmath>

#include "ftk_internal.h"
#include "transformer_plan.h"

static_assert(FTK_TRANSFORMER_MAX_ROWS == ftk::kTransformerMaxRows && FTK_TRANSFORMER_MAX_DIM == ftk::kTransformerMaxDim &&
                  FTK_TRANSFORMER_MAX_HEAD_DIM == ftk::kTransformerMaxHeadDim,
              "include/ftk.h states the limits");

namespace {

// A plan's refusal as the entry's return value.
int refusal(ftk_context *ctx, const char *who, const ftk::TransformerPlan &plan, int32_t rows0, int32_t rows1, int32_t dim, int32_t heads) {
    switch (plan.refused) {
        case ftk::TransformerRefusal::None:
            return FTK_OK;
        case ftk::TransformerRefusal::Rows:
            return ftk_fail(ctx, FTK_E_INVALID_ARGUMENT, "%s: %d x %d rows outside 1 .. %d per side", who, rows0, rows1, FTK_TRANSFORMER_MAX_ROWS);
        case ftk::TransformerRefusal::Dim:
            return ftk_fail(ctx, FTK_E_INVALID_ARGUMENT, "%s: dimension %d outside 1 .. %d", who, dim, FTK_TRANSFORMER_MAX_DIM);
        case ftk::TransformerRefusal::Heads:
            return ftk_fail(ctx, FTK_E_INVALID_ARGUMENT, "%s: %d heads do not divide dimension %d", who, heads, dim);
        default:
            return ftk_fail(ctx, FTK_E_INVALID_ARGUMENT, "%s: head dimension %d must be even and in 2 .. %d", who, heads > 0 ? dim / heads : 0,
                            FTK_TRANSFORMER_MAX_HEAD_DIM);
    }
}

bool usable_scale(float s) { return s > 0.0f && s <= 3.0e38f; }

// The layer's 12 launches.  `gate` null: ftk_transformer_layer_device.  Otherwise the adaptive pass: the counts are the
// live counts, every kernel returns at once when *gate != 0 or where all of its rows are pruned, and the layer may run in place
// (d_out == d_desc): the last launch is the only writer of the outputs and every read of the inputs lies in the self block.
int run_layer(ftk_context *ctx, const ftk::TransformerPlan &plan, const float *d_desc0, int32_t rows0, const float *d_desc1, int32_t rows1, int32_t dim,
              const float *d_enc0, const float *d_enc1, const float *d_weights, const int32_t *d_count0, const int32_t *d_count1, const int32_t *gate,
              void *d_workspace, float *d_out0, float *d_out1, hipStream_t s) {
    float *qkv = plan.qkv.in(d_workspace), *att = plan.ctx.in(d_workspace), *msg = plan.msg.in(d_workspace), *hidden = plan.hidden.in(d_workspace);
    float *x1 = plan.x1.in(d_workspace);
    const int32_t rows = rows0 + rows1, dh = plan.head_dim;
    const size_t d = (size_t)dim, plane = (size_t)rows * d, second = (size_t)rows0 * d;
    const bool vec = plan.vec_linear != 0;
    const int32_t *live0 = gate ? d_count0 : nullptr, *live1 = gate ? d_count1 : nullptr;
    const auto gated = [&](ftk::LinearParams &lin) { lin.gate = gate, lin.live0 = live0, lin.live1 = live1; };
    for (int block = 0; block < 2; ++block) {
        const bool self = block == 0;
        const size_t *w = self ? plan.w_self : plan.w_cross;
        const float *in0 = self ? d_desc0 : x1, *in1 = self ? d_desc1 : x1 + second;
        ftk::LinearParams lin{};
        gated(lin);
        lin.rows0 = rows0;
        lin.rows = rows;
        // q | k | v (self, rotary on q and k), or qk | v (cross), as planes
        lin.a0 = in0, lin.a1 = in1, lin.ka = dim;
        lin.w = d_weights + w[0], lin.bias = d_weights + w[1];
        lin.outs = (self ? 3 : 2) * dim;
        lin.epilogue = self ? ftk::kLinearRotary : ftk::kLinearPlain;
        lin.enc0 = d_enc0, lin.enc1 = d_enc1, lin.head_dim = dh, lin.rotary_outs = 2 * dim;
        lin.out0 = qkv, lin.out1 = qkv + second, lin.plane_cols = dim, lin.plane_stride = (int64_t)plane;
        FTK_HIP(ctx, ftk::linear_launch(lin, vec, plan.linear_grid_x, self ? plan.grid_y_3d : plan.grid_y_2d, s));
        ftk::AttentionParams at{};
        at.dim = dim;
        at.head_dim = dh;
        at.gate = gate;
        if (self) {
            at.prob[0] = ftk::AttentionProblem{qkv, qkv + plane, qkv + 2 * plane, att, rows0, rows0, d_count0, live0};
            at.prob[1] = ftk::AttentionProblem{qkv + second, qkv + plane + second, qkv + 2 * plane + second, att + second, rows1, rows1, d_count1, live1};
            at.pre = 1.0f;
            at.post = (float)(1.0 / std::sqrt((double)dh));
        } else {
            at.prob[0] = ftk::AttentionProblem{qkv, qkv + second, qkv + plane + second, att, rows0, rows1, d_count1, live0};
            at.prob[1] = ftk::AttentionProblem{qkv + second, qkv, qkv + plane, att + second, rows1, rows0, d_count0, live1};
            at.pre = (float)std::pow((double)dh, -0.25);
            at.post = 1.0f;
        }
        FTK_HIP(ctx, ftk::attention_launch(plan, at, s));
        // out_proj / to_out
        lin = ftk::LinearParams{};
        gated(lin);
        lin.rows0 = rows0, lin.rows = rows;
        lin.a0 = att, lin.a1 = att + second, lin.ka = dim;
        lin.w = d_weights + w[2], lin.bias = d_weights + w[3];
        lin.outs = dim;
        lin.out0 = msg, lin.out1 = msg + second, lin.plane_cols = dim;
        FTK_HIP(ctx, ftk::linear_launch(lin, vec, plan.linear_grid_x, plan.grid_y_d, s));
        // ffn.0 on [x | message]
        lin.a0 = in0, lin.a1 = in1;
        lin.b = msg, lin.kb = dim;
        lin.w = d_weights + w[4], lin.bias = d_weights + w[5];
        lin.outs = 2 * dim;
        lin.out0 = hidden, lin.out1 = hidden + 2 * second, lin.plane_cols = 2 * dim;
        FTK_HIP(ctx, ftk::linear_launch(lin, vec, plan.linear_grid_x, plan.grid_y_2d, s));
        FTK_HIP(ctx, ftk::layernorm_gelu_launch(ftk::NormParams{hidden, rows, 2 * dim, d_weights + w[6], d_weights + w[7], gate, live0, live1, rows0},
                                                plan.norm_blocks, s));
        // x + ffn.3
        lin = ftk::LinearParams{};
        gated(lin);
        lin.rows0 = rows0, lin.rows = rows;
        lin.a0 = hidden, lin.a1 = hidden + 2 * second, lin.ka = 2 * dim;
        lin.w = d_weights + w[8], lin.bias = d_weights + w[9];
        lin.outs = dim;
        lin.epilogue = ftk::kLinearResidual;
        lin.x0 = in0, lin.x1 = in1;
        lin.out0 = self ? x1 : d_out0, lin.out1 = self ? x1 + second : d_out1, lin.plane_cols = dim;
        FTK_HIP(ctx, ftk::linear_launch(lin, vec, plan.linear_grid_x, plan.grid_y_d, s));
    }
    return FTK_OK;
}

}  // namespace

extern "C" {

int ftk_transformer_layer_workspace_bytes(int32_t rows0, int32_t rows1, int32_t dim, int32_t heads, int64_t *bytes) {
    const char *who = "transformer_layer_workspace_bytes";
    return ftk_workspace_bytes<ftk::TransformerPlan>(who, bytes, [&](ftk::TransformerPlan *plan) {
        *plan = ftk::transformer_plan(ftk::TransformerPlanInput{rows0, rows1, dim, heads, 0});
        return refusal(nullptr, who, *plan, rows0, rows1, dim, heads);
    });
}

int ftk_attention_device(ftk_context *ctx, void *stream, const float *d_q, int32_t rows_q, const float *d_k, const float *d_v, int32_t rows_k,
                         int32_t heads, int32_t head_dim, const int32_t *d_count, float pre_scale, float post_scale, float *d_out) {
    if (!ctx) {
        return ftk_fail(nullptr, FTK_E_INVALID_ARGUMENT, "attention_device: null context");
    }
    FTK_LOCK(ctx);
    const bool aligned16 = ftk_aligned(d_q, 16) && ftk_aligned(d_k, 16) && ftk_aligned(d_v, 16);
    const ftk::TransformerPlan plan = ftk::attention_plan(rows_q, rows_k, heads, head_dim, aligned16 ? 1 : 0);
    const bool sized = heads >= 1 && heads <= FTK_TRANSFORMER_MAX_DIM && head_dim >= 1 && head_dim <= FTK_TRANSFORMER_MAX_DIM;
    const int rc = refusal(ctx, "attention_device", plan, rows_q, rows_k, sized ? heads * head_dim : head_dim, sized ? heads : 1);
    if (rc != FTK_OK) {
        return rc;
    }
    if (!d_q || !d_k || !d_v || !d_out) {
        return ftk_fail(ctx, FTK_E_INVALID_ARGUMENT, "attention_device: null buffer");
    }
    if (!usable_scale(pre_scale) || !usable_scale(post_scale)) {
        return ftk_fail(ctx, FTK_E_INVALID_ARGUMENT, "attention_device: scales %g, %g must be finite and positive", (double)pre_scale, (double)post_scale);
    }
    if (!ftk_aligned(d_q, 4) || !ftk_aligned(d_k, 4) || !ftk_aligned(d_v, 4) || !ftk_aligned(d_out, 4) || !ftk_aligned(d_count, 4)) {
        return ftk_fail(ctx, FTK_E_INVALID_ARGUMENT, "attention_device: every buffer must be 4-byte aligned");
    }
    ftk::AttentionParams p{};
    p.prob[0] = ftk::AttentionProblem{d_q, d_k, d_v, d_out, rows_q, rows_k, d_count, nullptr};
    p.prob[1] = p.prob[0];
    p.dim = heads * head_dim;
    p.head_dim = head_dim;
    p.pre = pre_scale;
    p.post = post_scale;
    FTK_HIP(ctx, hipSetDevice(ctx->device));
    FTK_HIP(ctx, ftk::attention_launch(plan, p, static_cast<hipStream_t>(stream)));
    return FTK_OK;
}

int ftk_linear_device(ftk_context *ctx, void *stream, const float *d_x, int32_t rows, int32_t in_dim, const float *d_weight, const float *d_bias,
                      int32_t out_dim, float *d_out) {
    if (!ctx) {
        return ftk_fail(nullptr, FTK_E_INVALID_ARGUMENT, "linear_device: null context");
    }
    FTK_LOCK(ctx);
    const ftk::LinearPlan plan = ftk::linear_plan(rows, in_dim, out_dim, ftk_aligned(d_x, 16) && ftk_aligned(d_weight, 16) ? 1 : 0);
    if (plan.refused == ftk::TransformerRefusal::Rows) {
        return ftk_fail(ctx, FTK_E_INVALID_ARGUMENT, "linear_device: %d rows outside 1 .. %d", rows, FTK_TRANSFORMER_MAX_ROWS);
    }
    if (plan.refused != ftk::TransformerRefusal::None) {
        return ftk_fail(ctx, FTK_E_INVALID_ARGUMENT, "linear_device: dimensions %d -> %d outside 1 .. %d", in_dim, out_dim, FTK_TRANSFORMER_MAX_DIM);
    }
    if (!d_x || !d_weight || !d_bias || !d_out) {
        return ftk_fail(ctx, FTK_E_INVALID_ARGUMENT, "linear_device: null buffer");
    }
    if (!ftk_aligned(d_x, 4) || !ftk_aligned(d_weight, 4) || !ftk_aligned(d_bias, 4) || !ftk_aligned(d_out, 4)) {
        return ftk_fail(ctx, FTK_E_INVALID_ARGUMENT, "linear_device: every buffer must be 4-byte aligned");
    }
    ftk::LinearParams p{};
    p.a0 = p.a1 = d_x;
    p.rows0 = p.rows = rows;
    p.ka = in_dim;
    p.w = d_weight;
    p.bias = d_bias;
    p.outs = out_dim;
    p.epilogue = ftk::kLinearPlain;
    p.out0 = p.out1 = d_out;
    p.plane_cols = out_dim;
    FTK_HIP(ctx, hipSetDevice(ctx->device));
    FTK_HIP(ctx, ftk::linear_launch(p, plan.vec != 0, plan.grid_x, plan.grid_y, static_cast<hipStream_t>(stream)));
    return FTK_OK;
}

int ftk_transformer_layer_device(ftk_context *ctx, void *stream, const float *d_desc0, int32_t rows0, const float *d_desc1, int32_t rows1, int32_t dim,
                                 int32_t heads, const float *d_enc0, const float *d_enc1, const float *d_weights, const int32_t *d_count0,
                                 const int32_t *d_count1, void *d_workspace, float *d_out0, float *d_out1) {
    if (!ctx) {
        return ftk_fail(nullptr, FTK_E_INVALID_ARGUMENT, "transformer_layer_device: null context");
    }
    FTK_LOCK(ctx);
    const bool aligned16 = ftk_aligned(d_desc0, 16) && ftk_aligned(d_desc1, 16) && ftk_aligned(d_weights, 16) && ftk_aligned(d_out0, 16) && ftk_aligned(d_out1, 16);
    const ftk::TransformerPlan plan = ftk::transformer_plan(ftk::TransformerPlanInput{rows0, rows1, dim, heads, aligned16 ? 1 : 0});
    const int rc = refusal(ctx, "transformer_layer_device", plan, rows0, rows1, dim, heads);
    if (rc != FTK_OK) {
        return rc;
    }
    if (!d_desc0 || !d_desc1 || !d_enc0 || !d_enc1 || !d_weights || !d_workspace || !d_out0 || !d_out1) {
        return ftk_fail(ctx, FTK_E_INVALID_ARGUMENT, "transformer_layer_device: null buffer");
    }
    if (!ftk_aligned(d_workspace, 16) || !ftk_aligned(d_desc0, 4) || !ftk_aligned(d_desc1, 4) || !ftk_aligned(d_enc0, 4) || !ftk_aligned(d_enc1, 4) || !ftk_aligned(d_weights, 4) ||
        !ftk_aligned(d_count0, 4) || !ftk_aligned(d_count1, 4) || !ftk_aligned(d_out0, 4) || !ftk_aligned(d_out1, 4)) {
        return ftk_fail(ctx, FTK_E_INVALID_ARGUMENT, "transformer_layer_device: the workspace must be 16-byte aligned, the others 4-byte");
    }
    FTK_HIP(ctx, hipSetDevice(ctx->device));
    return run_layer(ctx, plan, d_desc0, rows0, d_desc1, rows1, dim, d_enc0, d_enc1, d_weights, d_count0, d_count1, nullptr, d_workspace, d_out0, d_out1,
                     static_cast<hipStream_t>(stream));
}

int ftk_transformer_layer_adaptive_device(ftk_context *ctx, void *stream, float *d_desc0, int32_t rows0, float *d_desc1, int32_t rows1, int32_t dim,
                                          int32_t heads, const float *d_enc0, const float *d_enc1, const float *d_weights, const int32_t *d_live0,
                                          const int32_t *d_live1, const int32_t *d_gate, void *d_workspace) {
    if (!ctx) {
        return ftk_fail(nullptr, FTK_E_INVALID_ARGUMENT, "transformer_layer_adaptive_device: null context");
    }
    FTK_LOCK(ctx);
    const bool aligned16 = ftk_aligned(d_desc0, 16) && ftk_aligned(d_desc1, 16) && ftk_aligned(d_weights, 16);
    const ftk::TransformerPlan plan = ftk::transformer_plan(ftk::TransformerPlanInput{rows0, rows1, dim, heads, aligned16 ? 1 : 0});
    const int rc = refusal(ctx, "transformer_layer_adaptive_device", plan, rows0, rows1, dim, heads);
    if (rc != FTK_OK) {
        return rc;
    }
    if (!d_desc0 || !d_desc1 || !d_enc0 || !d_enc1 || !d_weights || !d_workspace || !d_live0 || !d_live1 || !d_gate) {
        return ftk_fail(ctx, FTK_E_INVALID_ARGUMENT, "transformer_layer_adaptive_device: null buffer (the live counts and the gate are required)");
    }
    if (!ftk_aligned(d_workspace, 16) || !ftk_aligned(d_desc0, 4) || !ftk_aligned(d_desc1, 4) || !ftk_aligned(d_enc0, 4) || !ftk_aligned(d_enc1, 4) || !ftk_aligned(d_weights, 4) ||
        !ftk_aligned(d_live0, 4) || !ftk_aligned(d_live1, 4) || !ftk_aligned(d_gate, 4)) {
        return ftk_fail(ctx, FTK_E_INVALID_ARGUMENT, "transformer_layer_adaptive_device: the workspace must be 16-byte aligned, the others 4-byte");
    }
    FTK_HIP(ctx, hipSetDevice(ctx->device));
    return run_layer(ctx, plan, d_desc0, rows0, d_desc1, rows1, dim, d_enc0, d_enc1, d_weights, d_live0, d_live1, d_gate, d_workspace, d_desc0, d_desc1,
                     static_cast<hipStream_t>(stream));
}

}  // extern "C"
