// ftk_lightglue_adaptive.cpp — LightGlue's adaptive depth and width behind the C ABI (include/ftk.h): the confidence
// heads, the per-layer step (decide and gather) and the finish (head select, the assignment head, the matcher, the map back to
// original indices) over device arrays, in a workspace the caller owns; nothing is copied to the host and nothing synchronises.  The
// gated layer itself is ftk_transformer_layer_adaptive_device (ftk_transformer.cpp).
#include <cmath>

#include "ftk_internal.h"
#include "lightglue_adaptive_plan.h"

static_assert(FTK_LIGHTGLUE_MAX_LAYERS == ftk::kAdaptiveMaxLayers && FTK_LIGHTGLUE_STATE_WORDS == ftk::kAdaptiveStateWords,
              "include/ftk.h states the limits");

namespace {

int plan_call(ftk_context *ctx, const char *who, int32_t rows0, int32_t rows1, int32_t dim, int32_t heads, ftk::LightglueAdaptivePlan *plan) {
    *plan = ftk::lightglue_adaptive_plan(ftk::LightglueAdaptivePlanInput{rows0, rows1, dim, heads});
    if (plan->refused != ftk::LightglueAdaptiveRefusal::None) {
        return ftk_fail(ctx, FTK_E_INVALID_ARGUMENT,
                        "%s: %d x %d rows of dimension %d with %d heads are outside the limits of ftk_transformer_layer_device (rows 1 .. %d per side, "
                        "dimension 1 .. %d, heads dividing it, an even head dimension in 2 .. %d)",
                        who, rows0, rows1, dim, heads, FTK_TRANSFORMER_MAX_ROWS, FTK_TRANSFORMER_MAX_DIM, FTK_TRANSFORMER_MAX_HEAD_DIM);
    }
    return FTK_OK;
}

bool aligned4(const void *p) { return ftk_aligned(p, 4); }
bool unit_interval(float v) { return v >= 0.0f && v <= 1.0f; }

}  // namespace

extern "C" {

int ftk_lightglue_adaptive_workspace_bytes(int32_t rows0, int32_t rows1, int32_t dim, int32_t heads, int64_t *bytes) {
    const char *who = "lightglue_adaptive_workspace_bytes";
    return ftk_workspace_bytes<ftk::LightglueAdaptivePlan>(who, bytes, [&](ftk::LightglueAdaptivePlan *plan) { return plan_call(nullptr, who, rows0, rows1, dim, heads, plan); });
}

int ftk_lightglue_confidence_device(ftk_context *ctx, void *stream, const float *d_desc0, int32_t rows0, const float *d_desc1, int32_t rows1, int32_t dim,
                                    const float *d_token_w, const float *d_token_b, const float *d_match_w, const float *d_match_b,
                                    const int32_t *d_live0, const int32_t *d_live1, const int32_t *d_gate, float *d_conf, float *d_mt) {
    if (!ctx) {
        return ftk_fail(nullptr, FTK_E_INVALID_ARGUMENT, "lightglue_confidence_device: null context");
    }
    FTK_LOCK(ctx);
    if (rows0 < 1 || rows1 < 1 || rows0 > FTK_TRANSFORMER_MAX_ROWS || rows1 > FTK_TRANSFORMER_MAX_ROWS) {
        return ftk_fail(ctx, FTK_E_INVALID_ARGUMENT, "lightglue_confidence_device: %d x %d rows outside 1 .. %d per side", rows0, rows1,
                        FTK_TRANSFORMER_MAX_ROWS);
    }
    if (dim < 1 || dim > FTK_TRANSFORMER_MAX_DIM) {
        return ftk_fail(ctx, FTK_E_INVALID_ARGUMENT, "lightglue_confidence_device: dimension %d outside 1 .. %d", dim, FTK_TRANSFORMER_MAX_DIM);
    }
    if (!d_desc0 || !d_desc1 || !d_token_w || !d_token_b || !d_match_w || !d_match_b || !d_conf || !d_mt) {
        return ftk_fail(ctx, FTK_E_INVALID_ARGUMENT, "lightglue_confidence_device: null buffer");
    }
    if (!aligned4(d_desc0) || !aligned4(d_desc1) || !aligned4(d_token_w) || !aligned4(d_token_b) || !aligned4(d_match_w) || !aligned4(d_match_b) ||
        !aligned4(d_live0) || !aligned4(d_live1) || !aligned4(d_gate) || !aligned4(d_conf) || !aligned4(d_mt)) {
        return ftk_fail(ctx, FTK_E_INVALID_ARGUMENT, "lightglue_confidence_device: every buffer must be 4-byte aligned");
    }
    ftk::LightglueAdaptivePlan plan{};
    plan.conf_blocks = ftk::lightglue_confidence_blocks((int64_t)rows0 + rows1);  // the one field this entry's launch reads
    ftk::ConfidenceParams p{d_desc0, d_desc1, rows0, rows1, dim, d_token_w, d_token_b, d_match_w, d_match_b, d_live0, d_live1, d_gate, d_conf, d_mt};
    FTK_HIP(ctx, hipSetDevice(ctx->device));
    FTK_HIP(ctx, ftk::confidence_launch(plan, p, static_cast<hipStream_t>(stream)));
    return FTK_OK;
}

int ftk_lightglue_adapt_step_device(ftk_context *ctx, void *stream, int32_t rows0, int32_t rows1, int32_t dim, int32_t heads, int32_t layer,
                                    const float *d_conf, const float *d_mt, const int32_t *d_count0, const int32_t *d_count1, int32_t *d_state,
                                    float threshold, float depth_confidence, float width_confidence, int32_t min_keypoints, const float *d_desc_in0,
                                    const float *d_desc_in1, const float *d_enc_in0, const float *d_enc_in1, const int32_t *d_ind_in0,
                                    const int32_t *d_ind_in1, float *d_desc_out0, float *d_desc_out1, float *d_enc_out0, float *d_enc_out1,
                                    int32_t *d_ind_out0, int32_t *d_ind_out1, int32_t *d_layers0, int32_t *d_layers1, void *d_workspace) {
    if (!ctx) {
        return ftk_fail(nullptr, FTK_E_INVALID_ARGUMENT, "lightglue_adapt_step_device: null context");
    }
    FTK_LOCK(ctx);
    ftk::LightglueAdaptivePlan plan;
    const int rc = plan_call(ctx, "lightglue_adapt_step_device", rows0, rows1, dim, heads, &plan);
    if (rc != FTK_OK) {
        return rc;
    }
    if (layer < 0 || layer >= FTK_LIGHTGLUE_MAX_LAYERS) {
        return ftk_fail(ctx, FTK_E_INVALID_ARGUMENT, "lightglue_adapt_step_device: layer %d outside 0 .. %d", layer, FTK_LIGHTGLUE_MAX_LAYERS - 1);
    }
    if (!unit_interval(threshold) || !(depth_confidence <= 1.0f) || !(width_confidence <= 1.0f) || min_keypoints < 0) {
        return ftk_fail(ctx, FTK_E_INVALID_ARGUMENT,
                        "lightglue_adapt_step_device: threshold %g must be in 0 .. 1, the confidences %g and %g at most 1 (<= 0: off), min_keypoints %d >= 0",
                        (double)threshold, (double)depth_confidence, (double)width_confidence, min_keypoints);
    }
    const void *all[] = {d_conf, d_mt, d_state, d_desc_in0, d_desc_in1, d_enc_in0, d_enc_in1, d_ind_in0, d_ind_in1, d_desc_out0, d_desc_out1,
                         d_enc_out0, d_enc_out1, d_ind_out0, d_ind_out1, d_layers0, d_layers1, d_workspace};
    for (const void *q : all) {
        if (!q || !aligned4(q)) {
            return ftk_fail(ctx, FTK_E_INVALID_ARGUMENT, "lightglue_adapt_step_device: null or misaligned buffer (4 bytes; the workspace 16)");
        }
    }
    if (!ftk_aligned(d_workspace, 16) || !aligned4(d_count0) || !aligned4(d_count1)) {
        return ftk_fail(ctx, FTK_E_INVALID_ARGUMENT, "lightglue_adapt_step_device: null or misaligned buffer (4 bytes; the workspace 16)");
    }
    if (d_desc_in0 == d_desc_out0 || d_desc_in1 == d_desc_out1 || d_enc_in0 == d_enc_out0 || d_enc_in1 == d_enc_out1 || d_ind_in0 == d_ind_out0 ||
        d_ind_in1 == d_ind_out1) {
        return ftk_fail(ctx, FTK_E_INVALID_ARGUMENT, "lightglue_adapt_step_device: the gather is not in place: the outputs are the other half of a pair");
    }
    ftk::AdaptStepParams p{};
    p.conf = d_conf, p.mt = d_mt;
    p.rows0 = rows0, p.rows1 = rows1, p.dim = dim, p.head_dim = dim / heads;
    p.count0 = d_count0, p.count1 = d_count1;
    p.state = d_state;
    p.layer = layer;
    p.depth_on = depth_confidence > 0.0f ? 1 : 0, p.width_on = width_confidence > 0.0f ? 1 : 0;
    p.threshold = threshold, p.depth = depth_confidence;
    p.width = (float)(1.0 - (double)width_confidence);
    p.min_keypoints = min_keypoints;
    p.src0 = plan.src0.in(d_workspace), p.src1 = plan.src1.in(d_workspace);
    p.desc_in0 = d_desc_in0, p.desc_in1 = d_desc_in1, p.enc_in0 = d_enc_in0, p.enc_in1 = d_enc_in1, p.ind_in0 = d_ind_in0, p.ind_in1 = d_ind_in1;
    p.desc_out0 = d_desc_out0, p.desc_out1 = d_desc_out1, p.enc_out0 = d_enc_out0, p.enc_out1 = d_enc_out1;
    p.ind_out0 = d_ind_out0, p.ind_out1 = d_ind_out1;
    p.layers0 = d_layers0, p.layers1 = d_layers1;
    FTK_HIP(ctx, hipSetDevice(ctx->device));
    FTK_HIP(ctx, ftk::adapt_step_launch(plan, p, static_cast<hipStream_t>(stream)));
    return FTK_OK;
}

int ftk_lightglue_finish_device(ftk_context *ctx, void *stream, const float *d_desc0, int32_t rows0, const float *d_desc1, int32_t rows1, int32_t dim,
                                int32_t heads, int32_t n_layers, const float *d_head_w, const float *d_head_b, const int32_t *d_state,
                                const int32_t *d_ind0, const int32_t *d_ind1, float min_score, void *d_workspace, float *d_scores,
                                int32_t *d_match_index, uint8_t *d_status, int32_t *d_layers0, int32_t *d_layers1) {
    if (!ctx) {
        return ftk_fail(nullptr, FTK_E_INVALID_ARGUMENT, "lightglue_finish_device: null context");
    }
    FTK_LOCK(ctx);
    ftk::LightglueAdaptivePlan plan;
    const int rc = plan_call(ctx, "lightglue_finish_device", rows0, rows1, dim, heads, &plan);
    if (rc != FTK_OK) {
        return rc;
    }
    if (n_layers < 1 || n_layers > FTK_LIGHTGLUE_MAX_LAYERS) {
        return ftk_fail(ctx, FTK_E_INVALID_ARGUMENT, "lightglue_finish_device: %d layers outside 1 .. %d", n_layers, FTK_LIGHTGLUE_MAX_LAYERS);
    }
    if (min_score != min_score) {
        return ftk_fail(ctx, FTK_E_INVALID_ARGUMENT, "lightglue_finish_device: min_score is NaN");
    }
    const void *all[] = {d_desc0, d_desc1, d_head_w, d_head_b, d_state, d_ind0, d_ind1, d_workspace, d_scores, d_match_index, d_status, d_layers0, d_layers1};
    for (const void *q : all) {
        if (!q) {
            return ftk_fail(ctx, FTK_E_INVALID_ARGUMENT, "lightglue_finish_device: null buffer");
        }
    }
    if (!ftk_aligned(d_workspace, 16) || !aligned4(d_desc0) || !aligned4(d_desc1) || !aligned4(d_head_w) || !aligned4(d_head_b) || !aligned4(d_state) ||
        !aligned4(d_ind0) || !aligned4(d_ind1) || !aligned4(d_scores) || !aligned4(d_match_index) || !aligned4(d_layers0) || !aligned4(d_layers1)) {
        return ftk_fail(ctx, FTK_E_INVALID_ARGUMENT, "lightglue_finish_device: the workspace must be 16-byte aligned, the others 4-byte");
    }
    ftk::FinishParams p{};
    p.rows0 = rows0, p.rows1 = rows1, p.dim = dim, p.n_layers = n_layers;
    p.head_w = d_head_w, p.head_b = d_head_b;
    p.sel_w = plan.head_w.in(d_workspace), p.sel_b = plan.head_b.in(d_workspace);
    p.state = d_state;
    p.ind0 = d_ind0, p.ind1 = d_ind1;
    int32_t *match = plan.match.in(d_workspace);
    uint8_t *status_in = plan.status.in(d_workspace);
    p.match = match, p.status_in = status_in;
    p.match_index = d_match_index, p.status = d_status;
    p.layers0 = d_layers0, p.layers1 = d_layers1;
    hipStream_t s = static_cast<hipStream_t>(stream);
    FTK_HIP(ctx, hipSetDevice(ctx->device));
    FTK_HIP(ctx, ftk::head_select_launch(plan, p, s));
    // the head and the matcher as they are, on the compacted sets with the live counts: rows and columns behind them are -inf
    int rc2 = ftk_match_assignment_device(ctx, stream, d_desc0, rows0, d_desc1, rows1, dim, p.sel_w, p.sel_b, 1.0f, d_state + ftk::kStateLive0,
                                          d_state + ftk::kStateLive1, plan.assign.in(d_workspace), d_scores, 0);
    if (rc2 != FTK_OK) {
        return rc2;
    }
    rc2 = ftk_nn_match_scores_device(ctx, stream, d_scores, 1, rows0, rows1, (int64_t)rows1 + 1, 0, min_score, match, status_in);
    if (rc2 != FTK_OK) {
        return rc2;
    }
    FTK_HIP(ctx, ftk::remap_launch(plan, p, s));
    return FTK_OK;
}

}  // extern "C"
