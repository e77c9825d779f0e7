// ftk_match_assignment.cpp — LightGlue's assignment head behind the C ABI (include/ftk.h): two descriptor sets to the
// [M + 1][N + 1] log-assignment tensor over device arrays, in a workspace the caller owns; nothing is copied to the host, nothing
// synchronises and nothing is allocated.
#include <cmath>

#include "ftk_internal.h"
#include "match_assignment_plan.h"

static_assert(FTK_MATCH_ASSIGNMENT_MAX_ROWS == ftk::kAssignMaxRows && FTK_MATCH_ASSIGNMENT_MAX_DIM == ftk::kAssignMaxDim,
              "include/ftk.h states the limits");

namespace {

// The plan of a call, or its refusal as the entry's return value.
int plan_call(ftk_context *ctx, const char *who, int32_t rows0, int32_t rows1, int32_t dim, int32_t with_weights, int64_t row_stride, bool aligned16,
              ftk::MatchAssignmentPlan *plan) {
    ftk::MatchAssignmentPlanInput in{};
    in.rows0 = rows0;
    in.rows1 = rows1;
    in.dim = dim;
    in.with_weights = with_weights;
    in.row_stride = row_stride;
    in.aligned16 = aligned16 ? 1 : 0;
    *plan = ftk::match_assignment_plan(in);
    switch (plan->refused) {
        case ftk::MatchAssignmentRefusal::None:
            return FTK_OK;
        case ftk::MatchAssignmentRefusal::Rows:
            return ftk_fail(ctx, FTK_E_INVALID_ARGUMENT, "%s: %d x %d descriptors outside 1 .. %d per side", who, rows0, rows1, FTK_MATCH_ASSIGNMENT_MAX_ROWS);
        case ftk::MatchAssignmentRefusal::Dim:
            return ftk_fail(ctx, FTK_E_INVALID_ARGUMENT, "%s: descriptor dimension %d outside 1 .. %d", who, dim, FTK_MATCH_ASSIGNMENT_MAX_DIM);
        default:
            return ftk_fail(ctx, FTK_E_INVALID_ARGUMENT, "%s: row_stride %lld must be 0 or at least %d (and at most 2^24)", who, (long long)row_stride,
                            rows1 + 1);
    }
}

}  // namespace

extern "C" {

int ftk_match_assignment_workspace_bytes(int32_t rows0, int32_t rows1, int32_t dim, int32_t with_weights, int64_t *bytes) {
    const char *who = "match_assignment_workspace_bytes";
    return ftk_workspace_bytes<ftk::MatchAssignmentPlan>(
        who, bytes, [&](ftk::MatchAssignmentPlan *plan) { return plan_call(nullptr, who, rows0, rows1, dim, with_weights, 0, false, plan); });
}

int ftk_match_assignment_device(ftk_context *ctx, void *stream, const float *d_desc0, int32_t rows0, const float *d_desc1, int32_t rows1, int32_t dim,
                                const float *d_weights, const float *d_bias, float scale, const int32_t *d_count0, const int32_t *d_count1,
                                void *d_workspace, float *d_scores, int64_t row_stride) {
    if (!ctx) {
        return ftk_fail(nullptr, FTK_E_INVALID_ARGUMENT, "match_assignment_device: null context");
    }
    FTK_LOCK(ctx);
    const bool with_weights = d_weights != nullptr;
    const bool aligned16 = ftk_aligned(d_desc0, 16) && ftk_aligned(d_desc1, 16) && ftk_aligned(d_weights, 16);
    ftk::MatchAssignmentPlan plan;
    const int rc = plan_call(ctx, "match_assignment_device", rows0, rows1, dim, with_weights ? 1 : 0, row_stride, aligned16, &plan);
    if (rc != FTK_OK) {
        return rc;
    }
    if (!d_desc0 || !d_desc1 || !d_workspace || !d_scores || (with_weights && !d_bias)) {
        return ftk_fail(ctx, FTK_E_INVALID_ARGUMENT, "match_assignment_device: null buffer");
    }
    if (!with_weights && (!(scale > 0.0f) || !(scale <= 3.0e38f))) {
        return ftk_fail(ctx, FTK_E_INVALID_ARGUMENT, "match_assignment_device: scale %g must be finite and positive", (double)scale);
    }
    if (!ftk_aligned(d_workspace, 16) || !ftk_aligned(d_desc0, 4) || !ftk_aligned(d_desc1, 4) || !ftk_aligned(d_weights, 4) || !ftk_aligned(d_bias, 4) ||
        !ftk_aligned(d_count0, 4) || !ftk_aligned(d_count1, 4) || !ftk_aligned(d_scores, 4)) {
        return ftk_fail(ctx, FTK_E_INVALID_ARGUMENT, "match_assignment_device: the workspace must be 16-byte aligned, the others 4-byte");
    }
    ftk::MatchAssignmentParams p{};
    p.desc0 = d_desc0;
    p.desc1 = d_desc1;
    p.rows0 = rows0;
    p.rows1 = rows1;
    p.dim = dim;
    p.weights = d_weights;
    p.bias = d_bias;
    p.q = (float)std::sqrt(std::sqrt((double)dim));
    p.scale = with_weights ? 1.0f : scale;
    p.count0 = d_count0;
    p.count1 = d_count1;
    p.md = with_weights ? plan.md.in(d_workspace) : nullptr;
    p.z = with_weights ? plan.z.in(d_workspace) : nullptr;
    p.lse_row = plan.lse_row.in(d_workspace);
    p.lse_col = plan.lse_col.in(d_workspace);
    p.ls0 = with_weights ? plan.ls0.in(d_workspace) : nullptr;
    p.ls1 = with_weights ? plan.ls1.in(d_workspace) : nullptr;
    p.scores = d_scores;
    p.row_stride = plan.row_stride;
    FTK_HIP(ctx, hipSetDevice(ctx->device));
    FTK_HIP(ctx, ftk::match_assignment_launch(plan, p, static_cast<hipStream_t>(stream)));
    return FTK_OK;
}

}  // extern "C"
