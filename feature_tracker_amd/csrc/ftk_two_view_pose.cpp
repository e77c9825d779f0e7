// ftk_two_view_pose.cpp — TwoViewPose behind the C ABI (include/ftk.h): the relative pose of two views and the landmarks of
// their inliers over device arrays, in a workspace the caller owns; nothing is copied to the host, nothing synchronises and nothing is
// allocated.
#include "ftk_internal.h"
#include "two_view_pose_plan.h"

static_assert(FTK_POSE_JACOBI_SWEEPS == ftk::kPoseJacobiSweeps && FTK_POSE_TILE == ftk::kPoseTile, "include/ftk.h states the constants");

namespace {

// The plan of a call, or its refusal as the entry's return value.
int plan_call(ftk_context *ctx, const char *who, int32_t n, ftk::TwoViewPosePlan *plan) {
    ftk::TwoViewPosePlanInput in{};
    in.n = n;
    *plan = ftk::two_view_pose_plan(in);
    switch (plan->refused) {
        case ftk::TwoViewPoseRefusal::None:
            return FTK_OK;
        case ftk::TwoViewPoseRefusal::Points:
            return ftk_fail(ctx, FTK_E_UNSUPPORTED, "%s: %d points above FTK_TRACK_TABLE_MAX_SLOTS = %d", who, n, FTK_TRACK_TABLE_MAX_SLOTS);
        default:
            return ftk_fail(ctx, FTK_E_INVALID_ARGUMENT, "%s: bad size (%d points)", who, n);
    }
}

}  // namespace

extern "C" {

int ftk_two_view_pose_workspace_bytes(int32_t n, int64_t *bytes) {
    const char *who = "two_view_pose_workspace_bytes";
    return ftk_workspace_bytes<ftk::TwoViewPosePlan>(who, bytes, [&](ftk::TwoViewPosePlan *plan) { return plan_call(nullptr, who, n, plan); });
}

int ftk_two_view_pose_device(ftk_context *ctx, void *stream, const float *d_ref_uv, const float *d_cur_uv, uint8_t *d_status, int32_t n, float fx,
                             float fy, float cx, float cy, float fx_cur, float fy_cur, float cx_cur, float cy_cur, float threshold, float baseline,
                             void *d_workspace, float *d_pose, float *d_points, float *d_E, int32_t *d_n_front, int32_t *d_valid, int32_t *d_n_points) {
    const char *who = "two_view_pose_device";
    if (!ctx) {
        return ftk_fail(nullptr, FTK_E_INVALID_ARGUMENT, "%s: null context", who);
    }
    FTK_LOCK(ctx);
    ftk::TwoViewPosePlan plan;
    const int rc = plan_call(ctx, who, n, &plan);
    if (rc != FTK_OK) {
        return rc;
    }
    if (!d_ref_uv || !d_cur_uv || !d_status || !d_workspace || !d_pose || !d_points || !d_E || !d_n_front || !d_valid || !d_n_points) {
        return ftk_fail(ctx, FTK_E_INVALID_ARGUMENT, "%s: null buffer", who);
    }
    if (!ftk_positive(fx) || !ftk_positive(fy) || !ftk_positive(fx_cur) || !ftk_positive(fy_cur) || !ftk_finite(cx) || !ftk_finite(cy) || !ftk_finite(cx_cur) || !ftk_finite(cy_cur)) {
        return ftk_fail(ctx, FTK_E_INVALID_ARGUMENT, "%s: a camera needs finite fx, fy > 0 and finite cx, cy (got %g %g %g %g and %g %g %g %g)", who,
                        (double)fx, (double)fy, (double)cx, (double)cy, (double)fx_cur, (double)fy_cur, (double)cx_cur, (double)cy_cur);
    }
    if (!(threshold >= 0.0f) || !ftk_finite(threshold * threshold)) {  // the kernels compare against threshold^2
        return ftk_fail(ctx, FTK_E_INVALID_ARGUMENT, "%s: the threshold %g must be >= 0 and its square finite in float32", who, (double)threshold);
    }
    if (!ftk_positive(baseline)) {
        return ftk_fail(ctx, FTK_E_INVALID_ARGUMENT, "%s: the baseline %g must be finite and > 0", who, (double)baseline);
    }
    if (!ftk_aligned(d_ref_uv, 8) || !ftk_aligned(d_cur_uv, 8)) {
        return ftk_fail(ctx, FTK_E_INVALID_ARGUMENT, "%s: the (u, v) arrays must be 8-byte aligned", who);
    }
    if (!ftk_aligned(d_workspace, 16) || !ftk_aligned(d_pose, 4) || !ftk_aligned(d_points, 4) || !ftk_aligned(d_E, 4) || !ftk_aligned(d_n_front, 4) || !ftk_aligned(d_valid, 4) ||
        !ftk_aligned(d_n_points, 4)) {
        return ftk_fail(ctx, FTK_E_INVALID_ARGUMENT, "%s: the workspace must be 16-byte aligned, the outputs 4-byte aligned", who);
    }
    ftk::TwoViewPoseParams p{};
    p.ref_uv = d_ref_uv;
    p.cur_uv = d_cur_uv;
    p.status = d_status;
    p.n = n;
    p.fx1 = fx, p.fy1 = fy, p.cx1 = cx, p.cy1 = cy;
    p.fx2 = fx_cur, p.fy2 = fy_cur, p.cx2 = cx_cur, p.cy2 = cy_cur;
    p.t2 = threshold * threshold;
    p.baseline = baseline;
    p.m = plan.m.in(d_workspace);
    p.points = plan.points.in(d_workspace);
    p.totals = plan.totals.in(d_workspace);
    p.model = plan.model.in(d_workspace);
    p.pose = d_pose;
    p.landmarks = d_points;
    p.E = d_E;
    p.n_front = d_n_front;
    p.valid = d_valid;
    p.n_points = d_n_points;
    FTK_HIP(ctx, hipSetDevice(ctx->device));
    FTK_HIP(ctx, ftk::two_view_pose_launch(plan, p, static_cast<hipStream_t>(stream)));
    return FTK_OK;
}

}  // extern "C"
