// ftk_pnp.cpp — PnpRansac behind the C ABI (include/ftk.h): the camera pose from landmarks and their pixels over device
// arrays, in a workspace the caller owns; nothing is copied to the host, nothing synchronises and nothing is allocated.
#include "ftk_internal.h"
#include "pnp_plan.h"

static_assert(FTK_PNP_SAMPLE == ftk::kPnpSample && FTK_PNP_MODEL_FLOATS == ftk::kPnpModelFloats && FTK_PNP_MAX_REFINE_ITERATIONS == ftk::kPnpMaxRefine,
              "include/ftk.h states the constants");
static_assert(FTK_PNP_SAMPLE_DLT6 == (int)ftk::PnpSample::Dlt6 && FTK_PNP_SAMPLE_P3P == (int)ftk::PnpSample::P3p && FTK_PNP_P3P_SAMPLE == ftk::kP3pSample,
              "include/ftk.h states the samplers");

namespace {

// The plan of a call, or its refusal as the entry's return value.
int plan_call(ftk_context *ctx, const char *who, int32_t n, int32_t hypotheses, int32_t refine_iterations, int32_t sample, ftk::PnpPlan *plan) {
    ftk::PnpPlanInput in{};
    in.n = n;
    in.hypotheses = hypotheses;
    in.refine_iterations = refine_iterations;
    in.sampler = static_cast<ftk::PnpSample>(sample);
    *plan = ftk::pnp_plan(in);
    switch (plan->refused) {
        case ftk::PnpRefusal::None:
            return FTK_OK;
        case ftk::PnpRefusal::Points:
            return ftk_fail(ctx, FTK_E_UNSUPPORTED, "%s: %d points above FTK_TRACK_TABLE_MAX_SLOTS = %d", who, n, FTK_TRACK_TABLE_MAX_SLOTS);
        case ftk::PnpRefusal::Hypotheses:
            return ftk_fail(ctx, FTK_E_UNSUPPORTED, "%s: %d hypotheses above FTK_EPIPOLAR_MAX_HYPOTHESES = %d", who, hypotheses,
                            FTK_EPIPOLAR_MAX_HYPOTHESES);
        case ftk::PnpRefusal::Refine:
            return ftk_fail(ctx, FTK_E_UNSUPPORTED, "%s: %d refit steps above FTK_PNP_MAX_REFINE_ITERATIONS = %d", who, refine_iterations,
                            FTK_PNP_MAX_REFINE_ITERATIONS);
        case ftk::PnpRefusal::Sampler:
            return ftk_fail(ctx, FTK_E_INVALID_ARGUMENT, "%s: sample %d is neither FTK_PNP_SAMPLE_DLT6 nor FTK_PNP_SAMPLE_P3P", who, sample);
        default:
            return ftk_fail(ctx, FTK_E_INVALID_ARGUMENT, "%s: bad sizes (%d points, %d hypotheses, %d refit steps)", who, n, hypotheses, refine_iterations);
    }
}

}  // namespace

extern "C" {

int ftk_pnp_ransac_workspace_bytes(int32_t n, int32_t hypotheses, int32_t refine_iterations, int64_t *bytes) {
    const char *who = "pnp_ransac_workspace_bytes";
    return ftk_workspace_bytes<ftk::PnpPlan>(who, bytes, [&](ftk::PnpPlan *plan) { return plan_call(nullptr, who, n, hypotheses, refine_iterations, FTK_PNP_SAMPLE_DLT6, plan); });
}

int ftk_pnp_ransac_device(ftk_context *ctx, void *stream, const float *d_landmarks, const float *d_uv, uint8_t *d_status, int32_t n, float fx,
                          float fy, float cx, float cy, float threshold, int32_t hypotheses, int32_t refine_iterations, uint32_t seed,
                          void *d_workspace, float *d_pose, int32_t *d_n_inliers, int32_t *d_best, int32_t *d_valid, int32_t *d_counts,
                          float *d_models) {
    return ftk_pnp_ransac_sampled_device(ctx, stream, d_landmarks, d_uv, d_status, n, fx, fy, cx, cy, threshold, hypotheses, refine_iterations, seed,
                                         FTK_PNP_SAMPLE_DLT6, d_workspace, d_pose, d_n_inliers, d_best, d_valid, d_counts, d_models);
}

int ftk_pnp_ransac_sampled_device(ftk_context *ctx, void *stream, const float *d_landmarks, const float *d_uv, uint8_t *d_status, int32_t n,
                                  float fx, float fy, float cx, float cy, float threshold, int32_t hypotheses, int32_t refine_iterations,
                                  uint32_t seed, int32_t sample, void *d_workspace, float *d_pose, int32_t *d_n_inliers, int32_t *d_best,
                                  int32_t *d_valid, int32_t *d_counts, float *d_models) {
    const char *who = sample == FTK_PNP_SAMPLE_DLT6 ? "pnp_ransac_device" : "pnp_ransac_sampled_device";
    if (!ctx) {
        return ftk_fail(nullptr, FTK_E_INVALID_ARGUMENT, "%s: null context", who);
    }
    FTK_LOCK(ctx);
    ftk::PnpPlan plan;
    const int rc = plan_call(ctx, who, n, hypotheses, refine_iterations, sample, &plan);
    if (rc != FTK_OK) {
        return rc;
    }
    if (!d_landmarks || !d_uv || !d_status || !d_workspace || !d_pose || !d_n_inliers || !d_best || !d_valid) {
        return ftk_fail(ctx, FTK_E_INVALID_ARGUMENT, "%s: null buffer", who);
    }
    if (!ftk_positive(fx) || !ftk_positive(fy) || !ftk_finite(cx) || !ftk_finite(cy)) {
        return ftk_fail(ctx, FTK_E_INVALID_ARGUMENT, "%s: the camera needs finite fx, fy > 0 and finite cx, cy (got %g %g %g %g)", who, (double)fx,
                        (double)fy, (double)cx, (double)cy);
    }
    if (!(threshold >= 0.0f) || !ftk_finite(threshold * threshold)) {
        return ftk_fail(ctx, FTK_E_INVALID_ARGUMENT, "%s: the threshold %g must be >= 0 and its square finite in float32", who, (double)threshold);
    }
    if (!ftk_aligned(d_uv, 8)) {
        return ftk_fail(ctx, FTK_E_INVALID_ARGUMENT, "%s: the (u, v) array must be 8-byte aligned", who);
    }
    if (!ftk_aligned(d_workspace, 16) || !ftk_aligned(d_landmarks, 4) || !ftk_aligned(d_pose, 4) || !ftk_aligned(d_n_inliers, 4) || !ftk_aligned(d_best, 4) ||
        !ftk_aligned(d_valid, 4) || !ftk_aligned(d_counts, 4) || !ftk_aligned(d_models, 4)) {
        return ftk_fail(ctx, FTK_E_INVALID_ARGUMENT, "%s: the workspace must be 16-byte aligned, the landmarks and the outputs 4-byte aligned", who);
    }
    ftk::PnpParams p{};
    p.landmarks = d_landmarks;
    p.uv = d_uv;
    p.status = d_status;
    p.n = n;
    p.hypotheses = hypotheses;
    p.fx = fx, p.fy = fy, p.cx = cx, p.cy = cy;
    // the two scalars of the inlier rule: float32, in this order
    p.ry = fy / fx;
    const float tn = threshold / fx;
    p.tn2 = tn * tn;
    p.seed = seed;
    p.m = plan.m.in(d_workspace);
    p.points = plan.points.in(d_workspace);
    p.depth = plan.depth.in(d_workspace);
    p.list = plan.list.in(d_workspace);
    p.counts = d_counts ? d_counts : plan.counts.in(d_workspace);
    p.models = d_models ? d_models : plan.models.in(d_workspace);
    p.valid = plan.valid.in(d_workspace);
    p.totals = plan.totals.in(d_workspace);
    p.tile_counts = plan.tile_counts.in(d_workspace);
    p.state = plan.state.in(d_workspace);
    p.flags = plan.flags.in(d_workspace);
    p.pose = d_pose;
    p.n_inliers = d_n_inliers;
    p.best = d_best;
    p.out_valid = d_valid;
    FTK_HIP(ctx, hipSetDevice(ctx->device));
    FTK_HIP(ctx, ftk::pnp_launch(plan, p, static_cast<hipStream_t>(stream)));
    return FTK_OK;
}

}  // extern "C"
