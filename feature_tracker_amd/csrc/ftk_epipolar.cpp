// ftk_epipolar.cpp — two-view outlier rejection behind the C ABI (include/ftk.h): RANSAC on the fundamental matrix over
// device arrays, in a workspace the caller owns; nothing is copied to the host, nothing synchronises and nothing is allocated.
#include "ftk_internal.h"
#include "epipolar_plan.h"

static_assert(FTK_EPIPOLAR_MAX_HYPOTHESES == ftk::kEpipolarMaxHypotheses && FTK_TRACK_TABLE_MAX_SLOTS == ftk::kEpipolarMaxPoints &&
                  FTK_EPIPOLAR_SAMPLE == ftk::kEpipolarSample && FTK_EPIPOLAR_MAX_ATTEMPTS == ftk::kEpipolarMaxAttempts &&
                  FTK_EPIPOLAR_SCORE_TILE == ftk::kEpipolarScoreTile,
              "include/ftk.h states the limits");

namespace {

// The plan of a call, or its refusal as the entry's return value.
int plan_call(ftk_context *ctx, const char *who, int32_t n, int32_t hypotheses, int32_t image_rows, int32_t image_cols, ftk::EpipolarPlan *plan) {
    ftk::EpipolarPlanInput in{};
    in.n = n;
    in.hypotheses = hypotheses;
    in.image_rows = image_rows;
    in.image_cols = image_cols;
    *plan = ftk::epipolar_plan(in);
    switch (plan->refused) {
        case ftk::EpipolarRefusal::None:
            return FTK_OK;
        case ftk::EpipolarRefusal::Points:
            return ftk_fail(ctx, FTK_E_UNSUPPORTED, "%s: %d points above FTK_TRACK_TABLE_MAX_SLOTS = %d", who, n, FTK_TRACK_TABLE_MAX_SLOTS);
        case ftk::EpipolarRefusal::Hypotheses:
            return ftk_fail(ctx, FTK_E_UNSUPPORTED, "%s: %d hypotheses above FTK_EPIPOLAR_MAX_HYPOTHESES = %d", who, hypotheses,
                            FTK_EPIPOLAR_MAX_HYPOTHESES);
        default:
            return ftk_fail(ctx, FTK_E_INVALID_ARGUMENT, "%s: bad sizes (%d points, %d hypotheses, a %d x %d image)", who, n, hypotheses, image_rows,
                            image_cols);
    }
}

bool aligned(const void *p, uintptr_t to) { return (reinterpret_cast<uintptr_t>(p) & (to - 1)) == 0; }

}  // namespace

extern "C" {

int ftk_epipolar_workspace_bytes(int32_t n, int32_t hypotheses, int64_t *bytes) {
    if (!bytes) {
        return ftk_fail(nullptr, FTK_E_INVALID_ARGUMENT, "epipolar_workspace_bytes: null argument");
    }
    ftk::EpipolarPlan plan;
    const int rc = plan_call(nullptr, "epipolar_workspace_bytes", n, hypotheses, 1, 1, &plan);
    if (rc != FTK_OK) {
        return rc;
    }
    *bytes = (int64_t)plan.bytes;
    return FTK_OK;
}

int ftk_epipolar_ransac_device(ftk_context *ctx, void *stream, const float *d_ref_uv, const float *d_cur_uv, uint8_t *d_status, int32_t n,
                               int32_t image_rows, int32_t image_cols, float threshold, int32_t hypotheses, uint32_t seed, void *d_workspace,
                               int32_t *d_best, int32_t *d_n_inliers, float *d_F, int32_t *d_counts, float *d_models) {
    if (!ctx) {
        return ftk_fail(nullptr, FTK_E_INVALID_ARGUMENT, "epipolar_ransac_device: null context");
    }
    FTK_LOCK(ctx);
    ftk::EpipolarPlan plan;
    const int rc = plan_call(ctx, "epipolar_ransac_device", n, hypotheses, image_rows, image_cols, &plan);
    if (rc != FTK_OK) {
        return rc;
    }
    if (!d_ref_uv || !d_cur_uv || !d_status || !d_workspace || !d_best || !d_n_inliers || !d_F) {
        return ftk_fail(ctx, FTK_E_INVALID_ARGUMENT, "epipolar_ransac_device: null buffer");
    }
    if (!(threshold >= 0.0f) || !(threshold <= 3.0e38f)) {
        return ftk_fail(ctx, FTK_E_INVALID_ARGUMENT, "epipolar_ransac_device: the threshold %g must be finite and >= 0", (double)threshold);
    }
    if (!aligned(d_ref_uv, 8) || !aligned(d_cur_uv, 8)) {
        return ftk_fail(ctx, FTK_E_INVALID_ARGUMENT, "epipolar_ransac_device: the (u, v) arrays must be 8-byte aligned");
    }
    if (!aligned(d_workspace, 16) || !aligned(d_best, 4) || !aligned(d_n_inliers, 4) || !aligned(d_F, 4) || !aligned(d_counts, 4) || !aligned(d_models, 4)) {
        return ftk_fail(ctx, FTK_E_INVALID_ARGUMENT, "epipolar_ransac_device: the workspace must be 16-byte aligned, the outputs 4-byte aligned");
    }
    uint8_t *ws = static_cast<uint8_t *>(d_workspace);
    ftk::EpipolarParams p{};
    p.ref_uv = d_ref_uv;
    p.cur_uv = d_cur_uv;
    p.status = d_status;
    p.n = n;
    p.hypotheses = hypotheses;
    // the normalisation is fixed by the image: float32, in this order
    p.cx = 0.5f * (float)(image_cols - 1);
    p.cy = 0.5f * (float)(image_rows - 1);
    p.s = 2.0f / (float)(image_cols + image_rows);
    const float tn = threshold * p.s;
    p.tn2 = tn * tn;
    p.seed = seed;
    p.m = reinterpret_cast<int32_t *>(ws);
    p.points = reinterpret_cast<float4 *>(ws + plan.off_points);
    p.list = reinterpret_cast<int32_t *>(ws + plan.off_list);
    p.counts = d_counts ? d_counts : reinterpret_cast<int32_t *>(ws + plan.off_counts);
    p.models = d_models ? d_models : reinterpret_cast<float *>(ws + plan.off_models);
    p.valid = ws + plan.off_valid;
    p.best = d_best;
    p.n_inliers = d_n_inliers;
    p.F = d_F;
    FTK_HIP(ctx, hipSetDevice(ctx->device));
    FTK_HIP(ctx, ftk::epipolar_launch(plan, p, static_cast<hipStream_t>(stream)));
    return FTK_OK;
}

}  // extern "C"
