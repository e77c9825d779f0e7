// ftk_two_view.cpp — two-view outlier rejection with a choice of model behind the C ABI (include/ftk.h): RANSAC on the
// fundamental matrix, on a homography, or on both with a rule that picks one, over device arrays, in a workspace the caller owns; nothing
// is copied to the host, nothing synchronises and nothing is allocated.
#include "ftk_internal.h"
#include "two_view_plan.h"

static_assert(FTK_TWO_VIEW_FUNDAMENTAL == ftk::kTwoViewFundamental && FTK_TWO_VIEW_HOMOGRAPHY == ftk::kTwoViewHomography &&
                  FTK_TWO_VIEW_AUTO == ftk::kTwoViewAuto && FTK_TWO_VIEW_HOMOGRAPHY_SAMPLE == ftk::kTwoViewHomSample,
              "include/ftk.h states the modes");

namespace {

// The plan of a call, or its refusal as the entry's return value.
int plan_call(ftk_context *ctx, const char *who, int32_t n, int32_t hypotheses, int32_t image_rows, int32_t image_cols, int32_t mode,
              int32_t permille, ftk::TwoViewPlan *plan) {
    ftk::TwoViewPlanInput in{};
    in.n = n;
    in.hypotheses = hypotheses;
    in.image_rows = image_rows;
    in.image_cols = image_cols;
    in.mode = mode;
    in.prefer_permille = permille;
    *plan = ftk::two_view_plan(in);
    switch (plan->refused) {
        case ftk::TwoViewRefusal::None:
            return FTK_OK;
        case ftk::TwoViewRefusal::Mode:
            return ftk_fail(ctx, FTK_E_INVALID_ARGUMENT, "%s: mode %d is none of FTK_TWO_VIEW_FUNDAMENTAL, _HOMOGRAPHY, _AUTO", who, mode);
        case ftk::TwoViewRefusal::Prefer:
            return ftk_fail(ctx, FTK_E_INVALID_ARGUMENT, "%s: prefer_homography_permille %d outside 0 .. 1000", who, permille);
        case ftk::TwoViewRefusal::Points:
            return ftk_fail(ctx, FTK_E_UNSUPPORTED, "%s: %d points above FTK_TRACK_TABLE_MAX_SLOTS = %d", who, n, FTK_TRACK_TABLE_MAX_SLOTS);
        case ftk::TwoViewRefusal::Hypotheses:
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

int ftk_two_view_workspace_bytes(int32_t n, int32_t hypotheses, int32_t mode, int64_t *bytes) {
    if (!bytes) {
        return ftk_fail(nullptr, FTK_E_INVALID_ARGUMENT, "two_view_workspace_bytes: null argument");
    }
    ftk::TwoViewPlan plan;
    const int rc = plan_call(nullptr, "two_view_workspace_bytes", n, hypotheses, 1, 1, mode, 0, &plan);
    if (rc != FTK_OK) {
        return rc;
    }
    *bytes = (int64_t)plan.bytes;
    return FTK_OK;
}

int ftk_two_view_ransac_device(ftk_context *ctx, void *stream, const float *d_ref_uv, const float *d_cur_uv, uint8_t *d_status, int32_t n,
                               int32_t image_rows, int32_t image_cols, float threshold, int32_t hypotheses, uint32_t seed, int32_t mode,
                               int32_t prefer_homography_permille, void *d_workspace, int32_t *d_model, int32_t *d_best, int32_t *d_n_inliers,
                               float *d_F, float *d_H, int32_t *d_counts, float *d_models) {
    if (!ctx) {
        return ftk_fail(nullptr, FTK_E_INVALID_ARGUMENT, "two_view_ransac_device: null context");
    }
    FTK_LOCK(ctx);
    ftk::TwoViewPlan plan;
    const int rc = plan_call(ctx, "two_view_ransac_device", n, hypotheses, image_rows, image_cols, mode, prefer_homography_permille, &plan);
    if (rc != FTK_OK) {
        return rc;
    }
    if (!d_ref_uv || !d_cur_uv || !d_status || !d_workspace || !d_model || !d_best || !d_n_inliers || !d_F || !d_H) {
        return ftk_fail(ctx, FTK_E_INVALID_ARGUMENT, "two_view_ransac_device: null buffer");
    }
    if (!(threshold >= 0.0f) || !(threshold <= 3.0e38f)) {
        return ftk_fail(ctx, FTK_E_INVALID_ARGUMENT, "two_view_ransac_device: the threshold %g must be finite and >= 0", (double)threshold);
    }
    if (!aligned(d_ref_uv, 8) || !aligned(d_cur_uv, 8)) {
        return ftk_fail(ctx, FTK_E_INVALID_ARGUMENT, "two_view_ransac_device: the (u, v) arrays must be 8-byte aligned");
    }
    if (!aligned(d_workspace, 16) || !aligned(d_model, 4) || !aligned(d_best, 4) || !aligned(d_n_inliers, 4) || !aligned(d_F, 4) || !aligned(d_H, 4) ||
        !aligned(d_counts, 4) || !aligned(d_models, 4)) {
        return ftk_fail(ctx, FTK_E_INVALID_ARGUMENT, "two_view_ransac_device: the workspace must be 16-byte aligned, the outputs 4-byte aligned");
    }
    uint8_t *ws = static_cast<uint8_t *>(d_workspace);
    const size_t K = (size_t)hypotheses;
    ftk::TwoViewParams p{};
    p.e.ref_uv = d_ref_uv;
    p.e.cur_uv = d_cur_uv;
    p.e.status = d_status;
    p.e.n = n;
    p.e.hypotheses = hypotheses;
    // the normalisation is fixed by the image: float32, in this order
    p.e.cx = 0.5f * (float)(image_cols - 1);
    p.e.cy = 0.5f * (float)(image_rows - 1);
    p.e.s = 2.0f / (float)(image_cols + image_rows);
    const float tn = threshold * p.e.s;
    p.e.tn2 = tn * tn;
    p.e.seed = seed;
    p.e.m = reinterpret_cast<int32_t *>(ws);
    p.e.points = reinterpret_cast<float4 *>(ws + plan.off_points);
    p.e.list = reinterpret_cast<int32_t *>(ws + plan.off_list);
    p.e.counts = d_counts ? d_counts : reinterpret_cast<int32_t *>(ws + plan.off_counts);
    p.e.models = d_models ? d_models : reinterpret_cast<float *>(ws + plan.off_models);
    p.e.valid = ws + plan.off_valid;
    p.counts_h = p.e.counts + K;
    p.models_h = p.e.models + 9 * K;
    p.valid_h = p.e.valid + K;
    p.mode = mode;
    p.prefer_permille = prefer_homography_permille;
    p.model = d_model;
    p.best = d_best;
    p.n_inliers = d_n_inliers;
    p.F = d_F;
    p.H = d_H;
    FTK_HIP(ctx, hipSetDevice(ctx->device));
    FTK_HIP(ctx, ftk::two_view_launch(plan, p, static_cast<hipStream_t>(stream)));
    return FTK_OK;
}

}  // extern "C"
