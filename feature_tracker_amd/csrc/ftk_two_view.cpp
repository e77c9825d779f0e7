// ftk_two_view.cpp — two-view outlier rejection behind the C ABI (include/ftk.h): RANSAC on the fundamental
// matrix (ftk_epipolar_*), or on the fundamental matrix, on a homography, or on both with a rule that picks one (ftk_two_view_*), over
// device arrays, in a workspace the caller owns; nothing is copied to the host, nothing synchronises and nothing is allocated.  The two
// pairs of entries are ONE implementation: the first is the second with one slot and the fundamental mode.
#include "ftk_internal.h"
#include "two_view_plan.h"

static_assert(FTK_EPIPOLAR_MAX_HYPOTHESES == ftk::kEpipolarMaxHypotheses && FTK_TRACK_TABLE_MAX_SLOTS == ftk::kEpipolarMaxPoints &&
                  FTK_EPIPOLAR_SAMPLE == ftk::kEpipolarSample && FTK_EPIPOLAR_MAX_ATTEMPTS == ftk::kEpipolarMaxAttempts &&
                  FTK_EPIPOLAR_SCORE_TILE == ftk::kEpipolarScoreTile,
              "include/ftk.h states the limits");
static_assert(FTK_TWO_VIEW_FUNDAMENTAL == ftk::kTwoViewFundamental && FTK_TWO_VIEW_HOMOGRAPHY == ftk::kTwoViewHomography &&
                  FTK_TWO_VIEW_AUTO == ftk::kTwoViewAuto && FTK_TWO_VIEW_HOMOGRAPHY_SAMPLE == ftk::kTwoViewHomSample,
              "include/ftk.h states the modes");

namespace {

// The plan of a call, or its refusal as the entry's return value.
int plan_call(ftk_context *ctx, const char *who, int32_t slots, int32_t n, int32_t hypotheses, int32_t image_rows, int32_t image_cols, int32_t mode,
              int32_t permille, ftk::TwoViewPlan *plan) {
    ftk::TwoViewPlanInput in{};
    in.n = n;
    in.hypotheses = hypotheses;
    in.image_rows = image_rows;
    in.image_cols = image_cols;
    in.slots = slots;
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

int workspace_bytes(const char *who, int32_t slots, int32_t n, int32_t hypotheses, int32_t mode, int64_t *bytes) {
    return ftk_workspace_bytes<ftk::TwoViewPlan>(
        who, bytes, [&](ftk::TwoViewPlan *plan) { return plan_call(nullptr, who, slots, n, hypotheses, 1, 1, mode, 0, plan); });
}

// Both device entries.  One slot: d_model and d_H are not part of the entry (null), d_best / d_n_inliers hold one element.
int ransac_device(const char *who, int32_t slots, ftk_context *ctx, void *stream, const float *d_ref_uv, const float *d_cur_uv, uint8_t *d_status,
                  int32_t n, int32_t image_rows, int32_t image_cols, float threshold, int32_t hypotheses, uint32_t seed, int32_t mode, int32_t permille,
                  void *d_workspace, int32_t *d_model, int32_t *d_best, int32_t *d_n_inliers, float *d_F, float *d_H, int32_t *d_counts,
                  float *d_models) {
    if (!ctx) {
        return ftk_fail(nullptr, FTK_E_INVALID_ARGUMENT, "%s: null context", who);
    }
    FTK_LOCK(ctx);
    ftk::TwoViewPlan plan;
    const int rc = plan_call(ctx, who, slots, n, hypotheses, image_rows, image_cols, mode, permille, &plan);
    if (rc != FTK_OK) {
        return rc;
    }
    if (!d_ref_uv || !d_cur_uv || !d_status || !d_workspace || !d_best || !d_n_inliers || !d_F || (slots > 1 && (!d_model || !d_H))) {
        return ftk_fail(ctx, FTK_E_INVALID_ARGUMENT, "%s: null buffer", who);
    }
    if (!(threshold >= 0.0f) || !(threshold <= 3.0e38f)) {
        return ftk_fail(ctx, FTK_E_INVALID_ARGUMENT, "%s: the threshold %g must be finite and >= 0", who, (double)threshold);
    }
    if (!ftk_aligned(d_ref_uv, 8) || !ftk_aligned(d_cur_uv, 8)) {
        return ftk_fail(ctx, FTK_E_INVALID_ARGUMENT, "%s: the (u, v) arrays must be 8-byte aligned", who);
    }
    if (!ftk_aligned(d_workspace, 16) || !ftk_aligned(d_model, 4) || !ftk_aligned(d_best, 4) || !ftk_aligned(d_n_inliers, 4) || !ftk_aligned(d_F, 4) ||
        !ftk_aligned(d_H, 4) || !ftk_aligned(d_counts, 4) || !ftk_aligned(d_models, 4)) {
        return ftk_fail(ctx, FTK_E_INVALID_ARGUMENT, "%s: the workspace must be 16-byte aligned, the outputs 4-byte aligned", who);
    }
    const size_t K = (size_t)hypotheses;
    ftk::TwoViewParams p{};
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
    p.m = plan.m.in(d_workspace);
    p.points = plan.points.in(d_workspace);
    p.list = plan.list.in(d_workspace);
    int32_t *const counts = d_counts ? d_counts : plan.counts.in(d_workspace);
    float *const models = d_models ? d_models : plan.models.in(d_workspace);
    for (int32_t s = 0; s < slots; ++s) {
        p.slot[s].counts = counts + (size_t)s * K;
        p.slot[s].models = models + (size_t)s * 9 * K;
        p.slot[s].valid = plan.valid.in(d_workspace) + (size_t)s * K;
    }
    p.prefer_permille = permille;
    p.model = d_model;
    p.best = d_best;
    p.n_inliers = d_n_inliers;
    p.F = d_F;
    p.H = d_H;
    FTK_HIP(ctx, hipSetDevice(ctx->device));
    FTK_HIP(ctx, ftk::two_view_launch(plan, p, static_cast<hipStream_t>(stream)));
    return FTK_OK;
}

}  // namespace

extern "C" {

int ftk_epipolar_workspace_bytes(int32_t n, int32_t hypotheses, int64_t *bytes) {
    return workspace_bytes("epipolar_workspace_bytes", 1, n, hypotheses, FTK_TWO_VIEW_FUNDAMENTAL, bytes);
}

int ftk_epipolar_ransac_device(ftk_context *ctx, void *stream, const float *d_ref_uv, const float *d_cur_uv, uint8_t *d_status, int32_t n,
                               int32_t image_rows, int32_t image_cols, float threshold, int32_t hypotheses, uint32_t seed, void *d_workspace,
                               int32_t *d_best, int32_t *d_n_inliers, float *d_F, int32_t *d_counts, float *d_models) {
    return ransac_device("epipolar_ransac_device", 1, ctx, stream, d_ref_uv, d_cur_uv, d_status, n, image_rows, image_cols, threshold, hypotheses, seed,
                         FTK_TWO_VIEW_FUNDAMENTAL, 0, d_workspace, nullptr, d_best, d_n_inliers, d_F, nullptr, d_counts, d_models);
}

int ftk_two_view_workspace_bytes(int32_t n, int32_t hypotheses, int32_t mode, int64_t *bytes) {
    return workspace_bytes("two_view_workspace_bytes", 2, n, hypotheses, mode, bytes);
}

int ftk_two_view_ransac_device(ftk_context *ctx, void *stream, const float *d_ref_uv, const float *d_cur_uv, uint8_t *d_status, int32_t n,
                               int32_t image_rows, int32_t image_cols, float threshold, int32_t hypotheses, uint32_t seed, int32_t mode,
                               int32_t prefer_homography_permille, void *d_workspace, int32_t *d_model, int32_t *d_best, int32_t *d_n_inliers,
                               float *d_F, float *d_H, int32_t *d_counts, float *d_models) {
    return ransac_device("two_view_ransac_device", 2, ctx, stream, d_ref_uv, d_cur_uv, d_status, n, image_rows, image_cols, threshold, hypotheses, seed,
                         mode, prefer_homography_permille, d_workspace, d_model, d_best, d_n_inliers, d_F, d_H, d_counts, d_models);
}

}  // extern "C"
