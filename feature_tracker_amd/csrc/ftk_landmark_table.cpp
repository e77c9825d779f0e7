// ftk_landmark_table.cpp — the landmark table behind the C ABI (include/ftk.h): the two entries of a frame over device
// arrays the caller owns; nothing is copied to the host, nothing synchronises and nothing is allocated.
#include "ftk_internal.h"
#include "landmark_table_plan.h"

static_assert(FTK_LANDMARK_TABLE_BLOCK == ftk::kLandmarkBlock && FTK_LANDMARK_TABLE_COUNTERS == ftk::kLandmarkCounters &&
                  FTK_LANDMARK_TABLE_VALID == ftk::kLandmarkValid && FTK_LANDMARK_TABLE_N_NEW == ftk::kLandmarkNew &&
                  FTK_LANDMARK_TABLE_N_ANCHORED == ftk::kLandmarkAnchored && FTK_LANDMARK_TABLE_N_LANDMARKS == ftk::kLandmarkCount &&
                  FTK_LANDMARK_TABLE_N_DROPPED == ftk::kLandmarkDropped && FTK_LANDMARK_TABLE_LOST == ftk::kLandmarkLost &&
                  FTK_LANDMARK_TABLE_STEADY == ftk::kLandmarkSteady && FTK_LANDMARK_TABLE_BOOTSTRAP == ftk::kLandmarkBootstrap,
              "include/ftk.h states the constants");

namespace {

// The plan of a call, or its refusal as the entry's return value.
int plan_call(ftk_context *ctx, const char *who, int32_t n, ftk::LandmarkPlan *plan) {
    *plan = ftk::landmark_table_plan(n);
    switch (plan->refused) {
        case ftk::LandmarkRefusal::None:
            return FTK_OK;
        case ftk::LandmarkRefusal::Slots:
            return ftk_fail(ctx, FTK_E_UNSUPPORTED, "%s: %d slots above FTK_TRACK_TABLE_MAX_SLOTS = %d", who, n, FTK_TRACK_TABLE_MAX_SLOTS);
        default:
            return ftk_fail(ctx, FTK_E_INVALID_ARGUMENT, "%s: bad size (%d slots)", who, n);
    }
}

}  // namespace

extern "C" {

int ftk_landmark_table_begin_device(ftk_context *ctx, void *stream, const int64_t *d_ids, int32_t n, int64_t *d_owner, float *d_landmarks,
                                    int32_t *d_anchor_frame, uint8_t *d_pnp_status, uint8_t *d_anchor_status, int32_t *d_counters) {
    const char *who = "landmark_table_begin_device";
    if (!ctx) {
        return ftk_fail(nullptr, FTK_E_INVALID_ARGUMENT, "%s: null context", who);
    }
    FTK_LOCK(ctx);
    ftk::LandmarkPlan plan;
    const int rc = plan_call(ctx, who, n, &plan);
    if (rc != FTK_OK) {
        return rc;
    }
    if (!d_ids || !d_owner || !d_landmarks || !d_anchor_frame || !d_pnp_status || !d_anchor_status || !d_counters) {
        return ftk_fail(ctx, FTK_E_INVALID_ARGUMENT, "%s: null buffer", who);
    }
    if (!ftk_aligned(d_ids, 8) || !ftk_aligned(d_owner, 8) || !ftk_aligned(d_landmarks, 4) || !ftk_aligned(d_anchor_frame, 4) || !ftk_aligned(d_counters, 4)) {
        return ftk_fail(ctx, FTK_E_INVALID_ARGUMENT, "%s: ids and owner must be 8-byte aligned, the other arrays 4-byte aligned", who);
    }
    ftk::LandmarkParams p{};
    p.ids = d_ids;
    p.n = n;
    p.owner = d_owner;
    p.landmarks = d_landmarks;
    p.anchor_frame = d_anchor_frame;
    p.pnp_status = d_pnp_status;
    p.anchor_status = d_anchor_status;
    p.counters = d_counters;
    FTK_HIP(ctx, hipSetDevice(ctx->device));
    FTK_HIP(ctx, ftk::landmark_begin_launch(plan, p, static_cast<hipStream_t>(stream)));
    return FTK_OK;
}

int ftk_landmark_table_end_device(ftk_context *ctx, void *stream, const int64_t *d_ids, const float *d_points, int32_t n, const uint8_t *d_status_in,
                                  const float *d_pose_in, const int32_t *d_valid_in, const int32_t *d_model_in, int32_t frame, int32_t mode, float fx,
                                  float fy, float cx, float cy, float threshold, float min_parallax_cos2, float *d_landmarks, float *d_anchor_uv,
                                  float *d_anchor_pose, int32_t *d_anchor_frame, int32_t *d_counters, float *d_pose) {
    const char *who = "landmark_table_end_device";
    if (!ctx) {
        return ftk_fail(nullptr, FTK_E_INVALID_ARGUMENT, "%s: null context", who);
    }
    FTK_LOCK(ctx);
    ftk::LandmarkPlan plan;
    const int rc = plan_call(ctx, who, n, &plan);
    if (rc != FTK_OK) {
        return rc;
    }
    if (mode != FTK_LANDMARK_TABLE_STEADY && mode != FTK_LANDMARK_TABLE_BOOTSTRAP) {
        return ftk_fail(ctx, FTK_E_INVALID_ARGUMENT, "%s: mode %d is neither FTK_LANDMARK_TABLE_STEADY nor FTK_LANDMARK_TABLE_BOOTSTRAP", who, mode);
    }
    if (frame < 0) {
        return ftk_fail(ctx, FTK_E_INVALID_ARGUMENT, "%s: frame %d is negative: a negative anchor_frame means no anchor", who, frame);
    }
    if (!d_ids || !d_points || !d_pose_in || !d_valid_in || !d_landmarks || !d_anchor_uv || !d_anchor_pose || !d_anchor_frame || !d_counters || !d_pose ||
        (mode == FTK_LANDMARK_TABLE_STEADY && !d_status_in)) {
        return ftk_fail(ctx, FTK_E_INVALID_ARGUMENT, "%s: null buffer", who);
    }
    if (!ftk_positive(fx) || !ftk_positive(fy) || !ftk_finite(cx) || !ftk_finite(cy)) {
        return ftk_fail(ctx, FTK_E_INVALID_ARGUMENT, "%s: the camera needs finite fx, fy > 0 and finite cx, cy (got %g %g %g %g)", who, (double)fx,
                        (double)fy, (double)cx, (double)cy);
    }
    if (!(threshold >= 0.0f) || !ftk_finite(threshold * threshold)) {
        return ftk_fail(ctx, FTK_E_INVALID_ARGUMENT, "%s: the threshold %g must be >= 0 and its square finite in float32", who, (double)threshold);
    }
    if (!(min_parallax_cos2 >= 0.0f && min_parallax_cos2 <= 1.0f)) {
        return ftk_fail(ctx, FTK_E_INVALID_ARGUMENT, "%s: min_parallax_cos2 %g is no squared cosine (0 .. 1)", who, (double)min_parallax_cos2);
    }
    if (!ftk_aligned(d_ids, 8) || !ftk_aligned(d_points, 8) || !ftk_aligned(d_anchor_uv, 8)) {
        return ftk_fail(ctx, FTK_E_INVALID_ARGUMENT, "%s: ids, points and anchor_uv must be 8-byte aligned", who);
    }
    if (!ftk_aligned(d_pose_in, 4) || !ftk_aligned(d_valid_in, 4) || !ftk_aligned(d_model_in, 4) || !ftk_aligned(d_landmarks, 4) || !ftk_aligned(d_anchor_pose, 4) ||
        !ftk_aligned(d_anchor_frame, 4) || !ftk_aligned(d_counters, 4) || !ftk_aligned(d_pose, 4)) {
        return ftk_fail(ctx, FTK_E_INVALID_ARGUMENT, "%s: the float and int32 arrays must be 4-byte aligned", who);
    }
    ftk::LandmarkParams p{};
    p.ids = d_ids;
    p.points = d_points;
    p.n = n;
    p.landmarks = d_landmarks;
    p.anchor_uv = d_anchor_uv;
    p.anchor_pose = d_anchor_pose;
    p.anchor_frame = d_anchor_frame;
    p.counters = d_counters;
    p.pose = d_pose;
    p.status_in = d_status_in;
    p.pose_in = d_pose_in;
    p.valid_in = d_valid_in;
    p.model_in = d_model_in;
    p.frame = frame;
    p.mode = mode;
    p.fx = fx, p.fy = fy, p.cx = cx, p.cy = cy;
    // the two scalars of PnpRansac's inlier rule: float32, in this order
    p.ry = fy / fx;
    const float tn = threshold / fx;
    p.tn2 = tn * tn;
    p.c2 = min_parallax_cos2;
    FTK_HIP(ctx, hipSetDevice(ctx->device));
    FTK_HIP(ctx, ftk::landmark_end_launch(plan, p, static_cast<hipStream_t>(stream)));
    return FTK_OK;
}

}  // extern "C"
