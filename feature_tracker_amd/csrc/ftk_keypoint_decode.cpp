// ftk_keypoint_decode.cpp — the keypoint decoder behind the C ABI (include/ftk.h): a SuperPoint-style network's head
// tensors to keypoints, scores and descriptors over device arrays, in a workspace the caller owns; nothing is copied to the host, nothing
// synchronises and nothing is allocated.
#include "ftk_internal.h"
#include "keypoint_decode_plan.h"

static_assert(FTK_KEYPOINT_DECODE_CELL == ftk::kKeypointCell && FTK_KEYPOINT_DECODE_MAX_KEYPOINTS == ftk::kKeypointMaxKeypoints &&
                  FTK_KEYPOINT_DECODE_MAX_CHANNELS == ftk::kKeypointMaxChannels && FTK_HARRIS_DEVICE_MAX_SURVIVORS == ftk::kKeypointMaxSurvivors &&
                  FTK_HARRIS_RANK_TILE == ftk::kKeypointRankTile,
              "include/ftk.h states the limits");

namespace {

// The plan of a call, or its refusal as the entry's return value.
int plan_call(ftk_context *ctx, const char *who, int32_t cell_rows, int32_t cell_cols, int32_t channels, int32_t max_keypoints, int32_t min_distance,
              int32_t border, int32_t n_occupied, ftk::KeypointDecodePlan *plan) {
    ftk::KeypointDecodePlanInput in{};
    in.cell_rows = cell_rows;
    in.cell_cols = cell_cols;
    in.channels = channels;
    in.max_keypoints = max_keypoints;
    in.min_distance = min_distance;
    in.border = border;
    in.n_occupied = n_occupied;
    *plan = ftk::keypoint_decode_plan(in);
    switch (plan->refused) {
        case ftk::KeypointDecodeRefusal::None:
            return FTK_OK;
        case ftk::KeypointDecodeRefusal::Survivors:
            return ftk_fail(ctx, FTK_E_UNSUPPORTED, "%s: a %d x %d image at min_distance %d can hold more than %d keypoints: raise min_distance", who,
                            cell_rows * FTK_KEYPOINT_DECODE_CELL, cell_cols * FTK_KEYPOINT_DECODE_CELL, min_distance, FTK_HARRIS_DEVICE_MAX_SURVIVORS);
        case ftk::KeypointDecodeRefusal::Keypoints:
            return ftk_fail(ctx, FTK_E_INVALID_ARGUMENT, "%s: max_keypoints %d outside 1 .. %d", who, max_keypoints, FTK_KEYPOINT_DECODE_MAX_KEYPOINTS);
        case ftk::KeypointDecodeRefusal::Channels:
            return ftk_fail(ctx, FTK_E_INVALID_ARGUMENT, "%s: %d descriptor channels outside 1 .. %d", who, channels, FTK_KEYPOINT_DECODE_MAX_CHANNELS);
        default:
            return ftk_fail(ctx, FTK_E_INVALID_ARGUMENT, "%s: bad sizes (a %d x %d cell grid, border %d, %d occupied points)", who, cell_rows, cell_cols,
                            border, n_occupied);
    }
}

}  // namespace

extern "C" {

int ftk_keypoint_decode_workspace_bytes(int32_t cell_rows, int32_t cell_cols, int32_t min_distance, int32_t n_occupied, int64_t *bytes) {
    const char *who = "keypoint_decode_workspace_bytes";
    return ftk_workspace_bytes<ftk::KeypointDecodePlan>(
        who, bytes, [&](ftk::KeypointDecodePlan *plan) { return plan_call(nullptr, who, cell_rows, cell_cols, 1, 1, min_distance, 0, n_occupied, plan); });
}

int ftk_keypoint_decode_device(ftk_context *ctx, void *stream, const float *d_semi, int32_t cell_rows, int32_t cell_cols, const float *d_desc,
                               int32_t channels, int64_t desc_stride_c, int64_t desc_stride_y, int64_t desc_stride_x, int32_t max_keypoints,
                               float min_score, int32_t min_distance, int32_t border, const float *d_occupied_uv, const uint8_t *d_occupied_flags,
                               int32_t n_occupied, void *d_workspace, float *d_uv, float *d_scores, float *d_descriptors, int32_t *d_count,
                               float *d_heatmap) {
    if (!ctx) {
        return ftk_fail(nullptr, FTK_E_INVALID_ARGUMENT, "keypoint_decode_device: null context");
    }
    FTK_LOCK(ctx);
    ftk::KeypointDecodePlan plan;
    const int rc = plan_call(ctx, "keypoint_decode_device", cell_rows, cell_cols, channels, max_keypoints, min_distance, border, n_occupied, &plan);
    if (rc != FTK_OK) {
        return rc;
    }
    if (!d_semi || !d_desc || !d_workspace || !d_uv || !d_scores || !d_descriptors || !d_count || (n_occupied > 0 && !d_occupied_uv)) {
        return ftk_fail(ctx, FTK_E_INVALID_ARGUMENT, "keypoint_decode_device: null buffer");
    }
    if (!(min_score >= -3.0e38f) || !(min_score <= 3.0e38f)) {
        return ftk_fail(ctx, FTK_E_INVALID_ARGUMENT, "keypoint_decode_device: min_score %g must be finite", (double)min_score);
    }
    if (desc_stride_c < 0 || desc_stride_y < 0 || desc_stride_x < 0) {
        return ftk_fail(ctx, FTK_E_INVALID_ARGUMENT, "keypoint_decode_device: the descriptor strides (%lld, %lld, %lld) must not be negative",
                        (long long)desc_stride_c, (long long)desc_stride_y, (long long)desc_stride_x);
    }
    if (!ftk_aligned(d_workspace, 16) || !ftk_aligned(d_uv, 8) || !ftk_aligned(d_semi, 4) || !ftk_aligned(d_desc, 4) || !ftk_aligned(d_scores, 4) ||
        !ftk_aligned(d_descriptors, 4) || !ftk_aligned(d_count, 4) || !ftk_aligned(d_heatmap, 4)) {
        return ftk_fail(ctx, FTK_E_INVALID_ARGUMENT, "keypoint_decode_device: the workspace must be 16-byte aligned, d_uv 8-byte, the others 4-byte");
    }
    ftk::KeypointDecodeParams p{};
    p.score.semi = d_semi;
    p.score.cell_rows = cell_rows;
    p.score.cell_cols = cell_cols;
    p.score.min_score = min_score;
    p.score.border = border;
    p.score.key = plan.key.in(d_workspace);
    p.score.heatmap = d_heatmap;
    p.select.rows = plan.rows;
    p.select.cols = plan.cols;
    p.select.reach = plan.reach;
    p.select.key = p.score.key;
    p.select.tmp = plan.tmp.in(d_workspace);
    p.select.wmax = plan.wmax.in(d_workspace);
    p.select.list = plan.list.in(d_workspace);
    p.select.count = plan.count.in(d_workspace);
    p.select.capacity = (unsigned)plan.capacity;
    p.occupied.uv = d_occupied_uv;
    p.occupied.flags = d_occupied_flags;
    p.occupied.n = n_occupied;
    p.occupied.plane = n_occupied > 0 ? plan.plane.in(d_workspace) : nullptr;
    p.occupied.dilated = n_occupied > 0 ? plan.dilated.in(d_workspace) : nullptr;
    p.rank.list = p.select.list;
    p.rank.count = p.select.count;
    p.rank.capacity = p.select.capacity;
    p.rank.cols = plan.cols;
    p.rank.uv_out = d_uv;
    p.rank.count_out = d_count;
    p.rank.max_count = max_keypoints;
    p.rank.score_out = d_scores;
    p.describe.desc = d_desc;
    p.describe.stride_c = desc_stride_c;
    p.describe.stride_y = desc_stride_y;
    p.describe.stride_x = desc_stride_x;
    p.describe.cell_rows = cell_rows;
    p.describe.cell_cols = cell_cols;
    p.describe.channels = channels;
    p.describe.uv = d_uv;
    p.describe.count = d_count;
    p.describe.max_keypoints = max_keypoints;
    p.describe.descriptors = d_descriptors;
    FTK_HIP(ctx, hipSetDevice(ctx->device));
    FTK_HIP(ctx, ftk::keypoint_decode_launch(plan, p, static_cast<hipStream_t>(stream)));
    return FTK_OK;
}

}  // extern "C"
