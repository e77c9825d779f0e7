// ftk_flow_points.cpp — sparse tracking from RAFT's coarse flow of the C ABI (include/ftk.h): feature points through the flow of
// Raft.UpsampleFlow (model.py:48-64) without storing it.
#include <math.h>

#include "ftk_internal.h"

extern "C" {

int ftk_flow_track_points_device(ftk_context *ctx, void *stream, const float *d_flow, const float *d_mask, const float *d_flow_back,
                                 const float *d_mask_back, int32_t B, int32_t H, int32_t W, int32_t N, int32_t image_rows, int32_t image_cols,
                                 float mask_scale, float fb_threshold, const float *d_points, float *d_cur_points, uint8_t *d_status,
                                 float *d_fb_error2) {
    if (!ctx) {
        return ftk_fail(nullptr, FTK_E_INVALID_ARGUMENT, "flow_track_points_device: null context");
    }
    FTK_LOCK(ctx);
    if (!d_flow || !d_mask || (N != 0 && (!d_points || !d_cur_points || !d_status))) {  // no points: their buffers are empty and may have no address
        return ftk_fail(ctx, FTK_E_INVALID_ARGUMENT, "flow_track_points_device: null argument");
    }
    if ((d_flow_back == nullptr) != (d_mask_back == nullptr)) {
        return ftk_fail(ctx, FTK_E_INVALID_ARGUMENT, "flow_track_points_device: half a backward pair (%s is null): pass both or neither",
                        d_flow_back ? "d_mask_back" : "d_flow_back");
    }
    if (B < 1 || H < 1 || W < 1 || N < 0) {
        return ftk_fail(ctx, FTK_E_INVALID_ARGUMENT, "flow_track_points_device: sizes B %d, H %d, W %d must be positive and N %d not negative", B, H, W, N);
    }
    constexpr int32_t kMaxCoarse = (1 << 24) / 8;  // float32 coordinates name every fine pixel up to 2^24
    if (H > kMaxCoarse || W > kMaxCoarse) {
        return ftk_fail(ctx, FTK_E_INVALID_ARGUMENT, "flow_track_points_device: sizes H %d, W %d above %d: float32 points cannot name the fine pixels", H, W,
                        kMaxCoarse);
    }
    if (image_rows < 1 || image_rows > 8 * H || image_cols < 1 || image_cols > 8 * W) {
        return ftk_fail(ctx, FTK_E_INVALID_ARGUMENT, "flow_track_points_device: image of %d x %d outside 1 .. %d x 1 .. %d, the grid of the flow", image_rows,
                        image_cols, 8 * H, 8 * W);
    }
    if (!isfinite(mask_scale)) {
        return ftk_fail(ctx, FTK_E_INVALID_ARGUMENT, "flow_track_points_device: mask_scale %g is not finite", (double)mask_scale);
    }
    if (!(fb_threshold >= 0.0f)) {
        return ftk_fail(ctx, FTK_E_INVALID_ARGUMENT, "flow_track_points_device: fb_threshold %g is negative or NaN", (double)fb_threshold);
    }
    // the largest buffers: the mask, 576 floats per coarse pixel, and the points, 2 floats each
    if ((int64_t)B * H > INT64_MAX / 2304 / W) {  // B * H < 2^62
        return ftk_fail(ctx, FTK_E_INVALID_ARGUMENT, "flow_track_points_device: a mask of B %d, %d x %d does not fit in a byte count", B, H, W);
    }
    if ((int64_t)B * N > INT64_MAX / 8) {
        return ftk_fail(ctx, FTK_E_INVALID_ARGUMENT, "flow_track_points_device: B %d x N %d points do not fit in a byte count", B, N);
    }
    if (N == 0) {
        return FTK_OK;
    }
    FTK_HIP(ctx, hipSetDevice(ctx->device));
    ftk::FlowPointsParams p{};
    p.flow = d_flow;
    p.mask = d_mask;
    p.flow_back = d_flow_back;
    p.mask_back = d_mask_back;
    p.points = d_points;
    p.cur_points = d_cur_points;
    p.status = d_status;
    p.fb_error2 = d_fb_error2;
    p.B = B;
    p.H = H;
    p.W = W;
    p.N = N;
    p.image_rows = image_rows;
    p.image_cols = image_cols;
    p.mask_scale = mask_scale;
    p.fb_threshold = fb_threshold;
    FTK_HIP(ctx, ftk::flow_track_points_launch(p, static_cast<hipStream_t>(stream)));
    return FTK_OK;
}

}  // extern "C"
