// ftk_flow_upsample.cpp — RAFT's convex flow upsampling of the C ABI (include/ftk.h): Raft.UpsampleFlow (model.py:48-64).
#include <math.h>

#include "ftk_internal.h"

extern "C" {

int ftk_flow_upsample_device(ftk_context *ctx, void *stream, const float *d_flow, const float *d_mask, int32_t B, int32_t H, int32_t W,
                             float mask_scale, float *d_out) {
    if (!ctx) {
        return ftk_fail(nullptr, FTK_E_INVALID_ARGUMENT, "flow_upsample_device: null context");
    }
    FTK_LOCK(ctx);
    if (!d_flow || !d_mask || !d_out) {
        return ftk_fail(ctx, FTK_E_INVALID_ARGUMENT, "flow_upsample_device: null argument");
    }
    if (B < 1 || H < 1 || W < 1) {
        return ftk_fail(ctx, FTK_E_INVALID_ARGUMENT, "flow_upsample_device: sizes B %d, H %d, W %d must be positive", B, H, W);
    }
    if (!isfinite(mask_scale)) {
        return ftk_fail(ctx, FTK_E_INVALID_ARGUMENT, "flow_upsample_device: mask_scale %g is not finite", (double)mask_scale);
    }
    // the mask is the largest of the three buffers: 576 floats per coarse pixel (the output has 128)
    if ((int64_t)B * H > INT64_MAX / 2304 / W) {  // B * H < 2^62
        return ftk_fail(ctx, FTK_E_INVALID_ARGUMENT, "flow_upsample_device: a mask of B %d, %d x %d does not fit in a byte count", B, H, W);
    }
    FTK_HIP(ctx, hipSetDevice(ctx->device));
    ftk::FlowUpsampleParams p{};
    p.flow = d_flow;
    p.mask = d_mask;
    p.out = d_out;
    p.B = B;
    p.H = H;
    p.W = W;
    p.mask_scale = mask_scale;
    FTK_HIP(ctx, ftk::flow_upsample_launch(p, static_cast<hipStream_t>(stream)));
    return FTK_OK;
}

}  // extern "C"
