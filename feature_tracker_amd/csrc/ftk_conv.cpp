// ftk_conv.cpp — the stock layers of RAFT's UpdateBlock of the C ABI (include/ftk.h): the nine convolutions of update_block.py:4-67,
// DESIGN.md 5.14; and the same layer with a stride, a residual and the image normalisation for its encoders (encoder.py:4-68).
#include <cmath>

#include "ftk_internal.h"
#include "raft_conv_plan.h"

extern "C" {

int ftk_conv2d_packed_elements(int32_t out_channels, int32_t in_channels, int32_t kernel_size, int64_t *elements) {
    if (!elements || out_channels < 1 || in_channels < 1) {
        return ftk_fail(nullptr, FTK_E_INVALID_ARGUMENT, "conv2d_packed_elements: null result or non-positive channel count");
    }
    if ((kernel_size != 1 && kernel_size != 3 && kernel_size != 7) || out_channels > FTK_CONV2D_MAX_OUT_CHANNELS || in_channels > FTK_CONV2D_MAX_IN_CHANNELS) {
        return ftk_fail(nullptr, FTK_E_UNSUPPORTED, "conv2d_packed_elements: kernel_size %d, %d x %d channels outside the supported sizes", kernel_size,
                        out_channels, in_channels);
    }
    *elements = ftk::raft_conv_packed_elements(out_channels, in_channels, kernel_size);
    return FTK_OK;
}

}  // extern "C"

// The checks, the plan and the launch of both entries; `strided` names the caller.  stride 1 with no residual and no normalisation is
// conv2d_kernel's plain form, whichever entry asks.
static int conv2d_entry(const char *what, ftk_context *ctx, void *stream, const ftk_gru_part *parts, int32_t n_parts, const float *d_weights,
                        const float *d_bias, int32_t out_channels, int32_t kernel_size, int32_t stride, int32_t relu, float out_scale,
                        const float *d_residual, int32_t normalise, int32_t B, int32_t H, int32_t W, float *d_out) {
    if (!ctx) {
        return ftk_fail(nullptr, FTK_E_INVALID_ARGUMENT, "%s: null context", what);
    }
    FTK_LOCK(ctx);
    if (!d_weights || !d_bias || !d_out) {
        return ftk_fail(ctx, FTK_E_INVALID_ARGUMENT, "%s: null argument", what);
    }
    if (!parts || n_parts < 1 || n_parts > FTK_CONV2D_MAX_PARTS) {
        return ftk_fail(ctx, FTK_E_INVALID_ARGUMENT, "%s: the input must be 1 .. %d parts (got %d)", what, FTK_CONV2D_MAX_PARTS, n_parts);
    }
    int64_t in_channels = 0;
    for (int32_t i = 0; i < n_parts; ++i) {
        if (!parts[i].data || parts[i].channels < 1) {
            return ftk_fail(ctx, FTK_E_INVALID_ARGUMENT, "%s: part %d of the input is null or has no channels", what, i);
        }
        in_channels += parts[i].channels;
    }
    if (B < 1 || H < 1 || W < 1) {
        return ftk_fail(ctx, FTK_E_INVALID_ARGUMENT, "%s: sizes B %d, H %d, W %d must be positive", what, B, H, W);
    }
    if (!std::isfinite(out_scale)) {
        return ftk_fail(ctx, FTK_E_INVALID_ARGUMENT, "%s: out_scale must be finite", what);
    }
    if (kernel_size != 1 && kernel_size != 3 && kernel_size != 7) {
        return ftk_fail(ctx, FTK_E_UNSUPPORTED, "%s: kernel_size %d is not supported (1, 3 and 7 are)", what, kernel_size);
    }
    if ((stride != 1 && stride != 2) || (stride == 2 && kernel_size == 7)) {
        return ftk_fail(ctx, FTK_E_UNSUPPORTED, "%s: stride %d with kernel_size %d is not supported (stride 1, and stride 2 with kernel sizes 1 and 3, are)",
                        what, stride, kernel_size);
    }
    if (out_channels < 1 || out_channels > FTK_CONV2D_MAX_OUT_CHANNELS) {
        return ftk_fail(ctx, FTK_E_UNSUPPORTED, "%s: out_channels %d outside 1 .. FTK_CONV2D_MAX_OUT_CHANNELS = %d", what, out_channels,
                        FTK_CONV2D_MAX_OUT_CHANNELS);
    }
    if (in_channels > FTK_CONV2D_MAX_IN_CHANNELS) {
        return ftk_fail(ctx, FTK_E_UNSUPPORTED, "%s: in_channels %lld above FTK_CONV2D_MAX_IN_CHANNELS = %d", what, (long long)in_channels,
                        FTK_CONV2D_MAX_IN_CHANNELS);
    }
    if ((int64_t)B * H > INT64_MAX / 16 / FTK_CONV2D_MAX_IN_CHANNELS / W) {
        return ftk_fail(ctx, FTK_E_INVALID_ARGUMENT, "%s: a tensor of B %d, %d x %d does not fit in a byte count", what, B, H, W);
    }
    ftk::ConvPlanInput in{};
    in.out_channels = out_channels, in.in_channels = (int32_t)in_channels, in.kernel_size = kernel_size, in.B = B, in.H = H, in.W = W, in.stride = stride;
    const ftk::ConvPlan plan = ftk::raft_conv_plan(in);
    if (plan.refused != ftk::ConvRefusal::None) {
        return ftk_fail(ctx, FTK_E_UNSUPPORTED, "%s: B %d, %d x %d does not fit a launch (%s)", what, B, H, W, ftk::conv_refusal_name(plan.refused));
    }
    ftk::ConvStridedParams sp{};
    ftk::ConvParams &p = sp.base;
    for (int32_t i = 0; i < n_parts; ++i) {
        p.seg[i].data = parts[i].data;
        p.seg[i].channels = parts[i].channels;
    }
    p.n_seg = n_parts;
    p.weights = d_weights, p.bias = d_bias, p.out = d_out, p.out_scale = out_scale;
    p.out_channels = out_channels, p.in_channels = (int32_t)in_channels, p.B = B, p.H = H, p.W = W;
    sp.residual = d_residual, sp.OH = plan.out_h, sp.OW = plan.out_w, sp.normalise = normalise != 0;
    FTK_HIP(ctx, hipSetDevice(ctx->device));
    FTK_HIP(ctx, ftk::raft_conv_strided_launch(plan, sp, kernel_size, relu != 0, static_cast<hipStream_t>(stream)));
    return FTK_OK;
}

extern "C" {

// update_block.py:7-14 (FlowHead), :21-35 with :37-40 (MotionEncoder: each Conv2d with the ReLU after it; :39's cat is the parts of
// out_conv.0), :57-59 with :66 (the mask head; :66's 0.25 is out_scale of its last layer)
int ftk_conv2d_device(ftk_context *ctx, void *stream, const ftk_gru_part *parts, int32_t n_parts, const float *d_weights, const float *d_bias,
                      int32_t out_channels, int32_t kernel_size, int32_t relu, float out_scale, int32_t B, int32_t H, int32_t W, float *d_out) {
    return conv2d_entry("conv2d_device", ctx, stream, parts, n_parts, d_weights, d_bias, out_channels, kernel_size, 1, relu, out_scale, nullptr, 0, B, H, W,
                        d_out);
}

// encoder.py:7-13 with :16-22 (ResNetBlock: conv1 + bn1 + ReLU; shortcut + its BatchNorm; conv2 + bn2 + the add + ReLU), :30-31 and :46-47
// (conv_in, conv_out) and model.py:70-71 (the normalisation, at conv_in's fetch)
int ftk_conv2d_strided_device(ftk_context *ctx, void *stream, const ftk_gru_part *parts, int32_t n_parts, const float *d_weights, const float *d_bias,
                              int32_t out_channels, int32_t kernel_size, int32_t stride, int32_t relu, float out_scale, const float *d_residual,
                              int32_t normalise, int32_t B, int32_t H, int32_t W, float *d_out) {
    return conv2d_entry("conv2d_strided_device", ctx, stream, parts, n_parts, d_weights, d_bias, out_channels, kernel_size, stride, relu, out_scale,
                        d_residual, normalise, B, H, W, d_out);
}

}  // extern "C"
