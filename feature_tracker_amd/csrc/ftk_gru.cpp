// ftk_gru.cpp — RAFT's separable ConvGRU of the C ABI (include/ftk.h): SepConvGru.forward (gru.py:59-76), DESIGN.md 5.13.
#include "ftk_internal.h"
#include "sep_conv_gru_plan.h"

namespace {

// The checks both entries share; on success `plan` and the segments of `p` (the x parts, then `last`) are set.
int gru_prepare(ftk_context *ctx, const char *what, const ftk_gru_part *x_parts, int32_t n_parts, const float *last, int32_t h_channels,
                int32_t kernel_size, int32_t vertical, int32_t gates, int32_t B, int32_t H, int32_t W, ftk::SepConvGruPlan &plan, ftk::SepConvGruParams &p) {
    if (!x_parts || n_parts < 1 || n_parts > FTK_SEP_CONV_GRU_MAX_PARTS) {
        return ftk_fail(ctx, FTK_E_INVALID_ARGUMENT, "%s: x must be 1 .. %d parts (got %d)", what, FTK_SEP_CONV_GRU_MAX_PARTS, n_parts);
    }
    int64_t in_channels = h_channels;
    for (int32_t i = 0; i < n_parts; ++i) {
        if (!x_parts[i].data || x_parts[i].channels < 1) {
            return ftk_fail(ctx, FTK_E_INVALID_ARGUMENT, "%s: part %d of x is null or has no channels", what, i);
        }
        in_channels += x_parts[i].channels;
    }
    if (B < 1 || H < 1 || W < 1) {
        return ftk_fail(ctx, FTK_E_INVALID_ARGUMENT, "%s: sizes B %d, H %d, W %d must be positive", what, B, H, W);
    }
    if (kernel_size != 3 && kernel_size != 5) {
        return ftk_fail(ctx, FTK_E_UNSUPPORTED, "%s: kernel_size %d is not supported (3 and 5 are)", what, kernel_size);
    }
    if (h_channels < 1 || h_channels > FTK_SEP_CONV_GRU_MAX_H_CHANNELS) {
        return ftk_fail(ctx, FTK_E_UNSUPPORTED, "%s: h_channels %d outside 1 .. FTK_SEP_CONV_GRU_MAX_H_CHANNELS = %d", what, h_channels,
                        FTK_SEP_CONV_GRU_MAX_H_CHANNELS);
    }
    if (in_channels > FTK_SEP_CONV_GRU_MAX_IN_CHANNELS) {
        return ftk_fail(ctx, FTK_E_UNSUPPORTED, "%s: x_channels + h_channels = %lld above FTK_SEP_CONV_GRU_MAX_IN_CHANNELS = %d", what,
                        (long long)in_channels, FTK_SEP_CONV_GRU_MAX_IN_CHANNELS);
    }
    if ((int64_t)B * H > INT64_MAX / 16 / FTK_SEP_CONV_GRU_MAX_IN_CHANNELS / W) {
        return ftk_fail(ctx, FTK_E_INVALID_ARGUMENT, "%s: an input of B %d, %d x %d does not fit in a byte count", what, B, H, W);
    }
    ftk::SepConvGruPlanInput in{};
    in.h_channels = h_channels, in.in_channels = (int32_t)in_channels, in.kernel_size = kernel_size, in.vertical = vertical != 0, in.gates = gates;
    in.B = B, in.H = H, in.W = W;
    plan = ftk::sep_conv_gru_plan(in);
    if (plan.refused != ftk::GruRefusal::None) {
        return ftk_fail(ctx, FTK_E_UNSUPPORTED, "%s: B %d, %d x %d does not fit a launch (%s)", what, B, H, W, ftk::gru_refusal_name(plan.refused));
    }
    for (int32_t i = 0; i < n_parts; ++i) {
        p.seg[i].data = x_parts[i].data;
        p.seg[i].channels = x_parts[i].channels;
    }
    p.seg[n_parts].data = last;
    p.seg[n_parts].channels = h_channels;
    p.n_seg = n_parts + 1;
    p.h_channels = h_channels, p.in_channels = (int32_t)in_channels, p.B = B, p.H = H, p.W = W;
    return FTK_OK;
}

}  // namespace

extern "C" {

int ftk_sep_conv_gru_packed_elements(int32_t out_channels, int32_t in_channels, int32_t kernel_size, int64_t *elements) {
    if (!elements || out_channels < 1 || in_channels < 1) {
        return ftk_fail(nullptr, FTK_E_INVALID_ARGUMENT, "sep_conv_gru_packed_elements: null result or non-positive channel count");
    }
    if ((kernel_size != 3 && kernel_size != 5) || out_channels > 2 * FTK_SEP_CONV_GRU_MAX_H_CHANNELS || in_channels > FTK_SEP_CONV_GRU_MAX_IN_CHANNELS) {
        return ftk_fail(nullptr, FTK_E_UNSUPPORTED, "sep_conv_gru_packed_elements: kernel_size %d, %d x %d channels outside the supported sizes", kernel_size,
                        out_channels, in_channels);
    }
    *elements = ftk::sep_conv_gru_packed_elements(out_channels, in_channels, kernel_size);
    return FTK_OK;
}

// gru.py:59-76: lines 64-66 (horizontal) and 71-73 (vertical): z = sigmoid(conv_z(cat[x, h])), r = sigmoid(conv_r(cat[x, h])), r * h
int ftk_sep_conv_gru_gates_device(ftk_context *ctx, void *stream, const ftk_gru_part *x_parts, int32_t n_parts, const float *d_h, const float *d_weights,
                                  const float *d_bias, int32_t h_channels, int32_t kernel_size, int32_t vertical, int32_t B, int32_t H, int32_t W, float *d_z,
                                  float *d_rh) {
    if (!ctx) {
        return ftk_fail(nullptr, FTK_E_INVALID_ARGUMENT, "sep_conv_gru_gates_device: null context");
    }
    FTK_LOCK(ctx);
    if (!d_h || !d_weights || !d_bias || !d_z || !d_rh) {
        return ftk_fail(ctx, FTK_E_INVALID_ARGUMENT, "sep_conv_gru_gates_device: null argument");
    }
    ftk::SepConvGruPlan plan{};
    ftk::SepConvGruParams p{};
    const int rc = gru_prepare(ctx, "sep_conv_gru_gates_device", x_parts, n_parts, d_h, h_channels, kernel_size, vertical, 1, B, H, W, plan, p);
    if (rc != FTK_OK) {
        return rc;
    }
    p.weights = d_weights, p.bias = d_bias, p.h = d_h, p.z = d_z, p.rh = d_rh;
    FTK_HIP(ctx, hipSetDevice(ctx->device));
    FTK_HIP(ctx, ftk::sep_conv_gru_launch(plan, p, kernel_size, vertical != 0, 1, static_cast<hipStream_t>(stream)));
    return FTK_OK;
}

// gru.py:59-76: lines 66-68 and 73-75: q = tanh(conv_q(cat[x, r * h])), h = (1 - z) * h + z * q
int ftk_sep_conv_gru_blend_device(ftk_context *ctx, void *stream, const ftk_gru_part *x_parts, int32_t n_parts, const float *d_rh, const float *d_z,
                                  const float *d_h, const float *d_weights, const float *d_bias, int32_t h_channels, int32_t kernel_size, int32_t vertical,
                                  int32_t B, int32_t H, int32_t W, float *d_out) {
    if (!ctx) {
        return ftk_fail(nullptr, FTK_E_INVALID_ARGUMENT, "sep_conv_gru_blend_device: null context");
    }
    FTK_LOCK(ctx);
    if (!d_rh || !d_z || !d_h || !d_weights || !d_bias || !d_out) {
        return ftk_fail(ctx, FTK_E_INVALID_ARGUMENT, "sep_conv_gru_blend_device: null argument");
    }
    ftk::SepConvGruPlan plan{};
    ftk::SepConvGruParams p{};
    const int rc = gru_prepare(ctx, "sep_conv_gru_blend_device", x_parts, n_parts, d_rh, h_channels, kernel_size, vertical, 0, B, H, W, plan, p);
    if (rc != FTK_OK) {
        return rc;
    }
    p.weights = d_weights, p.bias = d_bias, p.h = d_h, p.z = const_cast<float *>(d_z), p.out = d_out;
    FTK_HIP(ctx, hipSetDevice(ctx->device));
    FTK_HIP(ctx, ftk::sep_conv_gru_launch(plan, p, kernel_size, vertical != 0, 0, static_cast<hipStream_t>(stream)));
    return FTK_OK;
}

}  // extern "C"
