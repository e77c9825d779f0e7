// ftk_raft_layers.cpp — the layers of RAFT's update block and encoders of the C ABI (include/ftk.h), all launches of raft_gemm_core.h's
// implicit GEMM over an input given as parts: the separable ConvGRU (SepConvGru.forward, gru.py:59-76), the nine stock
// convolutions of update_block.py:4-67, the same layer with a stride, a residual and the image normalisation for the
// encoders (encoder.py:4-68) and with a 2 x 2 max-pool in its epilogue for SuperPoint's VGG.
#include <cmath>

#include "ftk_internal.h"
#include "raft_conv_plan.h"
#include "sep_conv_gru_plan.h"

namespace {

// What the checks every entry shares are told about their caller: its name, its limits and its wording.
struct PartsInput {
    const char *what;   // the entry
    const char *noun;   // what the parts are parts of
    const char *sized;  // the same, as the byte-count refusal names it
    int32_t max_parts, max_in_channels;
};

// The parts and the sizes; the parts' channels are added to `in_channels`.
int check_parts(ftk_context *ctx, const PartsInput &e, const ftk_gru_part *parts, int32_t n_parts, int32_t B, int32_t H, int32_t W, int64_t &in_channels) {
    if (!parts || n_parts < 1 || n_parts > e.max_parts) {
        return ftk_fail(ctx, FTK_E_INVALID_ARGUMENT, "%s: %s must be 1 .. %d parts (got %d)", e.what, e.noun, e.max_parts, n_parts);
    }
    for (int32_t i = 0; i < n_parts; ++i) {
        if (!parts[i].data || parts[i].channels < 1) {
            return ftk_fail(ctx, FTK_E_INVALID_ARGUMENT, "%s: part %d of %s is null or has no channels", e.what, i, e.noun);
        }
        in_channels += parts[i].channels;
    }
    if (B < 1 || H < 1 || W < 1) {
        return ftk_fail(ctx, FTK_E_INVALID_ARGUMENT, "%s: sizes B %d, H %d, W %d must be positive", e.what, B, H, W);
    }
    return FTK_OK;
}

// Every tensor of the call, at the most channels an input may have, fits in a byte count.
int check_bytes(ftk_context *ctx, const PartsInput &e, int32_t B, int32_t H, int32_t W) {
    if ((int64_t)B * H > INT64_MAX / 16 / e.max_in_channels / W) {
        return ftk_fail(ctx, FTK_E_INVALID_ARGUMENT, "%s: %s of B %d, %d x %d does not fit in a byte count", e.what, e.sized, B, H, W);
    }
    return FTK_OK;
}

// The parts as the first segments of a kernel's input; returns their number.
int32_t copy_parts(const ftk_gru_part *parts, int32_t n_parts, ftk::ChannelSegment *seg) {
    for (int32_t i = 0; i < n_parts; ++i) {
        seg[i].data = parts[i].data;
        seg[i].channels = parts[i].channels;
    }
    return n_parts;
}

// The checks both GRU entries share; on success `plan` and the segments of `p` (the x parts, then `last`) are set.
int gru_prepare(ftk_context *ctx, const char *what, const ftk_gru_part *x_parts, int32_t n_parts, const float *last, int32_t h_channels,
                int32_t kernel_size, int32_t vertical, int32_t gates, int32_t B, int32_t H, int32_t W, ftk::SepConvGruPlan &plan, ftk::SepConvGruParams &p) {
    const PartsInput e{what, "x", "an input", FTK_SEP_CONV_GRU_MAX_PARTS, FTK_SEP_CONV_GRU_MAX_IN_CHANNELS};
    int64_t in_channels = h_channels;
    if (const int rc = check_parts(ctx, e, x_parts, n_parts, B, H, W, in_channels)) {
        return rc;
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
    if (const int rc = check_bytes(ctx, e, B, H, W)) {
        return rc;
    }
    ftk::SepConvGruPlanInput in{};
    in.h_channels = h_channels, in.in_channels = (int32_t)in_channels, in.kernel_size = kernel_size, in.vertical = vertical != 0, in.gates = gates;
    in.B = B, in.H = H, in.W = W;
    plan = ftk::sep_conv_gru_plan(in);
    if (plan.refused != ftk::GruRefusal::None) {
        return ftk_fail(ctx, FTK_E_UNSUPPORTED, "%s: B %d, %d x %d does not fit a launch (%s)", what, B, H, W, ftk::gru_refusal_name(plan.refused));
    }
    p.n_seg = copy_parts(x_parts, n_parts, p.seg) + 1;
    p.seg[n_parts].data = last;
    p.seg[n_parts].channels = h_channels;
    p.h_channels = h_channels, p.in_channels = (int32_t)in_channels, p.B = B, p.H = H, p.W = W;
    return FTK_OK;
}

// The checks, the plan and the launch of the three conv entries; `what` names the caller.  stride 1 with no residual and no normalisation is
// conv2d_kernel's plain form, whichever entry asks; `pool` (the pooled entry alone: stride 1, no scale, no residual) is its pooled form.
int conv2d_entry(const char *what, ftk_context *ctx, void *stream, const ftk_gru_part *parts, int32_t n_parts, const float *d_weights, const float *d_bias,
                 int32_t out_channels, int32_t kernel_size, int32_t stride, int32_t relu, float out_scale, const float *d_residual, int32_t normalise,
                 int32_t pool, int32_t B, int32_t H, int32_t W, float *d_out) {
    if (!ctx) {
        return ftk_fail(nullptr, FTK_E_INVALID_ARGUMENT, "%s: null context", what);
    }
    FTK_LOCK(ctx);
    if (!d_weights || !d_bias || !d_out) {
        return ftk_fail(ctx, FTK_E_INVALID_ARGUMENT, "%s: null argument", what);
    }
    const PartsInput e{what, "the input", "a tensor", FTK_CONV2D_MAX_PARTS, FTK_CONV2D_MAX_IN_CHANNELS};
    int64_t in_channels = 0;
    if (const int rc = check_parts(ctx, e, parts, n_parts, B, H, W, in_channels)) {
        return rc;
    }
    if (!std::isfinite(out_scale)) {
        return ftk_fail(ctx, FTK_E_INVALID_ARGUMENT, "%s: out_scale must be finite", what);
    }
    if (kernel_size != 1 && kernel_size != 3 && kernel_size != 7) {
        return ftk_fail(ctx, FTK_E_UNSUPPORTED, "%s: kernel_size %d is not supported (1, 3 and 7 are)", what, kernel_size);
    }
    if (pool && kernel_size == 7) {
        return ftk_fail(ctx, FTK_E_UNSUPPORTED, "%s: kernel_size 7 is not supported with the max-pool (1 and 3 are)", what);
    }
    if (pool && (H < 2 || W < 2)) {
        return ftk_fail(ctx, FTK_E_INVALID_ARGUMENT, "%s: H %d, W %d must be at least 2: the output is floor(H / 2) x floor(W / 2)", what, H, W);
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
    if (const int rc = check_bytes(ctx, e, B, H, W)) {
        return rc;
    }
    ftk::ConvPlanInput in{};
    in.out_channels = out_channels, in.in_channels = (int32_t)in_channels, in.kernel_size = kernel_size, in.B = B, in.H = H, in.W = W, in.stride = stride;
    in.pool = pool ? 1 : 0;
    const ftk::ConvPlan plan = ftk::raft_conv_plan(in);
    if (plan.refused != ftk::ConvRefusal::None) {
        return ftk_fail(ctx, FTK_E_UNSUPPORTED, "%s: B %d, %d x %d does not fit a launch (%s)", what, B, H, W, ftk::conv_refusal_name(plan.refused));
    }
    ftk::ConvStridedParams sp{};
    ftk::ConvParams &p = sp.base;
    p.n_seg = copy_parts(parts, n_parts, p.seg);
    p.weights = d_weights, p.bias = d_bias, p.out = d_out, p.out_scale = out_scale;
    p.out_channels = out_channels, p.in_channels = (int32_t)in_channels, p.B = B, p.H = H, p.W = W;
    sp.residual = d_residual, sp.OH = plan.out_h, sp.OW = plan.out_w, sp.normalise = normalise != 0;
    FTK_HIP(ctx, hipSetDevice(ctx->device));
    if (pool) {
        FTK_HIP(ctx, ftk::raft_conv_pool_launch(plan, p, kernel_size, relu != 0, static_cast<hipStream_t>(stream)));
        return FTK_OK;
    }
    FTK_HIP(ctx, ftk::raft_conv_strided_launch(plan, sp, kernel_size, relu != 0, static_cast<hipStream_t>(stream)));
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

// update_block.py:7-14 (FlowHead), :21-35 with :37-40 (MotionEncoder: each Conv2d with the ReLU after it; :39's cat is the parts of
// out_conv.0), :57-59 with :66 (the mask head; :66's 0.25 is out_scale of its last layer)
int ftk_conv2d_device(ftk_context *ctx, void *stream, const ftk_gru_part *parts, int32_t n_parts, const float *d_weights, const float *d_bias,
                      int32_t out_channels, int32_t kernel_size, int32_t relu, float out_scale, int32_t B, int32_t H, int32_t W, float *d_out) {
    return conv2d_entry("conv2d_device", ctx, stream, parts, n_parts, d_weights, d_bias, out_channels, kernel_size, 1, relu, out_scale, nullptr, 0, 0, B, H,
                        W, d_out);
}

// encoder.py:7-13 with :16-22 (ResNetBlock: conv1 + bn1 + ReLU; shortcut + its BatchNorm; conv2 + bn2 + the add + ReLU), :30-31 and :46-47
// (conv_in, conv_out) and model.py:70-71 (the normalisation, at conv_in's fetch)
int ftk_conv2d_strided_device(ftk_context *ctx, void *stream, const ftk_gru_part *parts, int32_t n_parts, const float *d_weights, const float *d_bias,
                              int32_t out_channels, int32_t kernel_size, int32_t stride, int32_t relu, float out_scale, const float *d_residual,
                              int32_t normalise, int32_t B, int32_t H, int32_t W, float *d_out) {
    return conv2d_entry("conv2d_strided_device", ctx, stream, parts, n_parts, d_weights, d_bias, out_channels, kernel_size, stride, relu, out_scale,
                        d_residual, normalise, 0, B, H, W, d_out);
}

// SuperPoint's VGG: conv1b, conv2b and conv3b, each with the ReLU and the 2 x 2 max-pool after it
int ftk_conv2d_pool_device(ftk_context *ctx, void *stream, const ftk_gru_part *parts, int32_t n_parts, const float *d_weights, const float *d_bias,
                           int32_t out_channels, int32_t kernel_size, int32_t relu, int32_t B, int32_t H, int32_t W, float *d_out) {
    return conv2d_entry("conv2d_pool_device", ctx, stream, parts, n_parts, d_weights, d_bias, out_channels, kernel_size, 1, relu, 1.0f, nullptr, 0, 1, B, H, W,
                        d_out);
}

}  // extern "C"
