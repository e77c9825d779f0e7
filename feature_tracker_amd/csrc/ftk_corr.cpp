// ftk_corr.cpp — the RAFT all-pairs correlation pyramid of the C ABI (include/ftk.h): layout, build, lookup (correlation_volumes.py).
#include <math.h>

#include <algorithm>

#include "ftk_internal.h"

extern "C" {

int ftk_corr_pyramid_layout(int32_t B, int32_t H, int32_t W, int32_t levels, int64_t *elements, int64_t *level_offsets, int32_t *level_h,
                            int32_t *level_w) {
    if (!elements) {
        return ftk_fail(nullptr, FTK_E_INVALID_ARGUMENT, "corr_pyramid_layout: null output");
    }
    if (B < 1 || H < 1 || W < 1) {
        return ftk_fail(nullptr, FTK_E_INVALID_ARGUMENT, "corr_pyramid_layout: sizes B %d, H %d, W %d must be positive", B, H, W);
    }
    if (levels < 1 || levels > FTK_CORR_MAX_LEVELS) {
        return ftk_fail(nullptr, FTK_E_INVALID_ARGUMENT, "corr_pyramid_layout: %d levels (1 .. %d)", levels, FTK_CORR_MAX_LEVELS);
    }
    const int64_t slabs = (int64_t)B * H * W;  // < 2^63: each factor < 2^31
    int64_t total = 0;
    int32_t h = H, w = W;
    for (int32_t l = 0; l < levels; ++l) {
        if (h == 0 || w == 0) {
            return ftk_fail(nullptr, FTK_E_INVALID_ARGUMENT,
                            "corr_pyramid_layout: level %d of a %d x %d volume would be %d x %d (the reference's avg_pool2d raises): use at most %d levels",
                            l, H, W, h, w, l);
        }
        const int64_t hw = (int64_t)h * w;
        if (slabs > (INT64_MAX - total) / hw) {
            return ftk_fail(nullptr, FTK_E_INVALID_ARGUMENT, "corr_pyramid_layout: the volume of B %d, %d x %d, %d levels overflows int64", B, H, W, levels);
        }
        if (level_offsets) {
            level_offsets[l] = total;
        }
        if (level_h) {
            level_h[l] = h;
        }
        if (level_w) {
            level_w[l] = w;
        }
        total += slabs * hw;
        h /= 2;
        w /= 2;
    }
    if (total > INT64_MAX / 4) {
        return ftk_fail(nullptr, FTK_E_INVALID_ARGUMENT, "corr_pyramid_layout: %lld elements do not fit in a byte count", (long long)total);
    }
    *elements = total;
    return FTK_OK;
}

int ftk_corr_pyramid_build_device(ftk_context *ctx, void *stream, const float *d_fmap0, const float *d_fmap1, int32_t B, int32_t C, int32_t H,
                                  int32_t W, int32_t levels, float *d_volume) {
    if (!ctx) {
        return ftk_fail(nullptr, FTK_E_INVALID_ARGUMENT, "corr_pyramid_build_device: null context");
    }
    FTK_LOCK(ctx);
    if (!d_fmap0 || !d_fmap1 || !d_volume) {
        return ftk_fail(ctx, FTK_E_INVALID_ARGUMENT, "corr_pyramid_build_device: null argument");
    }
    if (C < 1) {
        return ftk_fail(ctx, FTK_E_INVALID_ARGUMENT, "corr_pyramid_build_device: %d channels", C);
    }
    int64_t elements = 0, off[FTK_CORR_MAX_LEVELS];
    int32_t lh[FTK_CORR_MAX_LEVELS], lw[FTK_CORR_MAX_LEVELS];
    if (ftk_corr_pyramid_layout(B, H, W, levels, &elements, off, lh, lw) != FTK_OK) {
        return ftk_fail(ctx, FTK_E_INVALID_ARGUMENT, "corr_pyramid_build_device: %s", ftk_last_error(nullptr));
    }
    if ((int64_t)B * C * H * W > INT64_MAX / 4) {
        return ftk_fail(ctx, FTK_E_INVALID_ARGUMENT, "corr_pyramid_build_device: feature maps too large");
    }
    FTK_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    ftk::CorrBuildParams p{};
    p.f0 = d_fmap0;
    p.f1 = d_fmap1;
    p.volume = d_volume;
    p.B = B;
    p.C = C;
    p.H = H;
    p.W = W;
    p.divisor = (float)sqrt((double)C);  // correlation / (channels ** 0.5): a double scalar, cast to float by torch (:46)
    p.fused = std::min(levels - 1, ftk::corr_fused_levels());
    for (int l = 0; l < 4; ++l) {
        p.level_offset[l] = l < levels ? off[l] : 0;
        p.level_h[l] = l < levels ? lh[l] : 0;
        p.level_w[l] = l < levels ? lw[l] : 0;
    }
    FTK_HIP(ctx, ftk::corr_build_launch(p, s));
    // deeper levels (:31-34), each from the one before it
    const int64_t slabs = (int64_t)B * H * W;
    for (int32_t l = p.fused + 1; l < levels; ++l) {
        FTK_HIP(ctx, ftk::corr_pool_launch(d_volume + off[l - 1], d_volume + off[l], slabs, lh[l - 1], lw[l - 1], lh[l], lw[l], s));
    }
    return FTK_OK;
}

int ftk_corr_pyramid_lookup_device(ftk_context *ctx, void *stream, const float *d_volume, int32_t B, int32_t H, int32_t W, int32_t levels,
                                   int32_t radius, const float *d_coords, float *d_out, int32_t per_level) {
    if (!ctx) {
        return ftk_fail(nullptr, FTK_E_INVALID_ARGUMENT, "corr_pyramid_lookup_device: null context");
    }
    FTK_LOCK(ctx);
    if (!d_volume || !d_coords || !d_out) {
        return ftk_fail(ctx, FTK_E_INVALID_ARGUMENT, "corr_pyramid_lookup_device: null argument");
    }
    if (radius < 0 || radius > FTK_CORR_MAX_RADIUS) {
        return ftk_fail(ctx, FTK_E_INVALID_ARGUMENT, "corr_pyramid_lookup_device: radius %d (0 .. %d)", radius, FTK_CORR_MAX_RADIUS);
    }
    int64_t elements = 0;
    ftk::CorrLookupParams p{};
    if (ftk_corr_pyramid_layout(B, H, W, levels, &elements, p.level_offset, p.level_h, p.level_w) != FTK_OK) {
        return ftk_fail(ctx, FTK_E_INVALID_ARGUMENT, "corr_pyramid_lookup_device: %s", ftk_last_error(nullptr));
    }
    FTK_HIP(ctx, hipSetDevice(ctx->device));
    p.volume = d_volume;
    p.coords = d_coords;
    p.out = d_out;
    p.B = B;
    p.H = H;
    p.W = W;
    p.levels = levels;
    p.radius = radius;
    p.per_level = per_level ? 1 : 0;
    FTK_HIP(ctx, ftk::corr_lookup_launch(p, static_cast<hipStream_t>(stream)));
    return FTK_OK;
}

}  // extern "C"
