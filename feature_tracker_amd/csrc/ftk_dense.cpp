// ftk_dense.cpp — dense optical flow (Farneback) of the C ABI (include/ftk.h).
#include <math.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "ftk_internal.h"

namespace {

struct DenseLayout {
    float4 *mom_ref, *mom_cur;
    float *raw_r, *raw_c, *smooth_r, *smooth_c;
    float k[3];
};

// Checks the options and levels [lo, hi] of both pyramids, makes the Gaussian table resident and the workspace large enough
// (never inside a stream capture), and carves the workspace.
int dense_setup(ftk_context *ctx, const char *who, const ftk_dense_flow_options *opt, const ftk_pyramid *ref, const ftk_pyramid *cur, int32_t lo,
                int32_t hi, DenseLayout *L) {
    const int32_t half = opt->half_patch;
    size_t ref_px = 1, cur_px = 1;
    for (int32_t l = lo; l <= hi; ++l) {
        const DevImage a = ref->levels[l], b = cur->levels[l];
        if (a.rows <= 0 || a.cols <= 0 || b.rows <= 0 || b.cols <= 0 || !a.data || !b.data) {
            return ftk_fail(ctx, FTK_E_INVALID_ARGUMENT, "%s: level %d is empty", who, l);
        }
        ref_px = std::max(ref_px, (size_t)a.rows * a.cols);
        cur_px = std::max(cur_px, (size_t)b.rows * b.cols);
    }
    ftk_layout ws;
    const auto s_mom_ref = ws.take<float4>(2 * ref_px), s_mom_cur = ws.take<float4>(2 * cur_px);
    const auto s_raw_r = ws.take<float>(ref_px), s_raw_c = ws.take<float>(ref_px), s_smooth_r = ws.take<float>(ref_px), s_smooth_c = ws.take<float>(ref_px);
    const size_t need = ws.bytes();
    if (need > ctx->dense_ws.bytes() || ctx->dense_half != half) {
        if (ftk_stream_capturing(ctx->stream)) {
            return ftk_fail(ctx, FTK_E_UNSUPPORTED, "%s: the workspace (%zu bytes) or the Gaussian table of half patch %d is not resident yet and "
                            "cannot be allocated while the stream is being captured: make one call of this shape and half patch before the capture", who,
                            need, half);
        }
    }
    std::vector<float> w((size_t)(2 * half + 1) * (2 * half + 1));
    L->k[0] = opt->k_moments[0];
    L->k[1] = opt->k_moments[1];
    L->k[2] = opt->k_moments[2];
    int rc = ftk_dense_flow_gaussian(half, w.data(), L->k);
    if (rc != FTK_OK) {
        return ftk_fail(ctx, rc, "%s: half_patch %d outside [0, %d]", who, half, FTK_DENSE_MAX_HALF_PATCH);
    }
    if (ctx->dense_half != half) {
        ctx->dense_half = -1;
        const size_t bytes = sizeof(float) * w.size();
        FTK_HIP(ctx, ctx->dense_weights.reserve(ctx->stream, bytes, 0, 1));
        rc = ftk_ensure_pinned(ctx, bytes);
        if (rc != FTK_OK) {
            return rc;
        }
        memcpy(ctx->pinned.get(), w.data(), bytes);  // (the copy is ordered behind the launches that still read the old table)
        FTK_HIP(ctx, hipMemcpyAsync(ctx->dense_weights.get(), ctx->pinned.get(), bytes, hipMemcpyHostToDevice, ctx->stream));
        FTK_HIP(ctx, hipStreamSynchronize(ctx->stream));  // the pinned block is reused by the caller right away
        ctx->dense_half = half;
    }
    rc = ftk_ensure_device_buffer(ctx, ctx->dense_ws, ws);
    if (rc != FTK_OK) {
        return rc;
    }
    void *base = ctx->dense_ws.get();
    L->mom_ref = s_mom_ref.in(base);
    L->mom_cur = s_mom_cur.in(base);
    L->raw_r = s_raw_r.in(base);
    L->raw_c = s_raw_c.in(base);
    L->smooth_r = s_smooth_r.in(base);
    L->smooth_c = s_smooth_c.in(base);
    return FTK_OK;
}

// One level: moments of ref and cur, the per-pixel refinement (initial flow per `init`), the median into out_r / out_c.
int dense_level(ftk_context *ctx, const ftk_dense_flow_options *opt, const DenseLayout &L, DevImage ref, DevImage cur, int32_t init, int32_t flow_valid,
                const float *init_r, const float *init_c, int32_t init_rows, int32_t init_cols, float *out_r, float *out_c) {
    ftk::DenseMomentsParams mp;
    mp.img[0] = ref;
    mp.img[1] = cur;
    mp.mom[0] = L.mom_ref;
    mp.mom[1] = L.mom_cur;
    mp.weights = ctx->dense_weights.as<float>();
    mp.half = opt->half_patch;
    FTK_HIP(ctx, ftk::dense_moments_launch(mp, ctx->stream));
    ftk::DenseFlowParams fp;
    fp.mom_ref = L.mom_ref;
    fp.mom_cur = L.mom_cur;
    fp.ref_rows = ref.rows;
    fp.ref_cols = ref.cols;
    fp.cur_rows = cur.rows;
    fp.cur_cols = cur.cols;
    fp.k2 = L.k[0];
    fp.k4 = L.k[1];
    fp.k22 = L.k[2];
    fp.max_iteration = opt->max_iteration;
    fp.converge = opt->max_converge_step;
    fp.max_step = opt->max_delta_flow_step;
    fp.init = init;
    fp.flow_valid = flow_valid;
    fp.init_r = init_r;
    fp.init_c = init_c;
    fp.init_rows = init_rows;
    fp.init_cols = init_cols;
    fp.out_r = L.raw_r;
    fp.out_c = L.raw_c;
    FTK_HIP(ctx, ftk::dense_flow_launch(fp, ctx->stream));
    ftk::DenseMedianParams md;
    md.in_r = L.raw_r;
    md.in_c = L.raw_c;
    md.out_r = out_r;
    md.out_c = out_c;
    md.rows = ref.rows;
    md.cols = ref.cols;
    FTK_HIP(ctx, ftk::dense_median_launch(md, ctx->stream));
    return FTK_OK;
}

}  // namespace

extern "C" {

void ftk_default_dense_flow_options(ftk_dense_flow_options *opt) {
    if (!opt) {
        return;
    }
    opt->max_iteration = 10;  // dense_optical_flow.h:15-20
    opt->half_patch = 2;
    opt->max_converge_step = 1e-6f;
    opt->max_delta_flow_step = 1.0f;
    opt->k_moments[0] = opt->k_moments[1] = opt->k_moments[2] = 0.0f;
}

int ftk_dense_flow_gaussian(int32_t half_patch, float *weights_out, float *k_out) {
    if (half_patch < 0 || half_patch > FTK_DENSE_MAX_HALF_PATCH) {
        return ftk_fail(nullptr, FTK_E_INVALID_ARGUMENT, "dense_flow_gaussian: half_patch %d outside [0, %d]", half_patch, FTK_DENSE_MAX_HALF_PATCH);
    }
    // InitializeGaussianKernel (dense_optical_flow.cpp:87-134)
    const int32_t center = half_patch, size = 2 * center + 1;
    std::vector<float> w((size_t)size * size, 0.0f);
    if (center == 0) {  // :95-98: [1], k2 / k4 / k22 not recomputed
        w[0] = 1.0f;
    } else {
        const float sigma = 1.0f, sigma2 = sigma * sigma;
        float sum = 0.0f;
        for (int32_t row = 0; row < size; ++row) {  // :106-113
            for (int32_t col = 0; col < size; ++col) {
                const int32_t dr = row - center, dc = col - center;
                w[(size_t)row * size + col] = expf(-0.5f * (float)(dr * dr + dc * dc) / sigma2);
                sum += w[(size_t)row * size + col];
            }
        }
        for (float &v : w) {  // :116
            v /= sum;
        }
        float k2 = 0.0f, k4 = 0.0f, k22 = 0.0f;  // :119-131, each product left to right
        for (int32_t row = 0; row < size; ++row) {
            for (int32_t col = 0; col < size; ++col) {
                const float fr = (float)(row - center), fc = (float)(col - center), wt = w[(size_t)row * size + col];
                k2 += wt * fr * fr;
                k4 += wt * fr * fr * fr * fr;
                k22 += wt * fr * fr * fc * fc;
            }
        }
        if (k_out) {
            k_out[0] = k2;
            k_out[1] = k4;
            k_out[2] = k22;
        }
    }
    if (weights_out) {
        memcpy(weights_out, w.data(), sizeof(float) * w.size());
    }
    return FTK_OK;
}

int ftk_dense_flow_device(ftk_context *ctx, const ftk_dense_flow_options *opt, const ftk_pyramid *ref_pyr, const ftk_pyramid *cur_pyr, float *d_flow_r,
                          float *d_flow_c) {
    if (!ctx) {
        return ftk_fail(nullptr, FTK_E_INVALID_ARGUMENT, "dense_flow_device: null context");
    }
    FTK_LOCK(ctx);
    if (!opt || !ref_pyr || !cur_pyr || !d_flow_r || !d_flow_c) {
        return ftk_fail(ctx, FTK_E_INVALID_ARGUMENT, "dense_flow_device: null argument");
    }
    if (ref_pyr->n_levels != cur_pyr->n_levels || ref_pyr->n_levels < 1) {
        return ftk_fail(ctx, FTK_E_INVALID_ARGUMENT, "dense_flow_device: level counts %d and %d (the reference returns false unless they are equal)",
                        ref_pyr->n_levels, cur_pyr->n_levels);
    }
    FTK_HIP(ctx, hipSetDevice(ctx->device));
    const DevImage ref0 = ref_pyr->levels[0];
    if (opt->half_patch < 0) {
        // every per-level Track returns false before it touches the flow (:12) and the pyramid overload ignores it (:53): the
        // zero flow of the coarsest level, upsampled to level 0, is zero
        const size_t bytes = sizeof(float) * (size_t)ref0.rows * ref0.cols;
        FTK_HIP(ctx, hipMemsetAsync(d_flow_r, 0, bytes, ctx->stream));
        FTK_HIP(ctx, hipMemsetAsync(d_flow_c, 0, bytes, ctx->stream));
        return FTK_OK;
    }
    DenseLayout L;
    const int32_t top = ref_pyr->n_levels - 1;
    int rc = dense_setup(ctx, "dense_flow_device", opt, ref_pyr, cur_pyr, 0, top, &L);
    if (rc != FTK_OK) {
        return rc;
    }
    for (int32_t level = top; level >= 0; --level) {
        const DevImage coarse = ref_pyr->levels[level < top ? level + 1 : top];
        rc = dense_level(ctx, opt, L, ref_pyr->levels[level], cur_pyr->levels[level], level == top ? 0 : 2, 0, L.smooth_r, L.smooth_c, coarse.rows,
                         coarse.cols, level == 0 ? d_flow_r : L.smooth_r, level == 0 ? d_flow_c : L.smooth_c);
        if (rc != FTK_OK) {
            return rc;
        }
    }
    return FTK_OK;
}

int ftk_dense_flow(ftk_context *ctx, const ftk_dense_flow_options *opt, const ftk_pyramid *ref_pyr, const ftk_pyramid *cur_pyr, float *flow_r,
                   float *flow_c) {
    FTK_TRACE_SCOPE("ftk_dense_flow");
    if (!ctx) {
        return ftk_fail(nullptr, FTK_E_INVALID_ARGUMENT, "dense_flow: null context");
    }
    FTK_LOCK(ctx);
    if (!ref_pyr || !flow_r || !flow_c || ref_pyr->n_levels < 1) {
        return ftk_fail(ctx, FTK_E_INVALID_ARGUMENT, "dense_flow: null argument");
    }
    FTK_HIP(ctx, hipSetDevice(ctx->device));
    const size_t px = (size_t)ref_pyr->levels[0].rows * ref_pyr->levels[0].cols;
    ftk_layout L;
    const auto s_r = L.take<float>(px), s_c = L.take<float>(px);
    int rc = ftk_ensure_scratch(ctx, L);
    if (rc != FTK_OK) {
        return rc;
    }
    float *d_r = s_r.in(ctx->scratch.get()), *d_c = s_c.in(ctx->scratch.get());
    rc = ftk_dense_flow_device(ctx, opt, ref_pyr, cur_pyr, d_r, d_c);
    if (rc != FTK_OK) {
        (void)hipStreamSynchronize(ctx->stream);
        return rc;
    }
    rc = ftk_ensure_pinned(ctx, L);  // after the device entry: it stages the Gaussian table through this block
    if (rc != FTK_OK) {
        return rc;
    }
    void *h = ctx->pinned.get();
    FTK_HIP(ctx, hipMemcpyAsync(s_r.in(h), d_r, s_r.size_bytes(), hipMemcpyDeviceToHost, ctx->stream));
    FTK_HIP(ctx, hipMemcpyAsync(s_c.in(h), d_c, s_c.size_bytes(), hipMemcpyDeviceToHost, ctx->stream));
    FTK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    memcpy(flow_r, s_r.in(h), s_r.size_bytes());
    memcpy(flow_c, s_c.in(h), s_c.size_bytes());
    return FTK_OK;
}

int ftk_dense_flow_level(ftk_context *ctx, const ftk_dense_flow_options *opt, const ftk_pyramid *ref_pyr, const ftk_pyramid *cur_pyr, int32_t level,
                         float *flow_r, float *flow_c, int32_t flow_valid) {
    FTK_TRACE_SCOPE("ftk_dense_flow_level");
    if (!ctx) {
        return ftk_fail(nullptr, FTK_E_INVALID_ARGUMENT, "dense_flow_level: null context");
    }
    FTK_LOCK(ctx);
    if (!opt || !ref_pyr || !cur_pyr || !flow_r || !flow_c || level < 0 || level >= ref_pyr->n_levels || level >= cur_pyr->n_levels) {
        return ftk_fail(ctx, FTK_E_INVALID_ARGUMENT, "dense_flow_level: bad arguments (level %d)", level);
    }
    if (opt->half_patch < 0) {
        return ftk_fail(ctx, FTK_E_INVALID_ARGUMENT, "dense_flow_level: half_patch %d < 0 (the reference returns false, the flow untouched)", opt->half_patch);
    }
    FTK_HIP(ctx, hipSetDevice(ctx->device));
    DenseLayout L;
    int rc = dense_setup(ctx, "dense_flow_level", opt, ref_pyr, cur_pyr, level, level, &L);
    if (rc != FTK_OK) {
        return rc;
    }
    const DevImage ref = ref_pyr->levels[level];
    ftk_layout H;  // the pinned block: [flow_r | flow_c]
    const auto s_r = H.take<float>((size_t)ref.rows * ref.cols), s_c = H.take<float>((size_t)ref.rows * ref.cols);
    rc = ftk_ensure_pinned(ctx, H);
    if (rc != FTK_OK) {
        return rc;
    }
    void *h = ctx->pinned.get();
    if (flow_valid & 1) {
        memcpy(s_r.in(h), flow_r, s_r.size_bytes());
        FTK_HIP(ctx, hipMemcpyAsync(L.raw_r, s_r.in(h), s_r.size_bytes(), hipMemcpyHostToDevice, ctx->stream));
    }
    if (flow_valid & 2) {
        memcpy(s_c.in(h), flow_c, s_c.size_bytes());
        FTK_HIP(ctx, hipMemcpyAsync(L.raw_c, s_c.in(h), s_c.size_bytes(), hipMemcpyHostToDevice, ctx->stream));
    }
    rc = dense_level(ctx, opt, L, ref, cur_pyr->levels[level], 1, flow_valid & 3, L.raw_r, L.raw_c, ref.rows, ref.cols, L.smooth_r, L.smooth_c);
    if (rc != FTK_OK) {
        (void)hipStreamSynchronize(ctx->stream);
        return rc;
    }
    FTK_HIP(ctx, hipMemcpyAsync(s_r.in(h), L.smooth_r, s_r.size_bytes(), hipMemcpyDeviceToHost, ctx->stream));
    FTK_HIP(ctx, hipMemcpyAsync(s_c.in(h), L.smooth_c, s_c.size_bytes(), hipMemcpyDeviceToHost, ctx->stream));
    FTK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    memcpy(flow_r, s_r.in(h), s_r.size_bytes());
    memcpy(flow_c, s_c.in(h), s_c.size_bytes());
    return FTK_OK;
}

}  // extern "C"
