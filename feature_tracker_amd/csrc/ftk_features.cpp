// ftk_features.cpp — the producers of the trackers' and matchers' input behind the C ABI (include/ftk.h): BRIEF descriptors,
// Harris corners, and the 6 x 6 LDLT diagnostic.
#include <string.h>

#include <algorithm>
#include <vector>

#include "ftk_internal.h"

namespace {

int harris_run(ftk_context *ctx, const ftk_pyramid *image, int32_t level, int32_t min_distance, float min_response, float *response_out,
                      std::vector<unsigned long long> *survivors) {
    if (!image || level < 0 || level >= image->n_levels) {
        return ftk_fail(ctx, FTK_E_INVALID_ARGUMENT, "harris: bad image / level");
    }
    FTK_HIP(ctx, hipSetDevice(ctx->device));
    const DevImage img = image->levels[level];
    const size_t px = (size_t)img.rows * img.cols;
    const size_t capacity = px;  // worst case (min_distance 1): every candidate is its own window maximum
    const size_t g_bytes = ftk_align_up(sizeof(short) * px, 256), f_bytes = ftk_align_up(sizeof(float) * px, 256);
    const size_t k_bytes = ftk_align_up(sizeof(unsigned long long) * px, 256), l_bytes = ftk_align_up(sizeof(unsigned long long) * capacity, 256);
    const int rc = ftk_ensure_scratch(ctx, 2 * g_bytes + f_bytes + 3 * k_bytes + l_bytes + 256);
    if (rc != FTK_OK) {
        return rc;
    }
    uint8_t *base = ctx->scratch.as<uint8_t>();
    ftk::HarrisParams p;
    p.img = img;
    p.gx = reinterpret_cast<short *>(base);
    p.gy = reinterpret_cast<short *>(base + g_bytes);
    p.response = response_out ? reinterpret_cast<float *>(base + 2 * g_bytes) : nullptr;
    p.key = reinterpret_cast<unsigned long long *>(base + 2 * g_bytes + f_bytes);
    p.tmp = p.key + k_bytes / sizeof(unsigned long long);
    p.wmax = p.tmp + k_bytes / sizeof(unsigned long long);
    p.list = survivors ? p.wmax + k_bytes / sizeof(unsigned long long) : nullptr;
    p.count = reinterpret_cast<unsigned *>(base + 2 * g_bytes + f_bytes + 3 * k_bytes + l_bytes);
    p.capacity = (unsigned)capacity;
    p.min_distance = min_distance;
    p.min_response = min_response;
    FTK_HIP(ctx, ftk::harris_launch(p, ctx->stream));
    if (response_out) {
        FTK_HIP(ctx, hipMemcpyAsync(response_out, p.response, sizeof(float) * px, hipMemcpyDeviceToHost, ctx->stream));
    }
    if (survivors) {
        unsigned count = 0;
        FTK_HIP(ctx, hipMemcpyAsync(&count, p.count, sizeof(unsigned), hipMemcpyDeviceToHost, ctx->stream));
        FTK_HIP(ctx, hipStreamSynchronize(ctx->stream));
        if (count > p.capacity) {
            return ftk_fail(ctx, FTK_E_UNSUPPORTED, "harris: %u survivors exceed the list capacity %u", count, p.capacity);
        }
        survivors->resize(count);
        if (count > 0) {
            FTK_HIP(ctx, hipMemcpyAsync(survivors->data(), p.list, sizeof(unsigned long long) * count, hipMemcpyDeviceToHost, ctx->stream));
            FTK_HIP(ctx, hipStreamSynchronize(ctx->stream));
        }
    } else {
        FTK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    }
    return FTK_OK;
}

}  // namespace

// The sampling pattern of (n_bits, half) resident on the device.
int ftk_ensure_brief_pattern(ftk_context *ctx, int32_t n_bits, int32_t half) {
    if (ctx->brief_pattern && ctx->brief_bits == n_bits && ctx->brief_half == half) {
        return FTK_OK;
    }
    ctx->brief_bits = 0;
    // LCG pattern: x <- 1664525 x + 1013904223 (seed 0x2545F491), offset = ((x >> 8) mod (2 half + 1)) - half
    std::vector<int8_t> pattern((size_t)4 * n_bits);
    uint32_t state = 0x2545F491u;
    const uint32_t span = (uint32_t)(2 * half + 1);
    for (auto &v : pattern) {
        state = state * 1664525u + 1013904223u;
        v = (int8_t)((int32_t)((state >> 8) % span) - half);
    }
    FTK_HIP(ctx, ctx->brief_pattern.reserve(ctx->stream, pattern.size(), 0, 1));
    // through the pinned block on the context's stream: a pageable hipMemcpy on the null stream costs milliseconds the first time
    const int prc = ftk_ensure_pinned(ctx, pattern.size());
    if (prc != FTK_OK) {
        return prc;
    }
    memcpy(ctx->pinned.get(), pattern.data(), pattern.size());
    FTK_HIP(ctx, hipMemcpyAsync(ctx->brief_pattern.get(), ctx->pinned.get(), pattern.size(), hipMemcpyHostToDevice, ctx->stream));
    FTK_HIP(ctx, hipStreamSynchronize(ctx->stream));  // the pinned block is reused by the caller right away
    ctx->brief_bits = n_bits;
    ctx->brief_half = half;
    return FTK_OK;
}

extern "C" {

int ftk_brief_compute_device(ftk_context *ctx, const ftk_pyramid *image, int32_t level, const float *d_uv, int32_t n, int32_t n_bits,
                             int32_t half_patch, uint32_t *d_words) {
    if (!ctx) {
        return ftk_fail(nullptr, FTK_E_INVALID_ARGUMENT, "brief_compute_device: null context");
    }
    FTK_LOCK(ctx);
    if (!image || level < 0 || level >= image->n_levels || n < 0 || n_bits <= 0 || half_patch <= 0 || half_patch > 63) {
        return ftk_fail(ctx, FTK_E_INVALID_ARGUMENT, "brief_compute_device: bad arguments (n %d, bits %d, half %d)", n, n_bits, half_patch);
    }
    if (n == 0) {
        return FTK_OK;
    }
    if (!d_uv || !d_words) {
        return ftk_fail(ctx, FTK_E_INVALID_ARGUMENT, "brief_compute_device: null buffer");
    }
    FTK_HIP(ctx, hipSetDevice(ctx->device));
    const int rc = ftk_ensure_brief_pattern(ctx, n_bits, half_patch);
    if (rc != FTK_OK) {
        return rc;
    }
    ftk::BriefParams p;
    p.img = image->levels[level];
    p.uv = d_uv;
    p.words = d_words;
    p.pattern = ctx->brief_pattern.as<int8_t>();
    p.n = n;
    p.n_bits = n_bits;
    p.n_words = (n_bits + 31) / 32;
    p.half = half_patch;
    FTK_HIP(ctx, ftk::brief_launch(p, ctx->stream));
    return FTK_OK;
}

int ftk_brief_compute(ftk_context *ctx, const ftk_pyramid *image, int32_t level, const float *uv, int32_t n, int32_t n_bits,
                      int32_t half_patch, uint32_t *words) {
    FTK_TRACE_SCOPE("ftk_brief_compute");
    if (!ctx) {
        return ftk_fail(nullptr, FTK_E_INVALID_ARGUMENT, "brief_compute: null context");
    }
    FTK_LOCK(ctx);
    if (n < 0 || n_bits <= 0) {
        return ftk_fail(ctx, FTK_E_INVALID_ARGUMENT, "brief_compute: bad sizes");
    }
    if (n == 0) {
        return FTK_OK;
    }
    if (!uv || !words) {
        return ftk_fail(ctx, FTK_E_INVALID_ARGUMENT, "brief_compute: null buffer");
    }
    FTK_HIP(ctx, hipSetDevice(ctx->device));
    const size_t n_words = (size_t)(n_bits + 31) / 32;
    const size_t uv_bytes = ftk_align_up(sizeof(float) * 2 * (size_t)n, 256);
    const size_t w_bytes = ftk_align_up(sizeof(uint32_t) * n_words * (size_t)n, 256);
    int rc = ftk_ensure_scratch(ctx, uv_bytes + w_bytes);
    if (rc != FTK_OK) {
        return rc;
    }
    if (n_bits <= 0 || half_patch <= 0 || half_patch > 63) {
        return ftk_fail(ctx, FTK_E_INVALID_ARGUMENT, "brief_compute: bad arguments (bits %d, half %d)", n_bits, half_patch);
    }
    rc = ftk_ensure_brief_pattern(ctx, n_bits, half_patch);  // before the pinned block is filled: it stages the pattern there
    if (rc == FTK_OK) {
        rc = ftk_ensure_pinned(ctx, uv_bytes + w_bytes);
    }
    if (rc != FTK_OK) {
        return rc;
    }
    uint8_t *base = ctx->scratch.as<uint8_t>(), *hbase = ctx->pinned.as<uint8_t>();
    float *d_uv = reinterpret_cast<float *>(base);
    uint32_t *d_words = reinterpret_cast<uint32_t *>(base + uv_bytes);
    memcpy(hbase, uv, sizeof(float) * 2 * (size_t)n);
    FTK_HIP(ctx, hipMemcpyAsync(d_uv, hbase, sizeof(float) * 2 * (size_t)n, hipMemcpyHostToDevice, ctx->stream));
    rc = ftk_brief_compute_device(ctx, image, level, d_uv, n, n_bits, half_patch, d_words);
    if (rc != FTK_OK) {
        (void)hipStreamSynchronize(ctx->stream);
        return rc;
    }
    FTK_HIP(ctx, hipMemcpyAsync(hbase + uv_bytes, d_words, sizeof(uint32_t) * n_words * (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
    FTK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    memcpy(words, hbase + uv_bytes, sizeof(uint32_t) * n_words * (size_t)n);
    return FTK_OK;
}

int ftk_harris_response(ftk_context *ctx, const ftk_pyramid *image, int32_t level, float *response) {
    FTK_TRACE_SCOPE("ftk_harris_response");
    if (!ctx) {
        return ftk_fail(nullptr, FTK_E_INVALID_ARGUMENT, "harris_response: null context");
    }
    FTK_LOCK(ctx);
    if (!response) {
        return ftk_fail(ctx, FTK_E_INVALID_ARGUMENT, "harris_response: null buffer");
    }
    return harris_run(ctx, image, level, 1, 0.0f, response, nullptr);
}

int ftk_harris_detect(ftk_context *ctx, const ftk_pyramid *image, int32_t level, int32_t max_count, int32_t min_distance, float min_response,
                      float *uv, int32_t *n_out) {
    FTK_TRACE_SCOPE("ftk_harris_detect");
    if (!ctx) {
        return ftk_fail(nullptr, FTK_E_INVALID_ARGUMENT, "harris_detect: null context");
    }
    FTK_LOCK(ctx);
    if (!n_out || max_count < 0 || (max_count > 0 && !uv)) {
        return ftk_fail(ctx, FTK_E_INVALID_ARGUMENT, "harris_detect: bad output arguments");
    }
    *n_out = 0;
    if (!image || level < 0 || level >= image->n_levels) {
        return ftk_fail(ctx, FTK_E_INVALID_ARGUMENT, "harris_detect: bad image / level");
    }
    const DevImage img = image->levels[level];
    if (max_count == 0 || img.rows < 23 || img.cols < 23) {
        return FTK_OK;
    }
    std::vector<unsigned long long> survivors;
    const int rc = harris_run(ctx, image, level, min_distance, min_response, nullptr, &survivors);
    if (rc != FTK_OK) {
        return rc;
    }
    // key order == (response descending, pixel index ascending): the final top-N selection is a sort of
    // a few thousand 64-bit keys on the host
    std::sort(survivors.begin(), survivors.end(), [](unsigned long long a, unsigned long long b) { return a > b; });
    const size_t n = survivors.size() < (size_t)max_count ? survivors.size() : (size_t)max_count;
    for (size_t i = 0; i < n; ++i) {
        const unsigned idx = 0xFFFFFFFFu - (unsigned)(survivors[i] & 0xFFFFFFFFull);
        uv[2 * i] = (float)(idx % (unsigned)img.cols);
        uv[2 * i + 1] = (float)(idx / (unsigned)img.cols);
    }
    *n_out = (int32_t)n;
    return FTK_OK;
}

int ftk_ldlt6_solve(ftk_context *ctx, const float *a, const float *b, float *x, int32_t n) {
    FTK_TRACE_SCOPE("ftk_ldlt6_solve");
    if (!ctx) {
        return ftk_fail(nullptr, FTK_E_INVALID_ARGUMENT, "ldlt6_solve: null context");
    }
    FTK_LOCK(ctx);
    if (n < 0 || (n > 0 && (!a || !b || !x))) {
        return ftk_fail(ctx, FTK_E_INVALID_ARGUMENT, "ldlt6_solve: bad arguments");
    }
    if (n == 0) {
        return FTK_OK;
    }
    FTK_HIP(ctx, hipSetDevice(ctx->device));
    const size_t a_bytes = ftk_align_up(sizeof(float) * 36 * (size_t)n, 256), b_bytes = ftk_align_up(sizeof(float) * 6 * (size_t)n, 256);
    const int rc = ftk_ensure_scratch(ctx, a_bytes + 2 * b_bytes);
    if (rc != FTK_OK) {
        return rc;
    }
    uint8_t *base = ctx->scratch.as<uint8_t>();
    float *d_a = reinterpret_cast<float *>(base), *d_b = reinterpret_cast<float *>(base + a_bytes), *d_x = reinterpret_cast<float *>(base + a_bytes + b_bytes);
    FTK_HIP(ctx, hipMemcpyAsync(d_a, a, sizeof(float) * 36 * (size_t)n, hipMemcpyHostToDevice, ctx->stream));
    FTK_HIP(ctx, hipMemcpyAsync(d_b, b, sizeof(float) * 6 * (size_t)n, hipMemcpyHostToDevice, ctx->stream));
    FTK_HIP(ctx, ftk::ldlt6_launch(d_a, d_b, d_x, n, ctx->stream));
    FTK_HIP(ctx, hipMemcpyAsync(x, d_x, sizeof(float) * 6 * (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
    FTK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return FTK_OK;
}

}  // extern "C"
