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
    ftk_layout L;
    const auto s_gx = L.take<short>(px), s_gy = L.take<short>(px);
    const auto s_response = L.take<float>(px);
    const auto s_key = L.take<unsigned long long>(px), s_tmp = L.take<unsigned long long>(px), s_wmax = L.take<unsigned long long>(px);
    const auto s_list = L.take<unsigned long long>(capacity);
    const auto s_count = L.take<unsigned>(1);
    const int rc = ftk_ensure_scratch(ctx, L);
    if (rc != FTK_OK) {
        return rc;
    }
    void *base = ctx->scratch.get();
    ftk::HarrisParams p;
    p.img = img;
    p.gx = s_gx.in(base);
    p.gy = s_gy.in(base);
    p.response = response_out ? s_response.in(base) : nullptr;
    p.key = s_key.in(base);
    p.tmp = s_tmp.in(base);
    p.wmax = s_wmax.in(base);
    p.list = survivors ? s_list.in(base) : nullptr;
    p.count = s_count.in(base);
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
    if (n_bits <= 0 || half_patch <= 0 || half_patch > 63) {
        return ftk_fail(ctx, FTK_E_INVALID_ARGUMENT, "brief_compute: bad arguments (bits %d, half %d)", n_bits, half_patch);
    }
    ftk_layout L;
    const auto s_uv = L.take<float>(2 * (size_t)n);
    const auto s_words = L.take<uint32_t>(n_words * (size_t)n);
    int rc = ftk_ensure_brief_pattern(ctx, n_bits, half_patch);  // before the pinned block is filled: it stages the pattern there
    if (rc != FTK_OK) {
        return rc;
    }
    uint8_t *base = nullptr, *hbase = nullptr;
    rc = ftk_ensure_mirror(ctx, L, &base, &hbase);
    if (rc != FTK_OK) {
        return rc;
    }
    memcpy(s_uv.in(hbase), uv, s_uv.size_bytes());
    FTK_HIP(ctx, hipMemcpyAsync(s_uv.in(base), s_uv.in(hbase), s_uv.size_bytes(), hipMemcpyHostToDevice, ctx->stream));
    rc = ftk_brief_compute_device(ctx, image, level, s_uv.in(base), n, n_bits, half_patch, s_words.in(base));
    if (rc != FTK_OK) {
        (void)hipStreamSynchronize(ctx->stream);
        return rc;
    }
    FTK_HIP(ctx, hipMemcpyAsync(s_words.in(hbase), s_words.in(base), s_words.size_bytes(), hipMemcpyDeviceToHost, ctx->stream));
    FTK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    memcpy(words, s_words.in(hbase), s_words.size_bytes());
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
    ftk_layout L;
    const auto s_a = L.take<float>(36 * (size_t)n), s_b = L.take<float>(6 * (size_t)n), s_x = L.take<float>(6 * (size_t)n);
    const int rc = ftk_ensure_scratch(ctx, L);
    if (rc != FTK_OK) {
        return rc;
    }
    void *base = ctx->scratch.get();
    float *d_a = s_a.in(base), *d_b = s_b.in(base), *d_x = s_x.in(base);
    FTK_HIP(ctx, hipMemcpyAsync(d_a, a, s_a.size_bytes(), hipMemcpyHostToDevice, ctx->stream));
    FTK_HIP(ctx, hipMemcpyAsync(d_b, b, s_b.size_bytes(), hipMemcpyHostToDevice, ctx->stream));
    FTK_HIP(ctx, ftk::ldlt6_launch(d_a, d_b, d_x, n, ctx->stream));
    FTK_HIP(ctx, hipMemcpyAsync(x, d_x, s_x.size_bytes(), hipMemcpyDeviceToHost, ctx->stream));
    FTK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return FTK_OK;
}

}  // extern "C"
