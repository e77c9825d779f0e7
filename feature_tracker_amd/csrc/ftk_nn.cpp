// ftk_nn.cpp — NNFeatureMatcher's post-processing behind the C ABI (include/ftk.h; nn_feature_matcher.cpp:155-216).
#include "ftk_internal.h"
#include "match_plan.h"

namespace {

// The key workspace of the nn_match entries, `count` 8-byte words, all 0.  It grows only outside a stream capture (an allocation is
// not a stream operation: a captured graph would keep launching on the freed block).
int ensure_nn_keys(ftk_context *ctx, const char *who, hipStream_t stream, size_t count) {
    constexpr size_t kWord = sizeof(unsigned long long);
    if (count * kWord <= ctx->nn_keys.bytes()) {
        return FTK_OK;
    }
    if (ftk_stream_capturing(stream)) {
        return ftk_fail(ctx, FTK_E_UNSUPPORTED, "%s: the key workspace holds %zu words and this call needs %zu, and it cannot grow while the stream is being "
                        "captured: make one call of this size (or larger) on this context before the capture", who, ctx->nn_keys.bytes() / kWord, count);
    }
    FTK_HIP(ctx, hipDeviceSynchronize());  // earlier calls, on whatever stream, may still use the old block
    FTK_HIP(ctx, ctx->nn_keys.reserve(ctx->stream, count * kWord, count / 4 * kWord, 512 * kWord));
    FTK_HIP(ctx, hipMemset(ctx->nn_keys.get(), 0, ctx->nn_keys.bytes()));  // 0 = empty; every call leaves it so
    FTK_HIP(ctx, hipDeviceSynchronize());
    return FTK_OK;
}

// The host-array forms: `in_bytes` of input go up, `launch(d_in, d_index, d_status)` runs on the context's stream, n_ref indices and
// statuses come back.  Synchronous.
template <class Launch>
int run_nn_host(ftk_context *ctx, const void *in, size_t in_bytes, int64_t n_out, int32_t *match_index, uint8_t *status, Launch launch) {
    FTK_HIP(ctx, hipSetDevice(ctx->device));
    ftk_layout L;
    const auto s_in = L.take<uint8_t>(in_bytes);
    const auto s_idx = L.take<int32_t>((size_t)n_out);
    const auto s_st = L.take<uint8_t>((size_t)n_out);
    const int rc = ftk_ensure_scratch(ctx, L);
    if (rc != FTK_OK) {
        return rc;
    }
    uint8_t *base = s_in.in(ctx->scratch.get());
    if (in_bytes > 0) {
        FTK_HIP(ctx, hipMemcpyAsync(base, in, in_bytes, hipMemcpyHostToDevice, ctx->stream));
    }
    int32_t *d_idx = s_idx.in(ctx->scratch.get());
    uint8_t *d_st = s_st.in(ctx->scratch.get());
    const int lrc = launch(base, d_idx, d_st);
    if (lrc != FTK_OK) {
        (void)hipStreamSynchronize(ctx->stream);
        return lrc;
    }
    FTK_HIP(ctx, hipMemcpyAsync(match_index, d_idx, s_idx.size_bytes(), hipMemcpyDeviceToHost, ctx->stream));
    FTK_HIP(ctx, hipMemcpyAsync(status, d_st, s_st.size_bytes(), hipMemcpyDeviceToHost, ctx->stream));
    FTK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return FTK_OK;
}

}  // namespace

extern "C" {

int ftk_nn_match_scores_device(ftk_context *ctx, void *stream, const float *d_scores, int32_t batch, int32_t n_ref, int32_t n_cur, int64_t row_stride,
                               int64_t batch_stride, float min_score, int32_t *d_match_index, uint8_t *d_status) {
    if (!ctx) {
        return ftk_fail(nullptr, FTK_E_INVALID_ARGUMENT, "nn_match_scores_device: null context");
    }
    FTK_LOCK(ctx);
    if (batch < 0 || n_ref < 0 || n_cur < 0) {
        return ftk_fail(ctx, FTK_E_INVALID_ARGUMENT, "nn_match_scores_device: negative size (batch %d, n_ref %d, n_cur %d)", batch, n_ref, n_cur);
    }
    if (batch == 0 || n_ref == 0) {
        return FTK_OK;  // nothing to write (nn_feature_matcher.cpp:92 returns false on an empty reference set: the callers' business)
    }
    if (n_cur == 0) {
        return ftk_fail(ctx, FTK_E_INVALID_ARGUMENT, "nn_match_scores_device: n_cur 0 with n_ref %d: a row of no scores has no maximum (the reference would read "
                        "scores(0) of an empty row)", n_ref);
    }
    if (!d_scores || !d_match_index || !d_status) {
        return ftk_fail(ctx, FTK_E_INVALID_ARGUMENT, "nn_match_scores_device: null buffer");
    }
    // rows may not overlap: row_stride >= n_cur, batch_stride >= the extent of one item; the whole extent must fit a byte count
    if (row_stride < n_cur || (n_ref > 1 && row_stride > INT64_MAX / 8 / n_ref)) {
        return ftk_fail(ctx, FTK_E_INVALID_ARGUMENT, "nn_match_scores_device: row stride %lld for %d x %d scores", (long long)row_stride, n_ref, n_cur);
    }
    const int64_t item = (int64_t)(n_ref - 1) * row_stride + n_cur;
    if (batch > 1 && (batch_stride < item || batch_stride > INT64_MAX / 8 / batch)) {
        return ftk_fail(ctx, FTK_E_INVALID_ARGUMENT, "nn_match_scores_device: batch stride %lld below the %lld elements of one item (or too large)",
                        (long long)batch_stride, (long long)item);
    }
    const ftk::NnMatchPlan plan = ftk::nn_match_plan({batch, n_ref, n_cur, row_stride, batch > 1 ? batch_stride : 0,
                                                      (reinterpret_cast<uintptr_t>(d_scores) & 15u) == 0});
    if (!plan.ok) {
        return ftk_fail(ctx, FTK_E_INVALID_ARGUMENT, "nn_match_scores_device: batch %d x (%d + %d) does not fit one launch (batch <= %d, batch * (n_ref + n_cur) < 2^31)",
                        batch, n_ref, n_cur, ftk::kNnMaxBatch);
    }
    FTK_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int rc = ensure_nn_keys(ctx, "nn_match_scores_device", s, plan.key_count);
    if (rc != FTK_OK) {
        return rc;
    }
    ftk::NnMatchParams p{};
    p.scores = d_scores;
    p.row_stride = row_stride;
    p.batch_stride = batch > 1 ? batch_stride : 0;
    p.batch = batch;
    p.n_ref = n_ref;
    p.n_cur = n_cur;
    p.tile_rows = plan.tile_rows;
    p.col_tiles = plan.col_tiles;
    p.min_score = min_score;
    p.row_key = ctx->nn_keys.as<unsigned long long>();
    p.col_key = p.row_key + (size_t)batch * n_ref;
    p.done = reinterpret_cast<unsigned int *>(p.row_key + (size_t)batch * ((size_t)n_ref + n_cur));
    p.match_index = d_match_index;
    p.status = d_status;
    FTK_HIP(ctx, ftk::nn_match_scores_launch(plan, p, s));
    return FTK_OK;
}

int ftk_nn_match_list_device(ftk_context *ctx, void *stream, const int64_t *d_matches, int32_t n_matches, int32_t n_ref, int32_t n_cur,
                             int32_t *d_match_index, uint8_t *d_status) {
    if (!ctx) {
        return ftk_fail(nullptr, FTK_E_INVALID_ARGUMENT, "nn_match_list_device: null context");
    }
    FTK_LOCK(ctx);
    if (n_matches < 0 || n_ref < 0 || n_cur < 0 || n_matches == INT32_MAX) {
        return ftk_fail(ctx, FTK_E_INVALID_ARGUMENT, "nn_match_list_device: bad size (%d matches, n_ref %d, n_cur %d)", n_matches, n_ref, n_cur);
    }
    if (n_ref == 0) {
        return FTK_OK;
    }
    if (!d_match_index || !d_status || (n_matches > 0 && !d_matches)) {
        return ftk_fail(ctx, FTK_E_INVALID_ARGUMENT, "nn_match_list_device: null buffer");
    }
    FTK_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int rc = ensure_nn_keys(ctx, "nn_match_list_device", s, (size_t)n_ref);
    if (rc != FTK_OK) {
        return rc;
    }
    FTK_HIP(ctx, ftk::nn_match_list_launch(reinterpret_cast<const long long *>(d_matches), n_matches, n_ref, n_cur, ctx->nn_keys.as<unsigned long long>(), d_match_index, d_status, s));
    return FTK_OK;
}

int ftk_nn_fill_pixels_device(ftk_context *ctx, void *stream, const int32_t *d_match_index, int32_t n_ref, const float *d_cur_uv, int32_t n_cur,
                              float *d_matched_uv) {
    if (!ctx) {
        return ftk_fail(nullptr, FTK_E_INVALID_ARGUMENT, "nn_fill_pixels_device: null context");
    }
    FTK_LOCK(ctx);
    if (n_ref < 0 || n_cur < 0) {
        return ftk_fail(ctx, FTK_E_INVALID_ARGUMENT, "nn_fill_pixels_device: negative size (n_ref %d, n_cur %d)", n_ref, n_cur);
    }
    if (n_cur == 0) {
        return FTK_OK;  // matched_uv has n_cur entries
    }
    if (!d_cur_uv || !d_matched_uv || (n_ref > 0 && !d_match_index)) {
        return ftk_fail(ctx, FTK_E_INVALID_ARGUMENT, "nn_fill_pixels_device: null buffer");
    }
    if (d_cur_uv == d_matched_uv) {
        return ftk_fail(ctx, FTK_E_INVALID_ARGUMENT, "nn_fill_pixels_device: matched_uv must not alias cur_uv (entries are gathered from cur_uv)");
    }
    FTK_HIP(ctx, hipSetDevice(ctx->device));
    FTK_HIP(ctx, ftk::nn_fill_pixels_launch(d_match_index, n_ref, d_cur_uv, n_cur, d_matched_uv, static_cast<hipStream_t>(stream)));
    return FTK_OK;
}

int ftk_nn_match_scores(ftk_context *ctx, const float *scores, int32_t batch, int32_t n_ref, int32_t n_cur, int64_t row_stride, int64_t batch_stride,
                        float min_score, int32_t *match_index, uint8_t *status, int *matched_ok) {
    FTK_TRACE_SCOPE("ftk_nn_match_scores");
    if (!ctx) {
        return ftk_fail(nullptr, FTK_E_INVALID_ARGUMENT, "nn_match_scores: null context");
    }
    FTK_LOCK(ctx);
    if (matched_ok) {
        *matched_ok = 0;
    }
    if (batch < 0 || n_ref < 0 || n_cur < 0) {
        return ftk_fail(ctx, FTK_E_INVALID_ARGUMENT, "nn_match_scores: negative size (batch %d, n_ref %d, n_cur %d)", batch, n_ref, n_cur);
    }
    if (n_ref == 0 || batch == 0) {
        return FTK_OK;  // nn_feature_matcher.cpp:92 — `return false`
    }
    if (n_cur == 0) {
        return ftk_fail(ctx, FTK_E_INVALID_ARGUMENT, "nn_match_scores: n_cur 0 with n_ref %d: a row of no scores has no maximum (the reference would read "
                        "scores(0) of an empty row)", n_ref);
    }
    if (!scores || !match_index || !status) {
        return ftk_fail(ctx, FTK_E_INVALID_ARGUMENT, "nn_match_scores: null buffer");
    }
    if (row_stride < n_cur || (n_ref > 1 && row_stride > INT64_MAX / 8 / n_ref)) {
        return ftk_fail(ctx, FTK_E_INVALID_ARGUMENT, "nn_match_scores: row stride %lld for %d x %d scores", (long long)row_stride, n_ref, n_cur);
    }
    const int64_t item = (int64_t)(n_ref - 1) * row_stride + n_cur;
    if (batch > 1 && (batch_stride < item || batch_stride > INT64_MAX / 8 / batch)) {
        return ftk_fail(ctx, FTK_E_INVALID_ARGUMENT, "nn_match_scores: batch stride %lld below the %lld elements of one item (or too large)",
                        (long long)batch_stride, (long long)item);
    }
    if ((int64_t)batch * n_ref >= (1ll << 31)) {
        return ftk_fail(ctx, FTK_E_INVALID_ARGUMENT, "nn_match_scores: batch %d x n_ref %d does not fit one launch", batch, n_ref);
    }
    const int64_t extent = (batch > 1 ? (int64_t)(batch - 1) * batch_stride : 0) + item;  // elements from the first score to the last
    const int rc = run_nn_host(ctx, scores, sizeof(float) * (size_t)extent, (int64_t)batch * n_ref, match_index, status,
                               [&](uint8_t *d_in, int32_t *d_idx, uint8_t *d_st) {
                                   return ftk_nn_match_scores_device(ctx, ctx->stream, reinterpret_cast<float *>(d_in), batch, n_ref, n_cur, row_stride,
                                                                     batch_stride, min_score, d_idx, d_st);
                               });
    if (rc == FTK_OK && matched_ok) {
        *matched_ok = 1;
    }
    return rc;
}

int ftk_nn_match_list(ftk_context *ctx, const int64_t *matches, int32_t n_matches, int32_t n_ref, int32_t n_cur, int32_t *match_index, uint8_t *status,
                      int *matched_ok) {
    FTK_TRACE_SCOPE("ftk_nn_match_list");
    if (!ctx) {
        return ftk_fail(nullptr, FTK_E_INVALID_ARGUMENT, "nn_match_list: null context");
    }
    FTK_LOCK(ctx);
    if (matched_ok) {
        *matched_ok = 0;
    }
    if (n_matches < 0 || n_ref < 0 || n_cur < 0 || n_matches == INT32_MAX) {
        return ftk_fail(ctx, FTK_E_INVALID_ARGUMENT, "nn_match_list: bad size (%d matches, n_ref %d, n_cur %d)", n_matches, n_ref, n_cur);
    }
    if (n_ref == 0) {
        return FTK_OK;  // nn_feature_matcher.cpp:92 — `return false`
    }
    if (!match_index || !status || (n_matches > 0 && !matches)) {
        return ftk_fail(ctx, FTK_E_INVALID_ARGUMENT, "nn_match_list: null buffer");
    }
    const int rc = run_nn_host(ctx, matches, sizeof(int64_t) * 2 * (size_t)n_matches, n_ref, match_index, status,
                               [&](uint8_t *d_in, int32_t *d_idx, uint8_t *d_st) {
                                   return ftk_nn_match_list_device(ctx, ctx->stream, reinterpret_cast<int64_t *>(d_in), n_matches, n_ref, n_cur, d_idx, d_st);
                               });
    if (rc == FTK_OK && matched_ok) {
        *matched_ok = 1;
    }
    return rc;
}

}  // extern "C"
