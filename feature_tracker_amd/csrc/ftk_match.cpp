// ftk_match.cpp — the descriptor matchers of the C ABI (include/ftk.h): Hamming (BRIEF) and cosine (SuperPoint / DISK) distance,
// device-resident and host-buffer forms, and the host-side index -> pixel fill.
#include <string.h>

#include "ftk_internal.h"
#include "match_plan.h"

namespace {

int env_int(const char *v) { return v ? atoi(v) : ftk::kPlanNotSet; }  // an FTK_* switch as a plan input

int ensure_match_boxes(ftk_context *ctx, size_t count) {
    FTK_HIP(ctx, ctx->match_boxes.reserve(ctx->stream, sizeof(float) * 4 * count, 0, 1));
    return FTK_OK;
}

// Zero-pads the n_words-wide descriptors to `dev_words` words in a context-owned copy (equal pad bits in both sets: same distances).
int pad_descriptors(ftk_context *ctx, const uint32_t **ref, int32_t n_ref, const uint32_t **cur, int32_t n_cur, int32_t n_words, int32_t dev_words) {
    ftk_layout L;
    const auto s_ref = L.take<uint32_t>((size_t)n_ref * dev_words), s_cur = L.take<uint32_t>((size_t)n_cur * dev_words);
    const int rc = ftk_ensure_device_buffer(ctx, ctx->match_pad, L);
    if (rc != FTK_OK) {
        return rc;
    }
    uint32_t *pad_ref = s_ref.in(ctx->match_pad.get()), *pad_cur = s_cur.in(ctx->match_pad.get());
    FTK_HIP(ctx, hipMemsetAsync(pad_ref, 0, L.bytes(), ctx->stream));
    FTK_HIP(ctx, hipMemcpy2DAsync(pad_ref, sizeof(uint32_t) * dev_words, *ref, sizeof(uint32_t) * n_words, sizeof(uint32_t) * n_words, (size_t)n_ref,
                                  hipMemcpyDeviceToDevice, ctx->stream));
    FTK_HIP(ctx, hipMemcpy2DAsync(pad_cur, sizeof(uint32_t) * dev_words, *cur, sizeof(uint32_t) * n_words, sizeof(uint32_t) * n_words, (size_t)n_cur,
                                  hipMemcpyDeviceToDevice, ctx->stream));
    *ref = pad_ref;
    *cur = pad_cur;
    return FTK_OK;
}

// The host-buffer matchers: [ref | cur | pred | cur_uv | index] gathered in the context's pinned block, laid out like the device
// scratch, and sent with ONE H2D (pageable hipMemcpyAsync calls are staged one by one by the runtime, ~10 us each; the reference's
// callers time these calls); `run` launches the device entry on the scratch copies, then the indices come back.  Descriptor rows of
// `row_bytes` are zero-padded to `dev_row_bytes` (pad bits equal in both sets: distance unchanged).
template <class Run>
int run_staged_match(ftk_context *ctx, const void *ref, int32_t n_ref, const void *cur, int32_t n_cur, size_t row_bytes, size_t dev_row_bytes,
                     const float *pred_uv, const float *cur_uv, int32_t *index_pairs, Run run) {
    FTK_HIP(ctx, hipSetDevice(ctx->device));
    ftk_layout L;
    const auto s_ref = L.take<uint8_t>(dev_row_bytes * (size_t)n_ref), s_cur = L.take<uint8_t>(dev_row_bytes * (size_t)n_cur);
    const auto s_pred = L.take<float>(pred_uv ? 2 * (size_t)n_ref : 0), s_cuv = L.take<float>(pred_uv ? 2 * (size_t)n_cur : 0);  // (nothing without pred_uv)
    const auto s_idx = L.take<int32_t>((size_t)n_ref);
    uint8_t *base = nullptr, *hbase = nullptr;
    int rc = ftk_ensure_mirror(ctx, L, &base, &hbase);
    if (rc != FTK_OK) {
        return rc;
    }
    if (dev_row_bytes == row_bytes) {
        memcpy(s_ref.in(hbase), ref, s_ref.size_bytes());
        memcpy(s_cur.in(hbase), cur, s_cur.size_bytes());
    } else {
        memset(s_ref.in(hbase), 0, L.span_bytes(s_ref, s_cur));
        for (int32_t i = 0; i < n_ref; ++i) {
            memcpy(s_ref.in(hbase) + dev_row_bytes * (size_t)i, static_cast<const uint8_t *>(ref) + row_bytes * (size_t)i, row_bytes);
        }
        for (int32_t i = 0; i < n_cur; ++i) {
            memcpy(s_cur.in(hbase) + dev_row_bytes * (size_t)i, static_cast<const uint8_t *>(cur) + row_bytes * (size_t)i, row_bytes);
        }
    }
    if (pred_uv) {
        memcpy(s_pred.in(hbase), pred_uv, s_pred.size_bytes());
        memcpy(s_cuv.in(hbase), cur_uv, s_cuv.size_bytes());
    }
    memcpy(s_idx.in(hbase), index_pairs, s_idx.size_bytes());
    FTK_HIP(ctx, hipMemcpyAsync(base, hbase, L.bytes(), hipMemcpyHostToDevice, ctx->stream));
    rc = run(s_ref.in(base), s_cur.in(base), pred_uv ? s_pred.in(base) : nullptr, pred_uv ? s_cuv.in(base) : nullptr, s_idx.in(base));
    if (rc != FTK_OK) {
        (void)hipStreamSynchronize(ctx->stream);
        return rc;
    }
    FTK_HIP(ctx, hipMemcpyAsync(s_idx.in(hbase), s_idx.in(base), s_idx.size_bytes(), hipMemcpyDeviceToHost, ctx->stream));
    FTK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    memcpy(index_pairs, s_idx.in(hbase), s_idx.size_bytes());
    return FTK_OK;
}

}  // namespace

// The Hamming matcher's keys, `count` of them, all ones.
int ftk_ensure_match_keys(ftk_context *ctx, size_t count) {
    bool grew = false;
    FTK_HIP(ctx, ctx->match_keys.reserve(ctx->stream, sizeof(unsigned long long) * count, 0, 1, &grew));
    if (grew) {  // all-ones = "no match yet"; the epilogue kernel restores this state after every call
        FTK_HIP(ctx, hipMemsetAsync(ctx->match_keys.get(), 0xFF, ctx->match_keys.bytes(), ctx->stream));
    }
    return FTK_OK;
}

extern "C" {

int ftk_hamming_match_device(ftk_context *ctx, const uint32_t *d_ref_words, int32_t n_ref, const uint32_t *d_cur_words, int32_t n_cur,
                             int32_t n_words, int32_t n_bits, float max_distance, const float *d_pred_uv, const float *d_cur_uv,
                             int32_t max_col_distance, int32_t max_row_distance, int32_t *d_index_pairs, uint64_t *d_workspace) {
    if (!ctx) {
        return ftk_fail(nullptr, FTK_E_INVALID_ARGUMENT, "hamming_match_device: null context");
    }
    FTK_LOCK(ctx);
    if (n_ref < 0 || n_cur < 0 || n_bits < 0) {
        return ftk_fail(ctx, FTK_E_INVALID_ARGUMENT, "hamming_match_device: negative size");
    }
    if (n_ref == 0 || n_cur == 0) {
        return FTK_OK;
    }
    if (n_words < 1) {
        return ftk_fail(ctx, FTK_E_INVALID_ARGUMENT, "hamming_match_device: n_words %d < 1", n_words);
    }
    if (n_bits > 32 * n_words) {
        return ftk_fail(ctx, FTK_E_INVALID_ARGUMENT, "hamming_match_device: n_bits %d exceeds %d words", n_bits, n_words);
    }
    if (!d_ref_words || !d_cur_words || !d_index_pairs || (d_pred_uv && !d_cur_uv)) {
        return ftk_fail(ctx, FTK_E_INVALID_ARGUMENT, "hamming_match_device: null buffer");
    }
    FTK_HIP(ctx, hipSetDevice(ctx->device));
    const char *kernel = FTK_ENV(ctx, match_kernel);
    const ftk::HammingPlan plan = ftk::hamming_plan({n_ref, n_cur, n_words, n_bits, d_pred_uv != nullptr, d_workspace != nullptr, env_int(FTK_ENV(ctx, match_small)),
                                                     kernel ? (strcmp(kernel, "mfma") == 0 ? 1 : 0) : ftk::kPlanNotSet});
    int rc = plan.dev_words != n_words ? pad_descriptors(ctx, &d_ref_words, n_ref, &d_cur_words, n_cur, n_words, plan.dev_words) : FTK_OK;
    rc = rc == FTK_OK && plan.keys_clean ? ftk_ensure_match_keys(ctx, (size_t)n_ref) : rc;  // (the context's keys hold "no match")
    rc = rc == FTK_OK && plan.n_boxes > 0 ? ensure_match_boxes(ctx, plan.n_boxes) : rc;
    if (rc != FTK_OK) {
        return rc;
    }
    unsigned long long *keys = plan.keys_clean ? ctx->match_keys.as<unsigned long long>() : reinterpret_cast<unsigned long long *>(d_workspace);
    const ftk::MatchParams p = {d_ref_words, d_cur_words, d_pred_uv, d_cur_uv, d_index_pairs, keys, n_ref, n_cur, plan.dev_words, n_bits, max_distance,
                                (float)max_col_distance, (float)max_row_distance, plan.cur_per_block, plan.keys_clean, plan.matrix_cores,
                                plan.n_boxes > 0 ? ctx->match_boxes.as<float4>() : nullptr};
    FTK_HIP(ctx, ftk::match_launch(plan, p, ctx->stream));
    return FTK_OK;
}

int ftk_hamming_match(ftk_context *ctx, const uint32_t *ref_words, int32_t n_ref, const uint32_t *cur_words, int32_t n_cur, int32_t n_words,
                      int32_t n_bits, float max_distance, const float *pred_uv, const float *cur_uv, int32_t max_col_distance,
                      int32_t max_row_distance, int32_t *index_pairs, int *matched_ok) {
    FTK_TRACE_SCOPE("ftk_hamming_match");
    if (!ctx) {
        return ftk_fail(nullptr, FTK_E_INVALID_ARGUMENT, "hamming_match: null context");
    }
    FTK_LOCK(ctx);
    if (matched_ok) {
        *matched_ok = 0;
    }
    if (n_ref < 0 || n_cur < 0 || n_words < 1 || n_bits < 0 || n_bits > 32 * n_words) {
        return ftk_fail(ctx, FTK_E_INVALID_ARGUMENT, "hamming_match: bad sizes (n_ref %d, n_cur %d, n_words %d, n_bits %d)", n_ref, n_cur, n_words, n_bits);
    }
    if (n_cur == 0) {
        return FTK_OK;  // descriptor_matcher.h:58 — `return false`
    }
    if (matched_ok) {
        *matched_ok = 1;
    }
    if (n_ref == 0) {
        return FTK_OK;
    }
    if (!ref_words || !cur_words || !index_pairs || (pred_uv && !cur_uv)) {
        return ftk_fail(ctx, FTK_E_INVALID_ARGUMENT, "hamming_match: null buffer");
    }
    const int32_t dev_words = ftk::hamming_device_words(n_words);  // padded on the host, during the gather
    return run_staged_match(ctx, ref_words, n_ref, cur_words, n_cur, sizeof(uint32_t) * n_words, sizeof(uint32_t) * dev_words, pred_uv, cur_uv, index_pairs,
                            [&](uint8_t *d_ref, uint8_t *d_cur, float *d_pred, float *d_cuv, int32_t *d_idx) {
                                return ftk_hamming_match_device(ctx, reinterpret_cast<uint32_t *>(d_ref), n_ref, reinterpret_cast<uint32_t *>(d_cur), n_cur,
                                                                dev_words, n_bits, max_distance, d_pred, d_cuv, max_col_distance, max_row_distance, d_idx, nullptr);
                            });
}

int ftk_cosine_match_device(ftk_context *ctx, const float *d_ref_desc, int32_t n_ref, const float *d_cur_desc, int32_t n_cur, int32_t dim,
                            float max_distance, const float *d_pred_uv, const float *d_cur_uv, int32_t max_col_distance,
                            int32_t max_row_distance, int32_t *d_index_pairs) {
    if (!ctx) {
        return ftk_fail(nullptr, FTK_E_INVALID_ARGUMENT, "cosine_match_device: null context");
    }
    FTK_LOCK(ctx);
    if (n_ref < 0 || n_cur < 0 || dim < 1) {
        return ftk_fail(ctx, FTK_E_INVALID_ARGUMENT, "cosine_match_device: bad sizes (n_ref %d, n_cur %d, dim %d)", n_ref, n_cur, dim);
    }
    if (dim > 4096) {
        return ftk_fail(ctx, FTK_E_UNSUPPORTED, "cosine_match_device: dim %d > 4096", dim);
    }
    if (n_ref == 0 || n_cur == 0) {
        return FTK_OK;
    }
    if (!d_ref_desc || !d_cur_desc || !d_index_pairs || (d_pred_uv && !d_cur_uv)) {
        return ftk_fail(ctx, FTK_E_INVALID_ARGUMENT, "cosine_match_device: null buffer");
    }
    FTK_HIP(ctx, hipSetDevice(ctx->device));
    const ftk::CosinePlanInput in = {n_ref, n_cur, dim, d_pred_uv != nullptr, ((reinterpret_cast<uintptr_t>(d_ref_desc) | reinterpret_cast<uintptr_t>(d_cur_desc)) & 15u) == 0,
                                     env_int(FTK_ENV(ctx, cosine_small)), env_int(FTK_ENV(ctx, cosine_chunked)), env_int(FTK_ENV(ctx, cosine_splits))};
    const ftk::CosinePlan plan = ftk::cosine_plan(in);
    const int rc = ftk_ensure_device_buffer(ctx, ctx->cosine_ws, plan.ws_bytes);
    if (rc != FTK_OK) {
        return rc;
    }
    uint8_t *ws = ctx->cosine_ws.as<uint8_t>();
    auto at = [ws](size_t offset) -> void * { return ws + offset; };
    const ftk::CosineParams p = {d_ref_desc, d_cur_desc, d_pred_uv, d_cur_uv, d_index_pairs, (_Float16 *)at(plan.ref_h), (_Float16 *)at(plan.cur_h),
                                 (float *)at(plan.ref_norm), (float *)at(plan.cur_norm), (float *)at(plan.cur_bias), (float4 *)at(plan.cur_info),
                                 plan.use_tile_box ? (float4 *)at(plan.tile_box) : nullptr, ws + plan.ref_irregular, (uint32_t *)at(plan.row_max),
                                 (uint32_t *)at(plan.cand_count), (int32_t *)at(plan.cand), plan.ref_stationary ? (float *)at(plan.cand_score) : nullptr,
                                 (uint32_t *)at(plan.irregular_count), (int32_t *)at(plan.irregular_list), at(plan.row_max), plan.clear_end - plan.row_max,
                                 n_ref, n_cur, dim, plan.n_ref_pad, plan.n_cur_pad, plan.dim_pad, plan.tiles_per_split, plan.ref_stationary, plan.splits,
                                 max_distance, (float)max_col_distance, (float)max_row_distance, plan.margin};
    FTK_HIP(ctx, ftk::cosine_match_launch(plan, p, ctx->stream));
    return FTK_OK;
}

int ftk_cosine_match(ftk_context *ctx, const float *ref_desc, int32_t n_ref, const float *cur_desc, int32_t n_cur, int32_t dim, float max_distance,
                     const float *pred_uv, const float *cur_uv, int32_t max_col_distance, int32_t max_row_distance, int32_t *index_pairs,
                     int *matched_ok) {
    FTK_TRACE_SCOPE("ftk_cosine_match");
    if (!ctx) {
        return ftk_fail(nullptr, FTK_E_INVALID_ARGUMENT, "cosine_match: null context");
    }
    FTK_LOCK(ctx);
    if (matched_ok) {
        *matched_ok = 0;
    }
    if (n_ref < 0 || n_cur < 0 || dim < 1) {
        return ftk_fail(ctx, FTK_E_INVALID_ARGUMENT, "cosine_match: bad sizes (n_ref %d, n_cur %d, dim %d)", n_ref, n_cur, dim);
    }
    if (n_cur == 0) {
        return FTK_OK;  // descriptor_matcher.h:58,94 — `return false`
    }
    if (matched_ok) {
        *matched_ok = 1;
    }
    if (n_ref == 0) {
        return FTK_OK;
    }
    if (!ref_desc || !cur_desc || !index_pairs || (pred_uv && !cur_uv)) {
        return ftk_fail(ctx, FTK_E_INVALID_ARGUMENT, "cosine_match: null buffer");
    }
    return run_staged_match(ctx, ref_desc, n_ref, cur_desc, n_cur, sizeof(float) * dim, sizeof(float) * dim, pred_uv, cur_uv, index_pairs,
                            [&](uint8_t *d_ref, uint8_t *d_cur, float *d_pred, float *d_cuv, int32_t *d_idx) {
                                return ftk_cosine_match_device(ctx, reinterpret_cast<float *>(d_ref), n_ref, reinterpret_cast<float *>(d_cur), n_cur, dim,
                                                               max_distance, d_pred, d_cuv, max_col_distance, max_row_distance, d_idx);
                            });
}

int ftk_fill_matched_pixels(const int32_t *index_pairs, int32_t n_ref, const float *cur_uv, int32_t n_cur, float *matched_uv, uint8_t *status) {
    if (n_ref < 0 || n_cur < 0 || (n_ref > 0 && (!index_pairs || !matched_uv || !status)) || (n_cur > 0 && !cur_uv)) {
        return FTK_E_INVALID_ARGUMENT;
    }
    for (int32_t i = 0; i < n_ref; ++i) {
        if (status[i] > FTK_TRACKED) {
            continue;
        }
        const int32_t j = index_pairs[i];
        if (j >= 0 && j < n_cur) {
            matched_uv[2 * i] = cur_uv[2 * j];
            matched_uv[2 * i + 1] = cur_uv[2 * j + 1];
            status[i] = FTK_TRACKED;
        } else {
            status[i] = FTK_LARGE_RESIDUAL;
        }
    }
    return FTK_OK;
}

}  // extern "C"
