/* nn_match_ref.c — scalar CPU restatement of what NNFeatureMatcher::Match does after the network
 * (src/nn_feature_matcher/nn_feature_matcher.cpp:155-216), DESIGN.md 5.11.  TEST INFRASTRUCTURE ONLY: own code that cites the
 * reference by line; nothing under feature_tracker_amd/ may use it.  Plain loops in the reference's order, nothing clever: this file
 * is what the kernels are held to, bit for bit.
 */
#include <stdint.h>

enum { kTracked = 1, kLargeResidual = 2 }; /* feature_tracker.h:10-13 */

/* `a` replaces the running maximum `m`: the reference's strict > (:193, :206).  mutant != 0 turns it into >= — a deliberately wrong
 * variant the tests must tell apart (ties would then go to the LAST index). */
static int beats(float a, float m, int mutant) { return mutant ? a >= m : a > m; }

/* Score mode, one batch item (:177-215).  scores(i, j) = s[i * row_stride + j].  n_ref >= 1, n_cur >= 1.
 * col_best is caller scratch of n_cur entries. */
void nmr_scores(const float *s, int32_t n_ref, int32_t n_cur, int64_t row_stride, float min_score, int32_t *col_best, int32_t *match_index,
                uint8_t *status, int mutant) {
    /* :188-199 — per column: start at row 0, replace on a strict > */
    for (int32_t j = 0; j < n_cur; ++j) {
        int32_t best = 0;
        float max_score = s[j];
        for (int32_t i = 1; i < n_ref; ++i) {
            const float v = s[(int64_t)i * row_stride + j];
            if (beats(v, max_score, mutant)) {
                max_score = v;
                best = i;
            }
        }
        col_best[j] = best;
    }
    /* :156 — every status starts as kLargeResidual; :201-215 — per row */
    for (int32_t i = 0; i < n_ref; ++i) {
        const float *row = s + (int64_t)i * row_stride;
        int32_t best = 0;
        float max_score = row[0];
        match_index[i] = -1;
        status[i] = kLargeResidual;
        for (int32_t j = 1; j < n_cur; ++j) {
            if (beats(row[j], max_score, mutant)) {
                max_score = row[j];
                best = j;
            }
        }
        if (max_score < min_score) { /* :211 — a NaN on either side does not skip */
            continue;
        }
        if (col_best[best] != i) { /* :212 */
            continue;
        }
        match_index[i] = best;
        status[i] = kTracked; /* :214 */
    }
}

/* List mode (:158-174): rows in order, a later applied row overrides an earlier one.  A row is applied iff
 * 0 <= idx_ref < min(n_ref, n_cur) and 0 <= idx_cur < n_cur: :169 bounds idx_ref by the size of matched_pixel_uv_cur (n_cur entries)
 * and :172 writes status[idx_ref] (n_ref entries) — the intersection is where the reference is defined. */
void nmr_list(const int64_t *matches, int32_t n_matches, int32_t n_ref, int32_t n_cur, int32_t *match_index, uint8_t *status) {
    const int64_t ref_bound = n_ref < n_cur ? n_ref : n_cur;
    for (int32_t i = 0; i < n_ref; ++i) {
        match_index[i] = -1;
        status[i] = kLargeResidual;
    }
    for (int32_t k = 0; k < n_matches; ++k) {
        const int64_t idx_ref = matches[2 * (int64_t)k], idx_cur = matches[2 * (int64_t)k + 1];
        if (idx_ref >= 0 && idx_ref < ref_bound && idx_cur >= 0 && idx_cur < n_cur) {
            match_index[idx_ref] = (int32_t)idx_cur;
            status[idx_ref] = kTracked;
        }
    }
}

/* Pixel fill (:157, :171, :213): matched_uv starts as a copy of cur_uv — n_cur entries — and entry idx_ref of a matched row becomes
 * cur_uv[match_index[idx_ref]].  A matched row with idx_ref >= n_cur has no entry (the reference's unchecked write at :213 is
 * undefined there): it is skipped. */
void nmr_fill(const int32_t *match_index, int32_t n_ref, const float *cur_uv, int32_t n_cur, float *matched_uv) {
    for (int32_t t = 0; t < 2 * n_cur; ++t) {
        matched_uv[t] = cur_uv[t];
    }
    for (int32_t i = 0; i < n_ref && i < n_cur; ++i) {
        const int32_t j = match_index[i];
        if (j >= 0 && j < n_cur) {
            matched_uv[2 * i] = cur_uv[2 * j];
            matched_uv[2 * i + 1] = cur_uv[2 * j + 1];
        }
    }
}
