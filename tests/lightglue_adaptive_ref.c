/* lightglue_adaptive_ref.c — the scalar CPU restatement of LightGlue's adaptive depth and width.
 *
 * TEST INFRASTRUCTURE ONLY.  It composes tests/transformer_ref.c's layer and exp_c and tests/match_assignment_ref.c's head, which the
 * binding (tests/lightglue_adaptive_ref.py) hands in as function pointers: no line of them is copied here.
 *
 * The contract.  All arithmetic is float32 with -ffp-contract=off.  L layers; n0, n1 the clamped input counts, P = n0 + n1.  The live
 * counts c0, c1 start at n0, n1 and the index maps at ind[j] = j.  For layer i = 0 .. L - 1:
 *   1. if not stopped, layer i runs in place on the live descriptors with counts c0, c1 (5.24's arithmetic);
 *   2. for i < L - 1 and not stopped, for every live row of both sets: conf = sigmoid_c(z), z the fmaf chain over the columns ascending
 *      from token_confidence.{i}.token.0.bias with its weight; mt likewise with log_assignment.{i}.matchability; sigmoid_c(v) is
 *      1 / (1 + e) for v >= 0 and e / (1 + e) otherwise, e = exp_c(-|v|);
 *   3. only with depth_confidence > 0: u = the number of live rows of both sets with conf < t_i; stop iff P > 0 and
 *      1.0f - (float)u / (float)P > (float)depth_confidence; on a stop stop_layer = i and nothing later changes descriptors, counts or
 *      maps;
 *   4. only with width_confidence > 0 and no stop at this layer, per set whose live count exceeds min_keypoints: a live row is kept iff
 *      mt > (float)(1 - width_confidence) or (with depth_confidence > 0) conf <= t_i; kept rows move to the front in their order with
 *      their encoding rows and ind; the count becomes the number kept; a row that leaves took part in i + 1 layers;
 *   5. stop_layer = L - 1 if the pass never stopped; the head is log_assignment.{stop_layer} on the compacted sets with the live
 *      counts; match_index[ind0[r]] = ind1[m[r]] for a matched live row r, -1 and the unmatched status (2) for every other original
 *      row; layers = stop_layer + 1 for the rows that stayed, 0 behind the input count.
 * Rows at or behind the live count are unspecified in every buffer.
 *
 * `variant` 0 is the contract; the others are mutants the CPU tests must tell apart:
 *   1 the stop ratio divided by the live count instead of P      4 the head of layer L - 1 after an early stop
 *   2 conf < t where the keep rule says <=                        5 an unstable compaction (the kept rows in reverse order)
 *   3 pruning at the stopping layer                               6 indices left in compacted space
 */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

typedef float (*exp_fn)(float);
typedef int (*layer_fn)(const float *, int32_t, const float *, int32_t, int32_t, int32_t, const float *, const float *, const float *, const int32_t *,
                        const int32_t *, int32_t, float *, float *);
typedef int (*assign_fn)(const float *, int32_t, const float *, int32_t, int32_t, const float *, const float *, float, const int32_t *, const int32_t *,
                         int32_t, float *, int64_t);

static int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

static float sigmoid_c(exp_fn exp_c, float v) {
    const float e = exp_c(-fabsf(v));
    const float d = 1.0f + e;
    return v >= 0.0f ? 1.0f / d : e / d;
}

float lga_sigmoid_c(exp_fn exp_c, float v) { return sigmoid_c(exp_c, v); }

/* step 2 for `rows` rows of x [rows][D] */
void lga_confidence(exp_fn exp_c, const float *x, int32_t rows, int32_t D, const float *w, float bias, float *out) {
    for (int r = 0; r < rows; ++r) {
        float z = bias;
        for (int c = 0; c < D; ++c) {
            z = fmaf(x[(size_t)r * D + c], w[c], z);
        }
        out[r] = sigmoid_c(exp_c, z);
    }
}

/* moves the kept rows of one set to the front: desc [rows][D], enc [2][rows][dh], ind [rows]; returns the number kept */
static int compact(const uint8_t *keep, int live, int rows, int D, int dh, int reverse, float *desc, float *enc, int32_t *ind) {
    int32_t *src = (int32_t *)malloc(sizeof(int32_t) * (size_t)(live + 1));
    int kept = 0;
    for (int r = 0; r < live; ++r) {
        if (keep[r]) {
            src[kept++] = r;
        }
    }
    if (reverse) {
        for (int a = 0, b = kept - 1; a < b; ++a, --b) {
            const int32_t t = src[a];
            src[a] = src[b];
            src[b] = t;
        }
    }
    float *d2 = (float *)malloc(sizeof(float) * (size_t)rows * D), *e2 = (float *)malloc(sizeof(float) * 2 * (size_t)rows * dh);
    int32_t *i2 = (int32_t *)malloc(sizeof(int32_t) * (size_t)rows);
    memcpy(d2, desc, sizeof(float) * (size_t)rows * D);
    memcpy(e2, enc, sizeof(float) * 2 * (size_t)rows * dh);
    memcpy(i2, ind, sizeof(int32_t) * (size_t)rows);
    for (int j = 0; j < kept; ++j) {
        memcpy(desc + (size_t)j * D, d2 + (size_t)src[j] * D, sizeof(float) * (size_t)D);
        for (int pl = 0; pl < 2; ++pl) {
            memcpy(enc + ((size_t)pl * rows + j) * dh, e2 + ((size_t)pl * rows + src[j]) * dh, sizeof(float) * (size_t)dh);
        }
        ind[j] = i2[src[j]];
    }
    free(src), free(d2), free(e2), free(i2);
    return kept;
}

/* The pass up to the scores.  desc0 [M][D], desc1 [N][D], enc0 [2][M][dh], enc1 [2][N][dh] are worked on in place (pass copies).
 * layer_w: [L][layer_floats] as tr_layer reads a layer; token_w [L][D], token_b [L]; head_w [L][D + 1][D], head_b [L][D + 1] packed as
 * mar_assign reads them; thresholds [L].  state: live0, live1, stopped, stop_layer.  trace_conf / trace_mt: [L][M + N], written for the
 * live rows of the layers whose step 2 ran (the caller presets them).  scores: [M + 1][N + 1]. */
int lga_pass(exp_fn exp_c, layer_fn layer, assign_fn assign, float *desc0, int32_t M, float *desc1, int32_t N, int32_t D, int32_t h, float *enc0,
             float *enc1, int32_t L, const float *layer_w, int64_t layer_floats, const float *token_w, const float *token_b, const float *head_w,
             const float *head_b, const float *thresholds, float depth, float width, int32_t min_keypoints, const int32_t *count0, const int32_t *count1,
             int32_t variant, int32_t *ind0, int32_t *ind1, int32_t *state, int32_t *layers0, int32_t *layers1, float *trace_conf, float *trace_mt,
             float *scores) {
    const int dh = D / h, n0 = count0 ? clampi(count0[0], 0, M) : M, n1 = count1 ? clampi(count1[0], 0, N) : N, P = n0 + n1;
    const int depth_on = depth > 0.0f, width_on = width > 0.0f;
    const float keep_above = (float)(1.0 - (double)width);
    int32_t c[2] = {n0, n1};
    int stopped = 0, stop_layer = L - 1;
    float *desc[2] = {desc0, desc1}, *enc[2] = {enc0, enc1};
    int32_t *ind[2] = {ind0, ind1}, *layers[2] = {layers0, layers1};
    const int rows[2] = {M, N};
    for (int s = 0; s < 2; ++s) {
        for (int j = 0; j < rows[s]; ++j) {
            ind[s][j] = j;
            layers[s][j] = 0;
        }
    }
    float *out0 = (float *)malloc(sizeof(float) * (size_t)M * D), *out1 = (float *)malloc(sizeof(float) * (size_t)N * D);
    float *conf = (float *)malloc(sizeof(float) * (size_t)(M + N)), *mt = (float *)malloc(sizeof(float) * (size_t)(M + N));
    uint8_t *keep = (uint8_t *)malloc((size_t)(M + N));
    int rc = 0;
    for (int i = 0; i < L && !stopped && rc == 0; ++i) {
        rc = layer(desc0, M, desc1, N, D, h, enc0, enc1, layer_w + (size_t)i * layer_floats, &c[0], &c[1], 0, out0, out1);
        memcpy(desc0, out0, sizeof(float) * (size_t)c[0] * D);
        memcpy(desc1, out1, sizeof(float) * (size_t)c[1] * D);
        if (i == L - 1 || rc != 0) {
            break;
        }
        int u = 0;
        for (int s = 0; s < 2; ++s) {
            const int base = s ? M : 0;
            lga_confidence(exp_c, desc[s], c[s], D, token_w + (size_t)i * D, token_b[i], conf + base);
            lga_confidence(exp_c, desc[s], c[s], D, head_w + ((size_t)i * (D + 1) + D) * D, head_b[(size_t)i * (D + 1) + D], mt + base);
            memcpy(trace_conf + (size_t)i * (M + N) + base, conf + base, sizeof(float) * (size_t)c[s]);
            memcpy(trace_mt + (size_t)i * (M + N) + base, mt + base, sizeof(float) * (size_t)c[s]);
            for (int r = 0; r < c[s]; ++r) {
                u += conf[base + r] < thresholds[i] ? 1 : 0;
            }
        }
        int stop = 0;
        if (depth_on) {
            const int over = variant == 1 ? c[0] + c[1] : P;
            stop = over > 0 && 1.0f - (float)u / (float)over > depth;
        }
        if (stop) {
            stopped = 1;
            stop_layer = i;
        }
        if (width_on && (!stop || variant == 3)) {
            for (int s = 0; s < 2; ++s) {
                if (c[s] <= min_keypoints) {
                    continue;
                }
                const int base = s ? M : 0;
                for (int r = 0; r < c[s]; ++r) {
                    const int unsure = variant == 2 ? conf[base + r] < thresholds[i] : conf[base + r] <= thresholds[i];
                    keep[r] = mt[base + r] > keep_above || (depth_on && unsure);
                    if (!keep[r]) {
                        layers[s][ind[s][r]] = i + 1;
                    }
                }
                c[s] = compact(keep, c[s], rows[s], D, dh, variant == 5, desc[s], enc[s], ind[s]);
            }
        }
    }
    if (rc == 0) {
        const int head = variant == 4 ? L - 1 : stop_layer;
        rc = assign(desc0, M, desc1, N, D, head_w + (size_t)head * (D + 1) * D, head_b + (size_t)head * (D + 1), 1.0f, &c[0], &c[1], 0, scores, N + 1);
    }
    for (int s = 0; s < 2; ++s) {
        for (int r = 0; r < c[s]; ++r) {
            layers[s][ind[s][r]] = stop_layer + 1;
        }
    }
    state[0] = c[0], state[1] = c[1], state[2] = stopped, state[3] = stop_layer;
    free(out0), free(out1), free(conf), free(mt), free(keep);
    return rc;
}

/* step 5's map back: m [M] and st [M] are the matcher's result on the compacted scores */
void lga_remap(const int32_t *m, const uint8_t *st, int32_t M, int32_t live0, int32_t live1, const int32_t *ind0, const int32_t *ind1, int32_t variant,
               int32_t *match_index, uint8_t *status) {
    for (int j = 0; j < M; ++j) {
        match_index[j] = -1;
        status[j] = 2;
    }
    for (int r = 0; r < live0; ++r) {
        const int beyond = m[r] >= live1;
        const int o = variant == 6 ? r : ind0[r];
        match_index[o] = m[r] >= 0 && !beyond ? (variant == 6 ? m[r] : ind1[m[r]]) : -1;
        status[o] = beyond ? 2 : st[r];
    }
}
