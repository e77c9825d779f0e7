/* transformer_ref.c — scalar CPU restatement of LightGlue's transformer layer, one float operation per line of the
 * contract.  TEST INFRASTRUCTURE ONLY: compiled by tests/transformer_ref.py with -ffp-contract=off; nothing under feature_tracker_amd/
 * uses it.  The weights arrive in UPSTREAM's layout (Wqkv's rows as (head, channel, q | k | v)), not in the library's packing.
 * `variant` 0 is the contract; 1 .. 6 are the mutants of tests/test_transformer_cpu.py. */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

enum { CONTRACT = 0, ROTARY_HALVES = 1, QKV_AS_3_H_DH = 2, REVERSE_SOFTMAX_WRONG_AXIS = 3, INVALID_KEYS_IN_SOFTMAX = 4, CAT_MSG_FIRST = 5, UNBIASED_VARIANCE = 6 };

static float from_bits(uint32_t u) {
    float f;
    memcpy(&f, &u, 4);
    return f;
}

/* exp_c of DESIGN.md 5.12, t <= 0 or NaN */
float tr_exp_c(float t) {
    if (t != t) {
        return t;
    }
    if (t < -87.0f) {
        return 0.0f;
    }
    const float n = rintf(t * 0x1.715476p+0f);
    float r = fmaf(n, -0x1.62e4p-1f, t);
    r = fmaf(n, -0x1.7f7d1cp-20f, r);
    float p = 0x1.a01a02p-13f;
    p = fmaf(p, r, 0x1.6c16c2p-10f);
    p = fmaf(p, r, 0x1.111112p-7f);
    p = fmaf(p, r, 0x1.555556p-5f);
    p = fmaf(p, r, 0x1.555556p-3f);
    p = fmaf(p, r, 0x1p-1f);
    p = fmaf(p, r, 1.0f);
    p = fmaf(p, r, 1.0f);
    return p * from_bits((uint32_t)((int)n + 127) << 23);
}

/* erf_c of DESIGN.md 5.24 */
float tr_erf_c(float x) {
    if (x != x) {
        return x;
    }
    const float a = fabsf(x);
    if (a < 1.0f) {
        static const float T[13] = {0x1.20dd76p+0f, -0x1.812746p-2f, 0x1.ce2f22p-4f, -0x1.b82ce4p-6f, 0x1.565bcep-8f, -0x1.c02db4p-11f, 0x1.f9a326p-14f,
                                    -0x1.f4d25cp-17f, 0x1.b9e6cap-20f, -0x1.5f742ep-23f, 0x1.fcc572p-27f, -0x1.51d718p-30f, 0x1.9e6ad6p-34f};
        const float s = x * x;
        float p = T[12];
        for (int k = 11; k >= 0; --k) {
            p = fmaf(p, s, T[k]);
        }
        return x * p;
    }
    if (a >= 4.0f) {
        return copysignf(1.0f, x);
    }
    static const float Q[10] = {0x1.11b274p-13f, 0x1.1f8b32p-1f, 0x1.634f56p-6f, -0x1.85acaap-2f, 0x1.effe7ap-3f, 0x1.c0ff9ap-3f, -0x1.08bcdap-1f,
                                0x1.b39f5p-2f, -0x1.6687c8p-3f, 0x1.eb6cf6p-6f};
    const float t = 1.0f / a;
    float q = Q[9];
    for (int k = 8; k >= 0; --k) {
        q = fmaf(q, t, Q[k]);
    }
    const float e = tr_exp_c(-(a * a));
    return copysignf(1.0f - e * q, x);
}

/* 5.23 step 3's partial sums and xor tree over n values from +0 */
static float tree_sum(const float *x, int n) {
    float p[64];
    for (int l = 0; l < 64; ++l) {
        p[l] = 0.0f;
    }
    for (int k = 0; k < n; ++k) {
        p[k & 63] = p[k & 63] + x[k];
    }
    for (int off = 32; off >= 1; off >>= 1) {
        float q[64];
        for (int l = 0; l < 64; ++l) {
            q[l] = p[l] + p[l ^ off];
        }
        memcpy(p, q, sizeof(p));
    }
    return p[0];
}

static int clamp(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

/* out [rows][outs] = [x | xb] w^T + bias (+ res); xb NULL: one segment */
void tr_linear(const float *x, const float *xb, int32_t rows, int32_t ka, int32_t kb, const float *w, const float *bias, int32_t outs, const float *res,
               float *out) {
    const size_t K = (size_t)ka + (size_t)(xb ? kb : 0);
    for (int i = 0; i < rows; ++i) {
        for (int o = 0; o < outs; ++o) {
            float acc = bias[o];
            for (int c = 0; c < ka; ++c) {
                acc = fmaf(x[(size_t)i * ka + c], w[(size_t)o * K + c], acc);
            }
            for (int c = 0; xb && c < kb; ++c) {
                acc = fmaf(xb[(size_t)i * kb + c], w[(size_t)o * K + ka + c], acc);
            }
            out[(size_t)i * outs + o] = res ? res[(size_t)i * outs + o] + acc : acc;
        }
    }
}

/* t [rows][D] in place; enc [2][rows][dh] */
void tr_rotary(float *t, int32_t rows, int32_t D, int32_t h, const float *enc, int32_t variant) {
    const int dh = D / h;
    const float *cs = enc, *sn = enc + (size_t)rows * dh;
    for (int i = 0; i < rows; ++i) {
        for (int a = 0; a < h; ++a) {
            float *x = t + (size_t)i * D + (size_t)a * dh;
            const float *c = cs + (size_t)i * dh, *s = sn + (size_t)i * dh;
            for (int e = 0; e < dh / 2; ++e) {
                const int lo = variant == ROTARY_HALVES ? e : 2 * e, hi = variant == ROTARY_HALVES ? e + dh / 2 : 2 * e + 1;
                const float x0 = x[lo], x1 = x[hi];
                x[lo] = x0 * c[lo] + (-x1) * s[lo];
                x[hi] = x1 * c[hi] + x0 * s[hi];
            }
        }
    }
}

/* the probabilities of one query row of one head over the first n keys: p [n] */
static void probabilities(const float *q, const float *k, int32_t D, int32_t dh, int32_t n, float pre, float post, float *p) {
    for (int j = 0; j < n; ++j) {
        float acc = 0.0f;
        for (int e = 0; e < dh; ++e) {
            acc = fmaf(q[e] * pre, k[(size_t)j * D + e] * pre, acc);
        }
        p[j] = acc * post;
    }
    float m = p[0];
    for (int j = 1; j < n; ++j) {
        if (p[j] > m) {
            m = p[j];
        }
    }
    for (int j = 0; j < n; ++j) {
        p[j] = tr_exp_c(p[j] - m);
    }
    const float l = tree_sum(p, n);
    for (int j = 0; j < n; ++j) {
        p[j] = p[j] / l;
    }
}

/* out [Mq][D]; count: one int32 or NULL */
void tr_attention(const float *q, const float *k, const float *v, int32_t Mq, int32_t Nk, int32_t D, int32_t h, const int32_t *count, float pre,
                  float post, float *out) {
    const int dh = D / h, n = count ? clamp(count[0], 0, Nk) : Nk;
    float *p = (float *)malloc(sizeof(float) * (size_t)(Nk + 1));
    for (int a = 0; a < h; ++a) {
        for (int i = 0; i < Mq; ++i) {
            if (n > 0) {
                probabilities(q + (size_t)i * D + (size_t)a * dh, k + (size_t)a * dh, D, dh, n, pre, post, p);
            }
            for (int d = 0; d < dh; ++d) {
                float acc = 0.0f;
                for (int j = 0; j < n; ++j) {
                    acc = fmaf(p[j], v[(size_t)j * D + (size_t)a * dh + d], acc);
                }
                out[(size_t)i * D + (size_t)a * dh + d] = acc;
            }
        }
    }
    free(p);
}

/* the mutant of the cross block's reverse direction: direction 0's probabilities (normalised over the keys of set 1), transposed */
static void attention_wrong_axis(const float *qk0, const float *qk1, const float *v0, int32_t M, int32_t N, int32_t D, int32_t h, int n0, int n1, float pre,
                                 float *out1) {
    const int dh = D / h;
    float *p = (float *)calloc((size_t)M * (size_t)(N + 1), sizeof(float));
    for (int a = 0; a < h; ++a) {
        for (int i = 0; i < M && n1 > 0; ++i) {
            probabilities(qk0 + (size_t)i * D + (size_t)a * dh, qk1 + (size_t)a * dh, D, dh, n1, pre, 1.0f, p + (size_t)i * (N + 1));
        }
        for (int j = 0; j < N; ++j) {
            for (int d = 0; d < dh; ++d) {
                float acc = 0.0f;
                for (int i = 0; i < n0; ++i) {
                    acc = fmaf(j < n1 ? p[(size_t)i * (N + 1) + j] : 0.0f, v0[(size_t)i * D + (size_t)a * dh + d], acc);
                }
                out1[(size_t)j * D + (size_t)a * dh + d] = acc;
            }
        }
    }
    free(p);
}

/* x [rows][n] in place */
void tr_layernorm_gelu(float *x, int32_t rows, int32_t n, const float *gamma, const float *beta, int32_t variant) {
    float *d = (float *)malloc(sizeof(float) * (size_t)n);
    for (int i = 0; i < rows; ++i) {
        float *row = x + (size_t)i * n;
        const float mean = tree_sum(row, n) / (float)n;
        float p[64];
        for (int l = 0; l < 64; ++l) {
            p[l] = 0.0f;
        }
        for (int c = 0; c < n; ++c) {
            d[c] = row[c] - mean;
            p[c & 63] = fmaf(d[c], d[c], p[c & 63]);
        }
        for (int off = 32; off >= 1; off >>= 1) {
            float q[64];
            for (int l = 0; l < 64; ++l) {
                q[l] = p[l] + p[l ^ off];
            }
            memcpy(p, q, sizeof(p));
        }
        const float var = p[0] / (float)(variant == UNBIASED_VARIANCE ? n - 1 : n);
        const float r = 1.0f / sqrtf(var + 1e-5f);
        for (int c = 0; c < n; ++c) {
            const float y = fmaf(d[c] * r, gamma[c], beta[c]);
            row[c] = (0.5f * y) * (1.0f + tr_erf_c(y * 0x1.6a09e6p-1f));
        }
    }
    free(d);
}

/* x + ffn.3(GELU(LN(ffn.0([x | msg])))); w: ffn.0 weight, bias, LayerNorm weight, bias, ffn.3 weight, bias */
static void ffn(const float *x, const float *msg, int32_t rows, int32_t D, const float *w, int32_t variant, float *out) {
    const size_t d = (size_t)D;
    const float *w0 = w, *b0 = w0 + 4 * d * d, *g = b0 + 2 * d, *be = g + 2 * d, *w3 = be + 2 * d, *b3 = w3 + 2 * d * d;
    float *hid = (float *)malloc(sizeof(float) * (size_t)rows * 2 * d);
    if (variant == CAT_MSG_FIRST) {
        tr_linear(msg, x, rows, D, D, w0, b0, 2 * D, NULL, hid);
    } else {
        tr_linear(x, msg, rows, D, D, w0, b0, 2 * D, NULL, hid);
    }
    tr_layernorm_gelu(hid, rows, 2 * D, g, be, variant);
    tr_linear(hid, NULL, rows, 2 * D, 0, w3, b3, D, x, out);
    free(hid);
}

static void self_block(const float *x, int32_t rows, int32_t D, int32_t h, const float *enc, const int32_t *count, const float *w, int32_t variant, float *out) {
    const size_t d = (size_t)D, plane = (size_t)rows * d;
    const int dh = D / h;
    const float *wqkv = w, *bqkv = wqkv + 3 * d * d, *wo = bqkv + 3 * d, *bo = wo + d * d, *rest = bo + d;
    float *raw = (float *)malloc(sizeof(float) * 3 * plane), *qkv = (float *)malloc(sizeof(float) * 3 * plane);
    float *ctx = (float *)malloc(sizeof(float) * plane), *msg = (float *)malloc(sizeof(float) * plane);
    tr_linear(x, NULL, rows, D, 0, wqkv, bqkv, 3 * D, NULL, raw);
    for (int i = 0; i < rows; ++i) {
        for (int a = 0; a < h; ++a) {
            for (int e = 0; e < dh; ++e) {
                for (int t = 0; t < 3; ++t) {
                    const size_t col = variant == QKV_AS_3_H_DH ? (size_t)t * d + (size_t)a * dh + e : ((size_t)a * dh + e) * 3 + t;
                    qkv[t * plane + (size_t)i * d + (size_t)a * dh + e] = raw[(size_t)i * 3 * d + col];
                }
            }
        }
    }
    tr_rotary(qkv, rows, D, h, enc, variant);
    tr_rotary(qkv + plane, rows, D, h, enc, variant);
    const int32_t all = rows;
    tr_attention(qkv, qkv + plane, qkv + 2 * plane, rows, rows, D, h, variant == INVALID_KEYS_IN_SOFTMAX ? &all : count, 1.0f,
                 (float)(1.0 / sqrt((double)dh)), ctx);
    tr_linear(ctx, NULL, rows, D, 0, wo, bo, D, NULL, msg);
    ffn(x, msg, rows, D, rest, variant, out);
    free(raw);
    free(qkv);
    free(ctx);
    free(msg);
}

/* floats of one layer's weights in upstream's layout: self (Wqkv, out_proj, ffn.0, ffn.1, ffn.3), cross (to_qk, to_v, to_out, ffn.0, ffn.1, ffn.3), each
 * weight then bias */
int64_t tr_layer_weight_floats(int32_t D) {
    const int64_t d = D, f = 4 * d * d + 2 * d + 4 * d + 2 * d * d + d;
    return (3 * d * d + 3 * d + d * d + d + f) + (3 * (d * d + d) + f);
}

int tr_layer(const float *desc0, int32_t M, const float *desc1, int32_t N, int32_t D, int32_t h, const float *enc0, const float *enc1, const float *weights,
             const int32_t *count0, const int32_t *count1, int32_t variant, float *out0, float *out1) {
    if (M < 1 || N < 1 || D < 1 || h < 1 || D % h != 0 || (D / h) % 2 != 0) {
        return -1;
    }
    const size_t d = (size_t)D;
    const int dh = D / h;
    const size_t f = 4 * d * d + 2 * d + 4 * d + 2 * d * d + d;
    const float *ws = weights, *wc = weights + (3 * d * d + 3 * d + d * d + d + f);
    const float *wqk = wc, *bqk = wqk + d * d, *wv = bqk + d, *bv = wv + d * d, *wout = bv + d, *bout = wout + d * d, *rest = bout + d;
    float *x0 = (float *)malloc(sizeof(float) * M * d), *x1 = (float *)malloc(sizeof(float) * N * d);
    self_block(desc0, M, D, h, enc0, count0, ws, variant, x0);
    self_block(desc1, N, D, h, enc1, count1, ws, variant, x1);
    float *qk0 = (float *)malloc(sizeof(float) * M * d), *qk1 = (float *)malloc(sizeof(float) * N * d);
    float *v0 = (float *)malloc(sizeof(float) * M * d), *v1 = (float *)malloc(sizeof(float) * N * d);
    float *m0 = (float *)malloc(sizeof(float) * M * d), *m1 = (float *)malloc(sizeof(float) * N * d);
    float *o0 = (float *)malloc(sizeof(float) * M * d), *o1 = (float *)malloc(sizeof(float) * N * d);
    tr_linear(x0, NULL, M, D, 0, wqk, bqk, D, NULL, qk0);
    tr_linear(x1, NULL, N, D, 0, wqk, bqk, D, NULL, qk1);
    tr_linear(x0, NULL, M, D, 0, wv, bv, D, NULL, v0);
    tr_linear(x1, NULL, N, D, 0, wv, bv, D, NULL, v1);
    const float pre = (float)pow((double)dh, -0.25);
    const int32_t all0 = M, all1 = N;
    const int32_t *c0 = variant == INVALID_KEYS_IN_SOFTMAX ? &all0 : count0, *c1 = variant == INVALID_KEYS_IN_SOFTMAX ? &all1 : count1;
    tr_attention(qk0, qk1, v1, M, N, D, h, c1, pre, 1.0f, m0);
    if (variant == REVERSE_SOFTMAX_WRONG_AXIS) {
        attention_wrong_axis(qk0, qk1, v0, M, N, D, h, c0 ? clamp(c0[0], 0, M) : M, c1 ? clamp(c1[0], 0, N) : N, pre, m1);
    } else {
        tr_attention(qk1, qk0, v0, N, M, D, h, c0, pre, 1.0f, m1);
    }
    tr_linear(m0, NULL, M, D, 0, wout, bout, D, NULL, o0);
    tr_linear(m1, NULL, N, D, 0, wout, bout, D, NULL, o1);
    ffn(x0, o0, M, D, rest, variant, out0);
    ffn(x1, o1, N, D, rest, variant, out1);
    float *all[] = {x0, x1, qk0, qk1, v0, v1, m0, m1, o0, o1};
    for (int k = 0; k < 10; ++k) {
        free(all[k]);
    }
    return 0;
}
