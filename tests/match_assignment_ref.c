/* match_assignment_ref.c — scalar CPU restatement of LightGlue's assignment head, steps 1-6, one float operation per
 * line of the contract.  TEST INFRASTRUCTURE ONLY: compiled by tests/match_assignment_ref.py with -ffp-contract=off; nothing under
 * feature_tracker_amd/ uses it.  `variant` 0 is the contract; 1 .. 5 are the mutants of tests/test_match_assignment_cpu.py. */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

enum { CONTRACT = 0, NO_COLUMN_SOFTMAX = 1, SCALE_ONE_SIDE = 2, DUSTBIN_FROM_LS_Z = 3, INVALID_COLUMNS_IN_ROW_NORMALISER = 4, Z_FROM_PROJECTED = 5 };

static float from_bits(uint32_t u) {
    float f;
    memcpy(&f, &u, 4);
    return f;
}
static uint32_t to_bits(float f) {
    uint32_t u;
    memcpy(&u, &f, 4);
    return u;
}

/* exp_c of DESIGN.md 5.12, t <= 0 or NaN */
float mar_exp_c(float t) {
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

/* log_c of DESIGN.md 5.23, x a positive normal number or NaN */
float mar_log_c(float x) {
    if (x != x) {
        return x;
    }
    const uint32_t ix = to_bits(x) + (0x3f800000u - 0x3f3504f3u);
    const float dk = (float)((int)(ix >> 23) - 127);
    const float f = from_bits((ix & 0x007fffffu) + 0x3f3504f3u) - 1.0f;
    const float s = f / (2.0f + f);
    const float z = s * s;
    const float w = z * z;
    const float t1 = w * fmaf(w, 0x1.f13c4cp-3f, 0x1.999c26p-2f);
    const float t2 = z * fmaf(w, 0x1.23d3dcp-2f, 0x1.555554p-1f);
    const float R = t2 + t1;
    const float hfsq = (0.5f * f) * f;
    float r = fmaf(s, hfsq + R, dk * 0x1.2fefa2p-17f);
    r = (r - hfsq) + f;
    return fmaf(dk, 0x1.62e3p-1f, r);
}

float mar_ls(float z) { return fminf(z, 0.0f) - mar_log_c(1.0f + mar_exp_c(-fabsf(z))); }

/* step 3: the normaliser of the `n` values x[0], x[step], ... */
static float normaliser(const float *x, int64_t step, int n) {
    float m = x[0];
    for (int k = 1; k < n; ++k) {
        if (x[k * step] > m) {
            m = x[k * step];
        }
    }
    float p[64];
    for (int l = 0; l < 64; ++l) {
        p[l] = 0.0f;
    }
    for (int k = 0; k < n; ++k) {
        p[k & 63] = p[k & 63] + mar_exp_c(x[k * step] - m);
    }
    for (int off = 32; off >= 1; off >>= 1) {
        float q[64];
        for (int l = 0; l < 64; ++l) {
            q[l] = p[l] + p[l ^ off];
        }
        memcpy(p, q, sizeof(p));
    }
    return m + mar_log_c(p[0]);
}

static int clamp(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

/* desc0 [M][D], desc1 [N][D]; weights [D + 1][D] and bias [D + 1] or NULL (then `scale`); count0 / count1: one int32 or NULL (absent); scores: M + 1 rows
 * of row_stride floats, N + 1 written in each. */
int mar_assign(const float *desc0, int32_t M, const float *desc1, int32_t N, int32_t D, const float *weights, const float *bias, float scale,
               const int32_t *count0, const int32_t *count1, int32_t variant, float *scores, int64_t row_stride) {
    if (M < 1 || N < 1 || D < 1 || row_stride < N + 1) {
        return -1;
    }
    const int n0 = count0 ? clamp(count0[0], 0, M) : M, n1 = count1 ? clamp(count1[0], 0, N) : N;
    const int rows = M + N;
    float *md = (float *)malloc(sizeof(float) * (size_t)rows * D);
    float *z = (float *)calloc((size_t)rows, sizeof(float));
    float *sim = (float *)malloc(sizeof(float) * (size_t)M * N);
    float *lse_row = (float *)calloc((size_t)M, sizeof(float)), *lse_col = (float *)calloc((size_t)N, sizeof(float));
    const float q = (float)sqrt(sqrt((double)D));
    /* 1. projection */
    for (int r = 0; r < rows; ++r) {
        const float *x = r < M ? desc0 + (size_t)r * D : desc1 + (size_t)(r - M) * D;
        const int one_side = variant == SCALE_ONE_SIDE && r >= M;
        if (!weights) {
            for (int c = 0; c < D; ++c) {
                md[(size_t)r * D + c] = one_side ? x[c] : x[c] * scale;
            }
            continue;
        }
        for (int o = 0; o < D; ++o) {
            float acc = bias[o];
            for (int c = 0; c < D; ++c) {
                acc = fmaf(x[c], weights[(size_t)o * D + c], acc);
            }
            md[(size_t)r * D + o] = one_side ? acc : acc / q;
        }
        float acc = bias[D];
        for (int c = 0; c < D; ++c) {
            acc = fmaf(variant == Z_FROM_PROJECTED ? md[(size_t)r * D + c] : x[c], weights[(size_t)D * D + c], acc);
        }
        z[r] = acc;
    }
    /* 2. similarity */
    for (int i = 0; i < M; ++i) {
        for (int j = 0; j < N; ++j) {
            float acc = 0.0f;
            for (int o = 0; o < D; ++o) {
                acc = fmaf(md[(size_t)i * D + o], md[(size_t)(M + j) * D + o], acc);
            }
            sim[(size_t)i * N + j] = acc;
        }
    }
    /* 3. normalisers over the valid block */
    const int row_span = variant == INVALID_COLUMNS_IN_ROW_NORMALISER ? N : n1;
    for (int i = 0; i < n0 && row_span > 0; ++i) {
        lse_row[i] = normaliser(sim + (size_t)i * N, 1, row_span);
    }
    for (int j = 0; j < n1 && n0 > 0; ++j) {
        lse_col[j] = variant == NO_COLUMN_SOFTMAX ? 0.0f : normaliser(sim + j, N, n0);
    }
    /* 4. - 6. */
    const float ninf = -INFINITY;
    for (int i = 0; i <= M; ++i) {
        float *out = scores + (size_t)i * row_stride;
        for (int j = 0; j <= N; ++j) {
            float v = ninf;
            if (i == M && j == N) {
                v = 0.0f;
            } else if (i == M) {
                if (j < n1 && weights) {
                    v = mar_ls(variant == DUSTBIN_FROM_LS_Z ? z[M + j] : -z[M + j]);
                }
            } else if (i < n0 && j == N) {
                if (weights) {
                    v = mar_ls(variant == DUSTBIN_FROM_LS_Z ? z[i] : -z[i]);
                }
            } else if (i < n0 && j < n1) {
                const float s = sim[(size_t)i * N + j];
                v = (s - lse_row[i]) + (s - lse_col[j]);
                if (weights) {
                    v = v + (mar_ls(z[i]) + mar_ls(z[M + j]));
                }
            }
            out[j] = v;
        }
    }
    free(md);
    free(z);
    free(sim);
    free(lse_row);
    free(lse_col);
    return 0;
}
