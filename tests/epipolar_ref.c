/* epipolar_ref.c — the scalar CPU restatement of two-view outlier rejection: RANSAC on the fundamental matrix, one
 * hypothesis and one point at a time, in the float32 operation order the contract states.  TEST INFRASTRUCTURE: built by
 * tests/epipolar_ref.py with gcc -ffp-contract=off; the package never sees it.  `variant` other than 0 is one deliberate mistake
 * (tests/test_epipolar_cpu.py shows that each is caught). */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

enum { CONTRACT = 0, MUTANT_HIGHEST_H = 1, MUTANT_TRANSPOSED = 2, MUTANT_DUPLICATES = 3, MUTANT_UNSCALED = 4, MUTANT_NON_PARTICIPANTS = 5 };
enum { TRACKED = 1, LARGE_RESIDUAL = 2, SAMPLE = 8, ATTEMPTS = 16 };

static int finite_f(float v) {
    uint32_t b;
    memcpy(&b, &v, 4);
    return (b & 0x7F800000u) != 0x7F800000u;
}

static uint32_t fmix32(uint32_t x) {
    x ^= x >> 16;
    x *= 0x85EBCA6Bu;
    x ^= x >> 13;
    x *= 0xC2B2AE35u;
    x ^= x >> 16;
    return x;
}

uint32_t epr_mix32(uint32_t seed, uint32_t h, uint32_t k, uint32_t a) {
    return fmix32(fmix32(seed + 0x9E3779B9u * (h + 1u)) ^ (0x85EBCA6Bu * (k * (uint32_t)ATTEMPTS + a + 1u)));
}

/* q = normalised (x1, y1, x2, y2) */
static int inlier(const float *f, const float *q, float tn2, int transposed) {
    float x1 = q[0], y1 = q[1], x2 = q[2], y2 = q[3];
    if (transposed) {
        x1 = q[2], y1 = q[3], x2 = q[0], y2 = q[1];
    }
    if (!(finite_f(x1) && finite_f(y1) && finite_f(x2) && finite_f(y2))) {
        return 0;
    }
    const float a0 = (f[0] * x1 + f[1] * y1) + f[2];
    const float a1 = (f[3] * x1 + f[4] * y1) + f[5];
    const float a2 = (f[6] * x1 + f[7] * y1) + f[8];
    const float b0 = (f[0] * x2 + f[3] * y2) + f[6];
    const float b1 = (f[1] * x2 + f[4] * y2) + f[7];
    const float num = (x2 * a0 + y2 * a1) + a2;
    const float den = ((a0 * a0 + a1 * a1) + b0 * b0) + b1 * b1;
    const float lhs = num * num, rhs = tn2 * den;
    return den > 0.0f && finite_f(lhs) && finite_f(rhs) && lhs <= rhs;
}

/* The normalised F of one sample (8 rows of normalised (x1, y1, x2, y2)); 0 = invalid, f zeroed. */
static int fit(const float (*q)[4], float *f) {
    float a[8][9];
    int perm[9];
    int ok = 1;
    for (int k = 0; k < 8; ++k) {
        const float x1 = q[k][0], y1 = q[k][1], x2 = q[k][2], y2 = q[k][3];
        ok = ok && finite_f(x1) && finite_f(y1) && finite_f(x2) && finite_f(y2);
        a[k][0] = x2 * x1;
        a[k][1] = x2 * y1;
        a[k][2] = x2;
        a[k][3] = y2 * x1;
        a[k][4] = y2 * y1;
        a[k][5] = y2;
        a[k][6] = x1;
        a[k][7] = y1;
        a[k][8] = 1.0f;
    }
    for (int c = 0; c < 9; ++c) {
        perm[c] = c;
        f[c] = 0.0f;
    }
    for (int s = 0; ok && s < 8; ++s) {
        float best = -1.0f;
        int br = s, bc = s;
        for (int r = s; r < 8; ++r) {
            for (int c = s; c < 9; ++c) {
                const float v = fabsf(a[r][c]);
                if (v > best) {
                    best = v, br = r, bc = c;
                }
            }
        }
        const float piv = a[br][bc];
        if (!finite_f(piv) || piv == 0.0f) {
            ok = 0;
            break;
        }
        for (int c = 0; c < 9; ++c) {
            const float t = a[s][c];
            a[s][c] = a[br][c];
            a[br][c] = t;
        }
        for (int r = 0; r < 8; ++r) {
            const float t = a[r][s];
            a[r][s] = a[r][bc];
            a[r][bc] = t;
        }
        const int t = perm[s];
        perm[s] = perm[bc];
        perm[bc] = t;
        for (int r = s + 1; r < 8; ++r) {
            const float mult = a[r][s] / piv;
            for (int c = s + 1; c < 9; ++c) {
                a[r][c] = a[r][c] - mult * a[s][c];
            }
        }
    }
    if (!ok) {
        return 0;
    }
    float z[9], v[9];
    z[8] = 1.0f;
    for (int s = 7; s >= 0; --s) {
        float acc = a[s][8];
        for (int c = s + 1; c < 8; ++c) {
            acc = acc + a[s][c] * z[c];
        }
        z[s] = -acc / a[s][s];
    }
    for (int c = 0; c < 9; ++c) {
        v[perm[c]] = z[c];
    }
    float n2 = v[0] * v[0];
    for (int i = 1; i < 9; ++i) {
        n2 = n2 + v[i] * v[i];
    }
    if (!(finite_f(n2) && n2 > 0.0f)) {
        return 0;
    }
    const float inv = 1.0f / sqrtf(n2);
    for (int i = 0; i < 9; ++i) {
        v[i] = v[i] * inv;
        ok = ok && finite_f(v[i]);
    }
    if (ok) {
        memcpy(f, v, sizeof(v));
    }
    return ok;
}

/* samples: [K][8] the point index of every draw (-1 from the first draw that ran out of attempts on); may be NULL, as counts and models. */
int32_t epr_ransac(const float *ref_uv, const float *cur_uv, uint8_t *status, int32_t n, int32_t rows, int32_t cols, float threshold, int32_t K,
                   uint32_t seed, int32_t variant, int32_t *best_out, int32_t *n_inliers_out, float *F, int32_t *counts_out, float *models_out,
                   int32_t *samples_out) {
    if (n < 1 || K < 1 || rows < 1 || cols < 1) {
        return -1;
    }
    const float cx = 0.5f * (float)(cols - 1), cy = 0.5f * (float)(rows - 1), s = 2.0f / (float)(cols + rows);
    const float tn = variant == MUTANT_UNSCALED ? threshold : threshold * s;
    const float tn2 = tn * tn;
    float(*pts)[4] = malloc(sizeof(float[4]) * (size_t)n);   /* every point, normalised */
    int32_t *list = malloc(sizeof(int32_t) * (size_t)n);     /* the participants, ascending */
    int32_t *counts = malloc(sizeof(int32_t) * (size_t)K);
    float *models = malloc(sizeof(float) * 9 * (size_t)K);
    int32_t m = 0;
    for (int32_t i = 0; i < n; ++i) {
        pts[i][0] = (ref_uv[2 * i] - cx) * s;
        pts[i][1] = (ref_uv[2 * i + 1] - cy) * s;
        pts[i][2] = (cur_uv[2 * i] - cx) * s;
        pts[i][3] = (cur_uv[2 * i + 1] - cy) * s;
        if (status[i] == TRACKED) {
            list[m++] = i;
        }
    }
    const uint32_t pool = variant == MUTANT_NON_PARTICIPANTS ? (uint32_t)n : (uint32_t)m;
    int32_t best = -1, best_count = -1;
    for (int32_t h = 0; h < K; ++h) {
        uint32_t idx[SAMPLE];
        float q[SAMPLE][4];
        int ok = m >= SAMPLE;
        for (int k = 0; k < SAMPLE; ++k) {
            int found = 0;
            for (uint32_t t = 0; ok && !found && t < ATTEMPTS; ++t) {
                const uint32_t j = (uint32_t)(((uint64_t)epr_mix32(seed, (uint32_t)h, (uint32_t)k, t) * (uint64_t)pool) >> 32);
                int dup = 0;
                for (int e = 0; e < k; ++e) {
                    dup = dup || idx[e] == j;
                }
                if (!dup || variant == MUTANT_DUPLICATES) {
                    idx[k] = j;
                    found = 1;
                }
            }
            ok = ok && found;
            if (samples_out) {
                samples_out[h * SAMPLE + k] = ok ? (variant == MUTANT_NON_PARTICIPANTS ? (int32_t)idx[k] : list[idx[k]]) : -1;
            }
        }
        if (ok) {
            for (int k = 0; k < SAMPLE; ++k) {
                memcpy(q[k], pts[variant == MUTANT_NON_PARTICIPANTS ? (int32_t)idx[k] : list[idx[k]]], sizeof(float[4]));
            }
            ok = fit(q, models + 9 * h);
        }
        if (!ok) {
            memset(models + 9 * h, 0, sizeof(float) * 9);
            counts[h] = -1;
        } else {
            counts[h] = 0;
            for (int32_t j = 0; j < m; ++j) {
                counts[h] += inlier(models + 9 * h, pts[list[j]], tn2, variant == MUTANT_TRANSPOSED);
            }
        }
        if (counts[h] > best_count || (variant == MUTANT_HIGHEST_H && counts[h] >= 0 && counts[h] == best_count)) {
            best_count = counts[h];
            best = h;
        }
    }
    if (best_count < 0) {
        best = -1;
    }
    *best_out = best;
    *n_inliers_out = best < 0 ? m : best_count;
    for (int i = 0; i < 9; ++i) {
        F[i] = 0.0f;
    }
    if (best >= 0) {
        const float *f = models + 9 * best;
        const float tx = -(cx * s), ty = -(cy * s);
        float g[9];
        for (int r = 0; r < 3; ++r) {
            g[r * 3 + 0] = f[r * 3 + 0] * s;
            g[r * 3 + 1] = f[r * 3 + 1] * s;
            g[r * 3 + 2] = (f[r * 3 + 0] * tx + f[r * 3 + 1] * ty) + f[r * 3 + 2];
        }
        for (int c = 0; c < 3; ++c) {
            F[0 + c] = s * g[0 + c];
            F[3 + c] = s * g[3 + c];
            F[6 + c] = (tx * g[0 + c] + ty * g[3 + c]) + g[6 + c];
        }
        for (int32_t j = 0; j < m; ++j) {
            if (!inlier(f, pts[list[j]], tn2, variant == MUTANT_TRANSPOSED)) {
                status[list[j]] = LARGE_RESIDUAL;
            }
        }
    }
    if (counts_out) {
        memcpy(counts_out, counts, sizeof(int32_t) * (size_t)K);
    }
    if (models_out) {
        memcpy(models_out, models, sizeof(float) * 9 * (size_t)K);
    }
    free(pts);
    free(list);
    free(counts);
    free(models);
    return 0;
}
