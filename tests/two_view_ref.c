/* two_view_ref.c — the scalar CPU restatement of two-view outlier rejection with a choice of model: RANSAC on the
 * fundamental matrix, on a homography, or on both with the rule that picks one; one hypothesis and one point at a time, in the float32
 * operation order the contract states.  TEST INFRASTRUCTURE: built by tests/two_view_ref.py with gcc -ffp-contract=off; the package never
 * sees it, and it shares no line with tests/epipolar_ref.c (tests/test_two_view_cpu.py compares the two).  `variant` other than 0 is one
 * deliberate mistake (tests/test_two_view_cpu.py shows that each is caught). */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

enum { CONTRACT = 0, MUTANT_H_TRANSPOSED = 1, MUTANT_DLT_SIGN = 2, MUTANT_RULE_SWAPPED = 3, MUTANT_LOSER_APPLIED = 4, MUTANT_DUPLICATES = 5 };
enum { TRACKED = 1, LARGE_RESIDUAL = 2, ATTEMPTS = 16, MODE_F = 0, MODE_H = 1, MODE_AUTO = 2 };

static int is_finite(float v) {
    uint32_t b;
    memcpy(&b, &v, 4);
    return ((b >> 23) & 0xFFu) != 0xFFu;
}

static uint32_t fmix(uint32_t x) {
    x ^= x >> 16;
    x *= 0x85EBCA6Bu;
    x ^= x >> 13;
    x *= 0xC2B2AE35u;
    x ^= x >> 16;
    return x;
}

static uint32_t mix(uint32_t seed, uint32_t h, uint32_t k, uint32_t a) {
    return fmix(fmix(seed + 0x9E3779B9u * (h + 1u)) ^ (0x85EBCA6Bu * (k * (uint32_t)ATTEMPTS + a + 1u)));
}

/* `draws` distinct positions of a list of m; 0 when m is too small or a draw runs out of attempts.  got: the draws that succeeded. */
static int draw(uint32_t seed, uint32_t h, uint32_t m, int draws, int duplicates, uint32_t *idx, int *got) {
    *got = 0;
    if (m < (uint32_t)draws) {
        return 0;
    }
    for (int k = 0; k < draws; ++k) {
        int found = 0;
        for (uint32_t t = 0; !found && t < ATTEMPTS; ++t) {
            const uint32_t j = (uint32_t)(((uint64_t)mix(seed, h, (uint32_t)k, t) * (uint64_t)m) >> 32);
            int dup = 0;
            for (int e = 0; e < k; ++e) {
                dup |= idx[e] == j;
            }
            if (!dup || duplicates) {
                idx[k] = j;
                found = 1;
            }
        }
        if (!found) {
            return 0;
        }
        *got = k + 1;
    }
    return 1;
}

/* The unit null vector of an 8 x 9 system by Gaussian elimination with complete pivoting; 0 = invalid, v zeroed. */
static int null_vector(float a[8][9], float *v) {
    int col[9];
    for (int c = 0; c < 9; ++c) {
        col[c] = c;
        v[c] = 0.0f;
    }
    for (int s = 0; s < 8; ++s) {
        float big = -1.0f;
        int pr = s, pc = s;
        for (int r = s; r < 8; ++r) {
            for (int c = s; c < 9; ++c) {
                if (fabsf(a[r][c]) > big) {
                    big = fabsf(a[r][c]), pr = r, pc = c;
                }
            }
        }
        const float piv = a[pr][pc];
        if (!is_finite(piv) || piv == 0.0f) {
            return 0;
        }
        for (int c = 0; c < 9; ++c) {
            const float t = a[s][c];
            a[s][c] = a[pr][c], a[pr][c] = t;
        }
        for (int r = 0; r < 8; ++r) {
            const float t = a[r][s];
            a[r][s] = a[r][pc], a[r][pc] = t;
        }
        const int t = col[s];
        col[s] = col[pc], col[pc] = t;
        for (int r = s + 1; r < 8; ++r) {
            const float mult = a[r][s] / piv;
            for (int c = s + 1; c < 9; ++c) {
                a[r][c] = a[r][c] - mult * a[s][c];
            }
        }
    }
    float z[9], u[9];
    z[8] = 1.0f;
    for (int s = 7; s >= 0; --s) {
        float acc = a[s][8];
        for (int c = s + 1; c < 8; ++c) {
            acc = acc + a[s][c] * z[c];
        }
        z[s] = -acc / a[s][s];
    }
    for (int c = 0; c < 9; ++c) {
        u[col[c]] = z[c];
    }
    float n2 = u[0] * u[0];
    for (int i = 1; i < 9; ++i) {
        n2 = n2 + u[i] * u[i];
    }
    if (!(is_finite(n2) && n2 > 0.0f)) {
        return 0;
    }
    const float inv = 1.0f / sqrtf(n2);
    int ok = 1;
    for (int i = 0; i < 9; ++i) {
        u[i] = u[i] * inv;
        ok = ok && is_finite(u[i]);
    }
    if (ok) {
        memcpy(v, u, sizeof(u));
    }
    return ok;
}

static int fit_f(float q[8][4], float *f) {
    float a[8][9];
    int ok = 1;
    for (int k = 0; k < 8; ++k) {
        const float x1 = q[k][0], y1 = q[k][1], x2 = q[k][2], y2 = q[k][3];
        ok = ok && is_finite(x1) && is_finite(y1) && is_finite(x2) && is_finite(y2);
        const float row[9] = {x2 * x1, x2 * y1, x2, y2 * x1, y2 * y1, y2, x1, y1, 1.0f};
        memcpy(a[k], row, sizeof(row));
    }
    if (!ok) {
        memset(f, 0, sizeof(float) * 9);
        return 0;
    }
    return null_vector(a, f);
}

static int fit_h(float q[4][4], float *g, int wrong_sign) {
    float a[8][9];
    int ok = 1;
    for (int k = 0; k < 4; ++k) {
        const float x1 = q[k][0], y1 = q[k][1], x2 = q[k][2], y2 = q[k][3];
        ok = ok && is_finite(x1) && is_finite(y1) && is_finite(x2) && is_finite(y2);
        const float r0[9] = {x1, y1, 1.0f, 0.0f, 0.0f, 0.0f, -(x2 * x1), -(x2 * y1), -x2};
        const float r1[9] = {0.0f, 0.0f, 0.0f, x1, y1, 1.0f, -(y2 * x1), -(y2 * y1), -y2};
        memcpy(a[2 * k], r0, sizeof(r0));
        memcpy(a[2 * k + 1], r1, sizeof(r1));
        if (wrong_sign) {
            for (int c = 6; c < 9; ++c) {
                a[2 * k][c] = -a[2 * k][c];
                a[2 * k + 1][c] = -a[2 * k + 1][c];
            }
        }
    }
    if (!ok) {
        memset(g, 0, sizeof(float) * 9);
        return 0;
    }
    return null_vector(a, g);
}

static int inlier_f(const float *f, const float *q, float tn2) {
    const float x1 = q[0], y1 = q[1], x2 = q[2], y2 = q[3];
    if (!(is_finite(x1) && is_finite(y1) && is_finite(x2) && is_finite(y2))) {
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
    return den > 0.0f && is_finite(lhs) && is_finite(rhs) && lhs <= rhs;
}

static int inlier_h(const float *gin, const float *q, float tn2, int transposed) {
    float g[9];
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) {
            g[r * 3 + c] = transposed ? gin[c * 3 + r] : gin[r * 3 + c];
        }
    }
    const float x1 = q[0], y1 = q[1], x2 = q[2], y2 = q[3];
    if (!(is_finite(x1) && is_finite(y1) && is_finite(x2) && is_finite(y2))) {
        return 0;
    }
    const float w = (g[6] * x1 + g[7] * y1) + g[8];
    const float px = (g[0] * x1 + g[1] * y1) + g[2];
    const float py = (g[3] * x1 + g[4] * y1) + g[5];
    const float ex = px - x2 * w;
    const float ey = py - y2 * w;
    const float lhs = ex * ex + ey * ey, rhs = tn2 * (w * w);
    return w != 0.0f && is_finite(lhs) && is_finite(rhs) && lhs <= rhs;
}

/* The rule: 1 the homography, 0 the fundamental matrix, -1 neither. */
int32_t tvr_choose(int32_t has_f, int32_t has_h, int32_t n_f, int32_t n_h, int32_t permille, int32_t variant) {
    if (variant == MUTANT_RULE_SWAPPED) {
        const int32_t t = n_f;
        n_f = n_h, n_h = t;
    }
    if (has_h && (!has_f || (int64_t)1000 * (int64_t)n_h >= (int64_t)permille * (int64_t)n_f)) {
        return 1;
    }
    return has_f ? 0 : -1;
}

/* best / n_inliers: [2]; F / H: [9]; counts: [2][K], models: [2][K][9], samples_f: [K][8], samples_h: [K][4] (point indices, -1 from the
 * first draw that ran out of attempts on), each may be NULL. */
int32_t tvr_ransac(const float *ref_uv, const float *cur_uv, uint8_t *status, int32_t n, int32_t rows, int32_t cols, float threshold, int32_t K,
                   uint32_t seed, int32_t mode, int32_t permille, int32_t variant, int32_t *model_out, int32_t *best_out, int32_t *n_inliers_out,
                   float *F, float *H, int32_t *counts_out, float *models_out, int32_t *samples_f, int32_t *samples_h) {
    if (n < 1 || K < 1 || rows < 1 || cols < 1 || mode < 0 || mode > 2 || permille < 0 || permille > 1000) {
        return -1;
    }
    const float cx = 0.5f * (float)(cols - 1), cy = 0.5f * (float)(rows - 1), s = 2.0f / (float)(cols + rows);
    const float tn = threshold * s;
    const float tn2 = tn * tn;
    float(*pts)[4] = malloc(sizeof(float[4]) * (size_t)n); /* the participants, normalised, ascending */
    int32_t *list = malloc(sizeof(int32_t) * (size_t)n);
    int32_t *counts = malloc(sizeof(int32_t) * 2 * (size_t)K);
    float *models = calloc(18 * (size_t)K, sizeof(float));
    int32_t m = 0;
    for (int32_t i = 0; i < n; ++i) {
        if (status[i] == TRACKED) {
            pts[m][0] = (ref_uv[2 * i] - cx) * s;
            pts[m][1] = (ref_uv[2 * i + 1] - cy) * s;
            pts[m][2] = (cur_uv[2 * i] - cx) * s;
            pts[m][3] = (cur_uv[2 * i + 1] - cy) * s;
            list[m++] = i;
        }
    }
    int32_t best[2] = {-1, -1}, top[2] = {-1, -1};
    for (int slot = 0; slot < 2; ++slot) {
        const int runs = slot == 0 ? mode != MODE_H : mode != MODE_F;
        const int draws = slot == 0 ? 8 : 4;
        int32_t *samples = slot == 0 ? samples_f : samples_h;
        for (int32_t h = 0; h < K; ++h) {
            int32_t *count = counts + (size_t)slot * K + h;
            float *model = models + 9 * ((size_t)slot * K + h);
            *count = -1;
            if (samples) {
                for (int k = 0; k < draws; ++k) {
                    samples[h * draws + k] = -1;
                }
            }
            if (!runs) {
                continue;
            }
            uint32_t idx[8];
            int got;
            int ok = draw(seed, (uint32_t)h, (uint32_t)m, draws, variant == MUTANT_DUPLICATES && slot == 1, idx, &got);
            if (samples) {
                for (int k = 0; k < got; ++k) {
                    samples[h * draws + k] = list[idx[k]];
                }
            }
            if (ok) {
                float q[8][4];
                for (int k = 0; k < draws; ++k) {
                    memcpy(q[k], pts[idx[k]], sizeof(float[4]));
                }
                ok = slot == 0 ? fit_f(q, model) : fit_h(q, model, variant == MUTANT_DLT_SIGN);
            }
            if (!ok) {
                memset(model, 0, sizeof(float) * 9);
                continue;
            }
            *count = 0;
            for (int32_t j = 0; j < m; ++j) {
                *count += slot == 0 ? inlier_f(model, pts[j], tn2) : inlier_h(model, pts[j], tn2, variant == MUTANT_H_TRANSPOSED);
            }
            if (*count > top[slot]) {
                top[slot] = *count, best[slot] = h;
            }
        }
    }
    const int has_f = best[0] >= 0, has_h = best[1] >= 0;
    const int32_t n_f = has_f ? top[0] : m, n_h = has_h ? top[1] : m;
    const int32_t model = tvr_choose(has_f, has_h, n_f, n_h, permille, variant);
    *model_out = model;
    best_out[0] = best[0], best_out[1] = best[1];
    n_inliers_out[0] = n_f, n_inliers_out[1] = n_h;
    memset(F, 0, sizeof(float) * 9);
    memset(H, 0, sizeof(float) * 9);
    const float tx = -(cx * s), ty = -(cy * s);
    if (has_f) { /* T^T F T: G = F T, then T^T G */
        const float *f = models + 9 * (size_t)best[0];
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
    }
    if (has_h) { /* T^-1 H T: G = H T, then T^-1 G with T^-1 = [1/s 0 cx; 0 1/s cy; 0 0 1] */
        const float *e = models + 9 * ((size_t)K + (size_t)best[1]);
        const float is = 1.0f / s;
        float g[9];
        for (int r = 0; r < 3; ++r) {
            g[r * 3 + 0] = e[r * 3 + 0] * s;
            g[r * 3 + 1] = e[r * 3 + 1] * s;
            g[r * 3 + 2] = (e[r * 3 + 0] * tx + e[r * 3 + 1] * ty) + e[r * 3 + 2];
        }
        for (int c = 0; c < 3; ++c) {
            H[0 + c] = is * g[0 + c] + cx * g[6 + c];
            H[3 + c] = is * g[3 + c] + cy * g[6 + c];
            H[6 + c] = g[6 + c];
        }
    }
    int applied = model;
    if (variant == MUTANT_LOSER_APPLIED && has_f && has_h) {
        applied = 1 - model;
    }
    if (applied >= 0) {
        const float *w = models + 9 * ((size_t)applied * K + (size_t)best[applied]);
        for (int32_t j = 0; j < m; ++j) {
            const int in = applied == 0 ? inlier_f(w, pts[j], tn2) : inlier_h(w, pts[j], tn2, variant == MUTANT_H_TRANSPOSED);
            if (!in) {
                status[list[j]] = LARGE_RESIDUAL;
            }
        }
    }
    if (counts_out) {
        memcpy(counts_out, counts, sizeof(int32_t) * 2 * (size_t)K);
    }
    if (models_out) {
        memcpy(models_out, models, sizeof(float) * 18 * (size_t)K);
    }
    free(pts);
    free(list);
    free(counts);
    free(models);
    return 0;
}
