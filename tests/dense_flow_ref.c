/* dense_flow_ref.c — scalar CPU restatement of feature_tracker::DenseOpticalFlow (Farneback), TEST INFRASTRUCTURE ONLY.
 *
 * Mirrors src/dense_optical_flow_tracker/dense_optical_flow.cpp function by function (file:line citations below), with the
 * two un-vendored substrate pieces DEFINED as DESIGN.md section 2 states them:
 *   - Utility::Interpolate(Mat, r, c): clamp-to-edge bilinear (dfr_interpolate);
 *   - the 3x3 median of SmoothFlow: the 5th smallest value under a total order (-0 < +0, every NaN above +inf) (dfr_median9).
 * Built by tests/dense_flow_ref.py with the oracle's flags (gcc -O3 -ffp-contract=off); the product never loads it.
 * Pinned independently by ref64 (tests/dense_ref64.py, a float64 numpy restatement written from the reference's source alone):
 * tests/test_dense_ref64_cpu.py holds this file to it stage by stage and end to end, tests/test_dense_ref64_gpu.py the kernels.
 * Mat planes are row-major float arrays here (the layout does not enter any arithmetic). */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

/* static_cast<int32_t>(float) as x86-64 cvttss2si (out of range / NaN -> INT32_MIN), DESIGN.md section 2 */
static int32_t f2i_x86(float x) {
    if (x >= -2147483648.0f && x < 2147483648.0f) {
        return (int32_t)x;
    }
    return INT32_MIN;
}

static int32_t clampi(int32_t x, int32_t lo, int32_t hi) { return x < lo ? lo : (x > hi ? hi : x); }

typedef struct dfr_options {
    int32_t max_iteration;     /* kMaxIteration     (10)   */
    int32_t half_patch;        /* kHalfPatchSize    (2)    */
    float max_converge_step;   /* kMaxConvergeStep  (1e-6) */
    float max_delta_flow_step; /* kMaxDeltaFlowStep (1.0)  */
} dfr_options;

/* Utility::Interpolate(Mat, r, c) — clamp-to-edge bilinear; ((tl + tr) + bl) + br */
float dfr_interpolate(const float *m, int32_t rows, int32_t cols, float r, float c) {
    const float fr = floorf(r), fc = floorf(c);
    const float sr = r - fr, sc = c - fc;
    const int32_t r0i = f2i_x86(fr), c0i = f2i_x86(fc);
    const int32_t r1i = (int32_t)((uint32_t)r0i + 1u), c1i = (int32_t)((uint32_t)c0i + 1u);
    const int32_t r0 = clampi(r0i, 0, rows - 1), r1 = clampi(r1i, 0, rows - 1);
    const int32_t c0 = clampi(c0i, 0, cols - 1), c1 = clampi(c1i, 0, cols - 1);
    const float w00 = (1.0f - sr) * (1.0f - sc), w01 = (1.0f - sr) * sc, w10 = sr * (1.0f - sc), w11 = sr * sc;
    const float tl = m[(int64_t)r0 * cols + c0] * w00;
    const float tr = m[(int64_t)r0 * cols + c1] * w01;
    const float bl = m[(int64_t)r1 * cols + c0] * w10;
    const float br = m[(int64_t)r1 * cols + c1] * w11;
    return ((tl + tr) + bl) + br;
}

/* total-order key: -0 < +0, every NaN above +inf */
static int32_t order_key(float v) {
    if (v != v) {
        return INT32_MAX;
    }
    int32_t b;
    memcpy(&b, &v, 4);
    return b < 0 ? (b ^ 0x7FFFFFFF) : b;
}

static float key_value(int32_t k) {
    const int32_t b = k < 0 ? (k ^ 0x7FFFFFFF) : k;
    float v;
    memcpy(&v, &b, 4);
    return v;
}

/* SmoothFlow's std::nth_element(.., begin() + 4, ..) (dense_optical_flow.cpp:360-363), defined as the 5th smallest */
float dfr_median9(const float *v) {
    int32_t k[9];
    for (int i = 0; i < 9; ++i) {
        k[i] = order_key(v[i]);
    }
    for (int i = 1; i < 9; ++i) {
        const int32_t x = k[i];
        int j = i - 1;
        while (j >= 0 && k[j] > x) {
            k[j + 1] = k[j];
            --j;
        }
        k[j + 1] = x;
    }
    return key_value(k[4]);
}

/* InitializeGaussianKernel (:87-134).  k = {k2, k4, k22} in/out: untouched for half_patch 0 (the object's previous values). */
int dfr_gaussian(int32_t half_patch, float *weights, float *k) {
    if (half_patch < 0) {
        return 0; /* :88 */
    }
    const int32_t center = half_patch, size = 2 * center + 1;
    memset(weights, 0, sizeof(float) * (size_t)size * size);
    if (center == 0) { /* :95-98 */
        weights[0] = 1.0f;
        return 1;
    }
    const float sigma = 1.0f, sigma2 = sigma * sigma;
    float sum = 0.0f;
    for (int32_t row = 0; row < size; ++row) { /* :106-113 */
        for (int32_t col = 0; col < size; ++col) {
            const int32_t dr = row - center, dc = col - center;
            weights[row * size + col] = expf(-0.5f * (float)(dr * dr + dc * dc) / sigma2);
            sum += weights[row * size + col];
        }
    }
    for (int32_t i = 0; i < size * size; ++i) { /* :116 */
        weights[i] /= sum;
    }
    k[0] = k[1] = k[2] = 0.0f; /* :119-131 */
    for (int32_t row = 0; row < size; ++row) {
        for (int32_t col = 0; col < size; ++col) {
            const int32_t dr = row - center, dc = col - center;
            const float w = weights[row * size + col];
            k[0] += w * (float)dr * (float)dr;
            k[1] += w * (float)dr * (float)dr * (float)dr * (float)dr;
            k[2] += w * (float)dr * (float)dr * (float)dc * (float)dc;
        }
    }
    return 1;
}

/* ComputeGaussianWeightedSecondMomentMatrix (:136-189) on a float image; planes S0, Sr, Sc, Src, Srr, Scc, each rows*cols */
void dfr_moments_f32(const float *img, int32_t rows, int32_t cols, int32_t half_patch, const float *weights, float *S) {
    const size_t n = (size_t)rows * cols;
    const int32_t size = 2 * half_patch + 1;
    for (int32_t row = 0; row < rows; ++row) {
        for (int32_t col = 0; col < cols; ++col) {
            float s0 = 0.0f, sr = 0.0f, sc = 0.0f, src = 0.0f, srr = 0.0f, scc = 0.0f;
            for (int32_t dr = -half_patch; dr <= half_patch; ++dr) {
                for (int32_t dc = -half_patch; dc <= half_patch; ++dc) {
                    const int32_t r = clampi(row + dr, 0, rows - 1), c = clampi(col + dc, 0, cols - 1); /* :161-170 */
                    const float w = weights[(dr + half_patch) * size + (dc + half_patch)];
                    const float val = img[(int64_t)r * cols + c];
                    s0 += val * w; /* :177-182 */
                    sr += (float)dr * val * w;
                    sc += (float)dc * val * w;
                    src += (float)(dr * dc) * val * w;
                    srr += (float)(dr * dr) * val * w;
                    scc += (float)(dc * dc) * val * w;
                }
            }
            const size_t i = (size_t)row * cols + col;
            S[i] = s0;
            S[n + i] = sr;
            S[2 * n + i] = sc;
            S[3 * n + i] = src;
            S[4 * n + i] = srr;
            S[5 * n + i] = scc;
        }
    }
}

void dfr_moments_u8(const uint8_t *img, int32_t rows, int32_t cols, int32_t half_patch, const float *weights, float *S) {
    const size_t n = (size_t)rows * cols;
    float *f = (float *)malloc(sizeof(float) * (n ? n : 1));
    for (size_t i = 0; i < n; ++i) {
        f[i] = (float)img[i];
    }
    dfr_moments_f32(f, rows, cols, half_patch, weights, S);
    free(f);
}

/* ConstructConstrainFunctionForPixel (:247-303 integer, :305-332 float after the six interpolations).
 * m = {S0, Sr, Sc, Src, Srr, Scc}; A = {a00, a01 (= a10), a11}; b = {b0, b1} */
void dfr_coefficients(const float *m, const float *k, float *A, float *b) {
    const float S0 = m[0], Sr = m[1], Sc = m[2], Src = m[3], Srr = m[4], Scc = m[5];
    const float k2 = k[0], k4 = k[1], k22 = k[2];
    const float D = k4 - k2 * k2;
    const float E = k22 - k2 * k2;
    const float inv_D_plus_E = 1.0f / (D + E + 1e-6f);
    const float inv_D_minus_E = 1.0f / (D - E + 1e-6f);
    const float term1 = (Srr + Scc - 2.0f * k2 * S0) * inv_D_plus_E;
    const float term2 = (Srr - Scc) * inv_D_minus_E;
    const float a = 0.5f * (term1 + term2);
    const float b_coeff = 0.5f * (term1 - term2);
    const float c_coeff = Src / (k22 + 1e-6f);
    A[0] = a;
    A[1] = 0.5f * c_coeff;
    A[2] = b_coeff;
    b[0] = Sr / (k2 + 1e-6f);
    b[1] = Sc / (k2 + 1e-6f);
}

/* ComputeFlowByPixel (:191-245) */
static void flow_by_pixel(int32_t row, int32_t col, const float *Sref, int32_t rr, int32_t rc, const float *Scur, int32_t cr, int32_t cc,
                          const float *k, const dfr_options *opt, float *flow_r, float *flow_c) {
    const size_t nref = (size_t)rr * rc, ncur = (size_t)cr * cc, i = (size_t)row * rc + col;
    float m1[6], A1[3], b1[2];
    for (int q = 0; q < 6; ++q) {
        m1[q] = Sref[q * nref + i];
    }
    dfr_coefficients(m1, k, A1, b1);
    for (int32_t iter = 0; iter < opt->max_iteration; ++iter) {
        const float sample_r = (float)row + flow_r[i]; /* :202-207 */
        const float sample_c = (float)col + flow_c[i];
        float m2[6], A2[3], b2[2];
        for (int q = 0; q < 6; ++q) { /* :307-312: the moments are interpolated, never A / b */
            m2[q] = dfr_interpolate(Scur + q * ncur, cr, cc, sample_r, sample_c);
        }
        dfr_coefficients(m2, k, A2, b2);
        /* :215-216 A_avg = (A1 + A2) * 0.5f, b_diff = b1 - b2; :220 M = A_avg * 2.0f (symmetric: M01 = M10) */
        const float M00 = ((A1[0] + A2[0]) * 0.5f) * 2.0f;
        const float M01 = ((A1[1] + A2[1]) * 0.5f) * 2.0f;
        const float M10 = M01;
        const float M11 = ((A1[2] + A2[2]) * 0.5f) * 2.0f;
        const float bd0 = b1[0] - b2[0], bd1 = b1[1] - b2[1];
        /* :221-222 MtM = M^T M, Mtb = M^T b_diff */
        const float T00 = M00 * M00 + M10 * M10, T01 = M00 * M01 + M10 * M11;
        const float T10 = M01 * M00 + M11 * M10, T11 = M01 * M01 + M11 * M11;
        const float g0 = M00 * bd0 + M10 * bd1, g1 = M01 * bd0 + M11 * bd1;
        /* :225-226 lambda = 0.1 trace + 1; H = MtM + I * lambda (off-diagonal + 0 * lambda) */
        const float lambda = 0.1f * (T00 + T11) + 1.0f;
        const float H00 = T00 + 1.0f * lambda, H01 = T01 + 0.0f * lambda;
        const float H10 = T10 + 0.0f * lambda, H11 = T11 + 1.0f * lambda;
        /* :227 H.inverse() (Eigen's 2x2 closed form) * Mtb */
        const float invdet = 1.0f / (H00 * H11 - H10 * H01);
        const float I00 = H11 * invdet, I01 = -H01 * invdet, I10 = -H10 * invdet, I11 = H00 * invdet;
        float d0 = I00 * g0 + I01 * g1;
        float d1 = I10 * g0 + I11 * g1;
        /* :230-234 cap */
        const float step_norm = sqrtf(d0 * d0 + d1 * d1);
        if (step_norm > opt->max_delta_flow_step) {
            const float s = opt->max_delta_flow_step / step_norm;
            d0 *= s;
            d1 *= s;
        }
        flow_r[i] += d0; /* :237-238 */
        flow_c[i] += d1;
        if (d0 * d0 + d1 * d1 < opt->max_converge_step) { /* :241 */
            break;
        }
    }
}

/* SmoothFlow (:334-371) */
static void smooth_flow(const float *in, int32_t rows, int32_t cols, float *out) {
    for (int32_t r = 0; r < rows; ++r) {
        for (int32_t c = 0; c < cols; ++c) {
            float w[9];
            int n = 0;
            for (int32_t dr = -1; dr <= 1; ++dr) {
                for (int32_t dc = -1; dc <= 1; ++dc) {
                    w[n++] = in[(int64_t)clampi(r + dr, 0, rows - 1) * cols + clampi(c + dc, 0, cols - 1)];
                }
            }
            out[(int64_t)r * cols + c] = dfr_median9(w);
        }
    }
}

/* Track(GrayImage, GrayImage, flow_rc) (:7-33).  flow_r / flow_c hold rr*rc floats; flow_valid bit 0 / 1: that plane is
 * ref-sized (the initial guess), otherwise it is reset to zero (:18-23).  k: the object's {k2, k4, k22}, in/out.
 * Returns 0 (flow untouched) where the reference returns false. */
int dfr_track_image(const uint8_t *ref, int32_t rr, int32_t rc, const uint8_t *cur, int32_t cr, int32_t cc, const dfr_options *opt, float *k,
                    float *flow_r, float *flow_c, int32_t flow_valid) {
    if (!ref || !cur || opt->half_patch < 0) { /* :9-12 */
        return 0;
    }
    const int32_t size = 2 * opt->half_patch + 1;
    float *weights = (float *)malloc(sizeof(float) * (size_t)size * size);
    dfr_gaussian(opt->half_patch, weights, k);
    const size_t nref = (size_t)rr * rc, ncur = (size_t)cr * cc;
    float *Sref = (float *)malloc(sizeof(float) * 6 * (nref ? nref : 1));
    float *Scur = (float *)malloc(sizeof(float) * 6 * (ncur ? ncur : 1));
    dfr_moments_u8(ref, rr, rc, opt->half_patch, weights, Sref); /* :14-15 */
    dfr_moments_u8(cur, cr, cc, opt->half_patch, weights, Scur);
    if (!(flow_valid & 1)) {
        memset(flow_r, 0, sizeof(float) * nref);
    }
    if (!(flow_valid & 2)) {
        memset(flow_c, 0, sizeof(float) * nref);
    }
    for (int32_t row = 0; row < rr; ++row) { /* :25-29 */
        for (int32_t col = 0; col < rc; ++col) {
            flow_by_pixel(row, col, Sref, rr, rc, Scur, cr, cc, k, opt, flow_r, flow_c);
        }
    }
    float *tmp = (float *)malloc(sizeof(float) * (nref ? nref : 1)); /* :31 */
    smooth_flow(flow_r, rr, rc, tmp);
    memcpy(flow_r, tmp, sizeof(float) * nref);
    smooth_flow(flow_c, rr, rc, tmp);
    memcpy(flow_c, tmp, sizeof(float) * nref);
    free(tmp);
    free(Sref);
    free(Scur);
    free(weights);
    return 1;
}

/* Track(ImagePyramid, ImagePyramid, flow_rc) (:35-85).  Levels as arrays of pointers / sizes; flow_r / flow_c receive level 0's
 * ref size.  Returns 0 where the reference returns false. */
int dfr_track_pyramid(const uint8_t *const *ref, const int32_t *ref_rows, const int32_t *ref_cols, const uint8_t *const *cur, const int32_t *cur_rows,
                      const int32_t *cur_cols, int32_t n_levels, const dfr_options *opt, float *k, float *flow_r, float *flow_c) {
    if (n_levels <= 0) {
        return 0;
    }
    const int32_t top = n_levels - 1;
    size_t cap = 1;
    for (int32_t l = 0; l < n_levels; ++l) {
        const size_t n = (size_t)ref_rows[l] * ref_cols[l];
        cap = n > cap ? n : cap;
    }
    float *tr = (float *)calloc(cap, sizeof(float)), *tc = (float *)calloc(cap, sizeof(float)); /* :42-46 */
    float *ur = (float *)malloc(sizeof(float) * cap), *uc = (float *)malloc(sizeof(float) * cap);
    for (int32_t level = top; level >= 0; --level) {
        dfr_track_image(ref[level], ref_rows[level], ref_cols[level], cur[level], cur_rows[level], cur_cols[level], opt, k, tr, tc, 3); /* :53 */
        if (level == 0) {
            break;
        }
        const int32_t nr = ref_rows[level - 1], nc = ref_cols[level - 1]; /* :63-77 */
        for (int32_t r = 0; r < nr; ++r) {
            for (int32_t c = 0; c < nc; ++c) {
                const float fr = (float)r * 0.5f, fc = (float)c * 0.5f;
                ur[(size_t)r * nc + c] = dfr_interpolate(tr, ref_rows[level], ref_cols[level], fr, fc) * 2.0f;
                uc[(size_t)r * nc + c] = dfr_interpolate(tc, ref_rows[level], ref_cols[level], fr, fc) * 2.0f;
            }
        }
        memcpy(tr, ur, sizeof(float) * (size_t)nr * nc);
        memcpy(tc, uc, sizeof(float) * (size_t)nr * nc);
    }
    memcpy(flow_r, tr, sizeof(float) * (size_t)ref_rows[0] * ref_cols[0]);
    memcpy(flow_c, tc, sizeof(float) * (size_t)ref_rows[0] * ref_cols[0]);
    free(tr);
    free(tc);
    free(ur);
    free(uc);
    return 1;
}
