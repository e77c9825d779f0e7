/* flow_points_ref.c — scalar CPU restatement of sparse tracking from RAFT's coarse flow as DESIGN.md 5.17 states it: feature points moved
 * by the bilinear sample of the convex-upsampled flow (Raft.UpsampleFlow, src/nn_optical_flow_tracker/raft/model.py:48-64), their
 * TrackStatus and the forward-backward error.  TEST INFRASTRUCTURE ONLY: independent code, it includes nothing from feature_tracker_amd/
 * and nothing there may use it; steps 1 to 6 of DESIGN.md 5.12 below are its own copy.  Compile with -ffp-contract=off: every operation
 * is one correctly rounded float32 operation, the fused ones are written as fmaf.
 *
 * `variant` is a test-only argument: 0 the contract; 1 a mutant that reads a point's (u, v) as (v, u) when it samples (indices held to
 * the grid); 2 a mutant whose right / lower neighbour ix0 + 1 wraps to 0 at the grid's edge instead of being clamped to it. */
#include <math.h>
#include <stdint.h>
#include <string.h>

enum { FPR_NOT_TRACKED = 0, FPR_TRACKED = 1, FPR_LARGE_RESIDUAL = 2, FPR_OUTSIDE = 3, FPR_NUMERIC_ERROR = 4 }; /* include/ftk.h's values */

#define FPR_CUTOFF (-87.0f)
#define FPR_LOG2E 0x1.715476p+0f
#define FPR_LN2_HI 0x1.62e4p-1f
#define FPR_LN2_LO 0x1.7f7d1cp-20f

/* exp_c of DESIGN.md 5.12, t <= 0 or NaN */
static float exp_c(float t) {
    if (t != t) {
        return t;
    }
    if (t < FPR_CUTOFF) {
        return 0.0f;
    }
    const float n = rintf(t * FPR_LOG2E);
    float r = fmaf(n, -FPR_LN2_HI, t);
    r = fmaf(n, -FPR_LN2_LO, r);
    float p = 0x1.a01a02p-13f;
    p = fmaf(p, r, 0x1.6c16c2p-10f);
    p = fmaf(p, r, 0x1.111112p-7f);
    p = fmaf(p, r, 0x1.555556p-5f);
    p = fmaf(p, r, 0x1.555556p-3f);
    p = fmaf(p, r, 0x1p-1f);
    p = fmaf(p, r, 1.0f);
    p = fmaf(p, r, 1.0f);
    const uint32_t bits = (uint32_t)((int32_t)n + 127) << 23;
    float scale;
    memcpy(&scale, &bits, sizeof scale);
    return p * scale;
}

/* Where the fine values come from: the coarse pair (flow [B][2][H][W], mask [B][576][H][W], mask_scale), or a stored fine field
 * `dense` [B][2][8H][8W] (what upsample_flow wrote), never both. */
typedef struct {
    const float *flow, *mask, *dense;
    int64_t H, W;
    float mask_scale;
} fpr_field;

/* the two components of fine pixel (iy, ix) of batch entry b: steps 1 to 6 of DESIGN.md 5.12 */
static void fine_value(const fpr_field *s, int64_t b, int64_t iy, int64_t ix, float out[2]) {
    const int64_t H = s->H, W = s->W, HW = H * W;
    if (s->dense) {
        for (int c = 0; c < 2; ++c) {
            out[c] = s->dense[((b * 2 + c) * 8 * H + iy) * 8 * W + ix];
        }
        return;
    }
    const int64_t y = iy / 8, i = iy % 8, x = ix / 8, j = ix % 8;
    float xs[9], e[9];
    for (int k = 0; k < 9; ++k) { /* step 1 */
        xs[k] = s->mask[(b * 576 + k * 64 + i * 8 + j) * HW + y * W + x] * s->mask_scale;
    }
    float m = xs[0]; /* step 2 */
    for (int k = 1; k < 9; ++k) {
        if (xs[k] > m) {
            m = xs[k];
        }
    }
    for (int k = 0; k < 9; ++k) { /* step 3 */
        e[k] = exp_c(xs[k] - m);
    }
    float sum = e[0] + e[1]; /* step 4 */
    for (int k = 2; k < 9; ++k) {
        sum = sum + e[k];
    }
    for (int c = 0; c < 2; ++c) {
        float acc = 0.0f;
        for (int k = 0; k < 9; ++k) {
            const int64_t yy = y + k / 3 - 1, xx = x + k % 3 - 1;
            const int in = yy >= 0 && yy < H && xx >= 0 && xx < W;
            const float f = in ? 8.0f * s->flow[(b * 2 + c) * HW + yy * W + xx] : 0.0f; /* step 5 */
            const float p = f * (e[k] / sum);                                            /* step 6 */
            acc = k == 0 ? p : acc + p;
        }
        out[c] = acc;
    }
}

/* the contract's three fmaf of one component */
float fpr_bilinear(float v00, float v01, float v10, float v11, float fx, float fy) {
    const float top = fmaf(fx, v01 - v00, v00);
    const float bot = fmaf(fx, v11 - v10, v10);
    return fmaf(fy, bot - top, top);
}

void fpr_bilinear_array(const float *v00, const float *v01, const float *v10, const float *v11, const float *fx, const float *fy, int64_t count,
                        float *out) {
    for (int64_t q = 0; q < count; ++q) {
        out[q] = fpr_bilinear(v00[q], v01[q], v10[q], v11[q], fx[q], fy[q]);
    }
}

static int64_t held(int64_t v, int64_t n) { return v < 0 ? 0 : v > n - 1 ? n - 1 : v; }

/* S(field, u, v) of an inside point: contract step 2 */
static void sample(const fpr_field *s, int64_t b, float u, float v, int variant, float out[2]) {
    const int64_t W8 = 8 * s->W, H8 = 8 * s->H;
    if (variant == 1) {
        const float t = u;
        u = v;
        v = t;
    }
    const float x0 = floorf(u), y0 = floorf(v);
    const float fx = u - x0, fy = v - y0;
    int64_t ix0 = (int64_t)x0, iy0 = (int64_t)y0;
    if (variant == 1) {
        ix0 = held(ix0, W8);
        iy0 = held(iy0, H8);
    }
    const int64_t ix1 = variant == 2 ? (ix0 + 1) % W8 : (ix0 + 1 < W8 - 1 ? ix0 + 1 : W8 - 1);
    const int64_t iy1 = variant == 2 ? (iy0 + 1) % H8 : (iy0 + 1 < H8 - 1 ? iy0 + 1 : H8 - 1);
    float v00[2], v01[2], v10[2], v11[2];
    fine_value(s, b, iy0, ix0, v00);
    fine_value(s, b, iy0, ix1, v01);
    fine_value(s, b, iy1, ix0, v10);
    fine_value(s, b, iy1, ix1, v11);
    for (int c = 0; c < 2; ++c) {
        out[c] = fpr_bilinear(v00[c], v01[c], v10[c], v11[c], fx, fy);
    }
}

static int inside(float u, float v, float last_col, float last_row) { return u >= 0.0f && u <= last_col && v >= 0.0f && v <= last_row; }

static int track(const fpr_field *fwd, const fpr_field *back, int32_t B, int32_t N, int32_t image_rows, int32_t image_cols, float fb_threshold,
                 int32_t variant, const float *points, float *cur_points, uint8_t *status, float *fb_error2) {
    const float last_col = (float)(image_cols - 1), last_row = (float)(image_rows - 1);
    for (int64_t b = 0; b < B; ++b) {
        for (int64_t n = 0; n < N; ++n) {
            const int64_t at = b * N + n;
            const float u = points[2 * at], v = points[2 * at + 1];
            float cx = u, cy = v, e2 = 0.0f;
            uint8_t st = FPR_OUTSIDE;
            if (inside(u, v, last_col, last_row)) { /* step 1 */
                float s[2];
                sample(fwd, b, u, v, variant, s);
                const float x = u + s[0], y = v + s[1]; /* step 3 */
                if (!(isfinite(x) && isfinite(y))) {
                    st = FPR_NUMERIC_ERROR;
                } else {
                    cx = x;
                    cy = y;
                    if (inside(x, y, last_col, last_row)) {
                        st = FPR_TRACKED; /* step 5 */
                        if (back) {       /* step 4 */
                            sample(back, b, cx, cy, variant, s);
                            const float ex = (cx + s[0]) - u, ey = (cy + s[1]) - v;
                            e2 = fmaf(ey, ey, ex * ex);
                            if (!(e2 <= fb_threshold * fb_threshold)) {
                                st = FPR_LARGE_RESIDUAL;
                            }
                        }
                    }
                }
            }
            cur_points[2 * at] = cx;
            cur_points[2 * at + 1] = cy;
            status[at] = st;
            if (fb_error2) {
                fb_error2[at] = e2;
            }
        }
    }
    return 0;
}

static int bad_sizes(int32_t B, int32_t H, int32_t W, int32_t N, int32_t image_rows, int32_t image_cols, int32_t variant) {
    return B < 1 || H < 1 || W < 1 || N < 0 || image_rows < 1 || image_rows > 8 * (int64_t)H || image_cols < 1 || image_cols > 8 * (int64_t)W ||
           variant < 0 || variant > 2;
}

/* flow [B][2][H][W], mask [B][576][H][W] (and the backward pair, both or neither), points [B][N][2] -> cur_points, status, fb_error2 (or NULL) */
int fpr_track(const float *flow, const float *mask, const float *flow_back, const float *mask_back, int32_t B, int32_t H, int32_t W, int32_t N,
              int32_t image_rows, int32_t image_cols, float mask_scale, float fb_threshold, int32_t variant, const float *points, float *cur_points,
              uint8_t *status, float *fb_error2) {
    if (!flow || !mask || !points || !cur_points || !status || (flow_back == NULL) != (mask_back == NULL) ||
        bad_sizes(B, H, W, N, image_rows, image_cols, variant)) {
        return -1;
    }
    const fpr_field fwd = {flow, mask, NULL, H, W, mask_scale}, back = {flow_back, mask_back, NULL, H, W, mask_scale};
    return track(&fwd, flow_back ? &back : NULL, B, N, image_rows, image_cols, fb_threshold, variant, points, cur_points, status, fb_error2);
}

/* the same rules on stored fine fields [B][2][8H][8W] (upsample_flow's output; dense_back or NULL) */
int fpr_track_dense(const float *dense, const float *dense_back, int32_t B, int32_t H, int32_t W, int32_t N, int32_t image_rows, int32_t image_cols,
                    float fb_threshold, int32_t variant, const float *points, float *cur_points, uint8_t *status, float *fb_error2) {
    if (!dense || !points || !cur_points || !status || bad_sizes(B, H, W, N, image_rows, image_cols, variant)) {
        return -1;
    }
    const fpr_field fwd = {NULL, NULL, dense, H, W, 1.0f}, back = {NULL, NULL, dense_back, H, W, 1.0f};
    return track(&fwd, dense_back ? &back : NULL, B, N, image_rows, image_cols, fb_threshold, variant, points, cur_points, status, fb_error2);
}
