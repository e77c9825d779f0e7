/* flow_upsample_ref.c — scalar CPU restatement of RAFT's convex flow upsampling (Raft.UpsampleFlow,
 * src/nn_optical_flow_tracker/raft/model.py:48-64) as DESIGN.md 5.12 states it.  TEST INFRASTRUCTURE ONLY: independent code, it includes
 * nothing from feature_tracker_amd/ and nothing there may use it.  Compile with -ffp-contract=off: every operation below is one
 * correctly rounded float32 operation, the fused ones are written as fmaf.
 *
 * `variant` is a test-only argument: 0 the contract; 1 a mutant with the 3 x 3 window transposed (neighbour k taken at
 * (y + k%3 - 1, x + k/3 - 1)); 2 a mutant whose exp_c polynomial stops at degree 3.  The tests show that each mutant fails the float64
 * comparison the contract passes. */
#include <math.h>
#include <stdint.h>
#include <string.h>

#define FUR_CUTOFF (-87.0f)
#define FUR_LOG2E 0x1.715476p+0f   /* log2(e) rounded to float32 */
#define FUR_LN2_HI 0x1.62e4p-1f    /* the leading 16 bits of ln 2: n * FUR_LN2_HI is exact for |n| < 256 */
#define FUR_LN2_LO 0x1.7f7d1cp-20f /* ln 2 - FUR_LN2_HI rounded to float32 */

/* exp_c(t) for t <= 0: NaN for NaN, +0 below the cutoff, else 2^n * P(r) with n = rint(t * log2e),
 * r = t - n * ln2 in two fmaf steps, P the degree-7 Taylor polynomial of exp in Horner form. */
static float exp_c_degree(float t, int degree) {
    static const float c[8] = {1.0f, 1.0f, 0x1p-1f, 0x1.555556p-3f, 0x1.555556p-5f, 0x1.111112p-7f, 0x1.6c16c2p-10f, 0x1.a01a02p-13f};
    if (t != t) {
        return t;
    }
    if (t < FUR_CUTOFF) {
        return 0.0f;
    }
    const float n = rintf(t * FUR_LOG2E); /* round to nearest even; -126 .. 0 */
    float r = fmaf(n, -FUR_LN2_HI, t);
    r = fmaf(n, -FUR_LN2_LO, r);
    float p = c[degree];
    for (int d = degree - 1; d >= 0; --d) {
        p = fmaf(p, r, c[d]);
    }
    const uint32_t bits = (uint32_t)((int32_t)n + 127) << 23; /* 2^n, a normal number: n >= -126 */
    float scale;
    memcpy(&scale, &bits, sizeof scale);
    return p * scale;
}

float fur_exp_c(float t) { return exp_c_degree(t, 7); }

/* exp_c over an array (the accuracy sweep of tests/test_flow_upsample_cpu.py) */
void fur_exp_c_array(const float *t, int64_t count, float *out) {
    for (int64_t q = 0; q < count; ++q) {
        out[q] = exp_c_degree(t[q], 7);
    }
}

float fur_cutoff(void) { return FUR_CUTOFF; }

/* flow [B][2][H][W], mask [B][576][H][W] -> out [B][2][8H][8W] */
int fur_upsample(const float *flow, const float *mask, int32_t B, int32_t H, int32_t W, float mask_scale, int32_t variant, float *out) {
    if (!flow || !mask || !out || B < 1 || H < 1 || W < 1 || variant < 0 || variant > 2) {
        return -1;
    }
    const int degree = variant == 2 ? 3 : 7;
    const int64_t HW = (int64_t)H * W;
    for (int64_t b = 0; b < B; ++b) {
        for (int64_t y = 0; y < H; ++y) {
            for (int64_t x = 0; x < W; ++x) {
                float f[2][9]; /* step 5: 8 * flow of the padded 3 x 3 neighbourhood */
                for (int k = 0; k < 9; ++k) {
                    const int dy = (variant == 1 ? k % 3 : k / 3) - 1, dx = (variant == 1 ? k / 3 : k % 3) - 1;
                    const int64_t yy = y + dy, xx = x + dx;
                    const int inside = yy >= 0 && yy < H && xx >= 0 && xx < W;
                    for (int c = 0; c < 2; ++c) {
                        f[c][k] = inside ? 8.0f * flow[(b * 2 + c) * HW + yy * W + xx] : 0.0f;
                    }
                }
                for (int i = 0; i < 8; ++i) {
                    for (int j = 0; j < 8; ++j) {
                        float xs[9], e[9];
                        for (int k = 0; k < 9; ++k) { /* step 1 */
                            xs[k] = mask[(b * 576 + k * 64 + i * 8 + j) * HW + y * W + x] * mask_scale;
                        }
                        float m = xs[0]; /* step 2 */
                        for (int k = 1; k < 9; ++k) {
                            if (xs[k] > m) {
                                m = xs[k];
                            }
                        }
                        for (int k = 0; k < 9; ++k) { /* step 3 */
                            e[k] = exp_c_degree(xs[k] - m, degree);
                        }
                        float s = e[0] + e[1]; /* step 4 */
                        for (int k = 2; k < 9; ++k) {
                            s = s + e[k];
                        }
                        for (int c = 0; c < 2; ++c) { /* step 6 */
                            float acc = 0.0f;
                            for (int k = 0; k < 9; ++k) {
                                const float p = f[c][k] * (e[k] / s);
                                acc = k == 0 ? p : acc + p;
                            }
                            out[((b * 2 + c) * 8 * H + 8 * y + i) * 8 * W + 8 * x + j] = acc;
                        }
                    }
                }
            }
        }
    }
    return 0;
}
