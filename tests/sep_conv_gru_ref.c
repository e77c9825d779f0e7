/* sep_conv_gru_ref.c — scalar CPU restatement of RAFT's separable ConvGRU (SepConvGru.forward,
 * src/nn_optical_flow_tracker/raft/gru.py:59-76) as DESIGN.md 5.13 states it.  TEST INFRASTRUCTURE ONLY: independent code, it includes
 * nothing from feature_tracker_amd/ and nothing there may use it.  Compile with -ffp-contract=off: every operation below is one
 * correctly rounded float32 operation, the fused ones are written as fmaf.
 *
 * `variant` is a test-only argument: 0 the contract, and five mutants that the float64 comparison of tests/test_sep_conv_gru_cpu.py
 * must reject: 1 taps reversed (tap t reads the pixel shifted by pad - t); 2 the z and r weights and biases exchanged; 3 the vertical
 * pass first; 4 z and 1 - z exchanged in the blend; 5 a tap outside the image reads the clamped edge pixel instead of +0. */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#define SCG_CUTOFF (-87.0f)
#define SCG_LOG2E 0x1.715476p+0f
#define SCG_LN2_HI 0x1.62e4p-1f
#define SCG_LN2_LO 0x1.7f7d1cp-20f
/* tanh_c: below this |v| the odd polynomial, from it on the exp_c form */
#define SCG_TANH_SMALL 0.25f

/* exp_c of DESIGN.md 5.12 (its own copy of the sequence in tests/flow_upsample_ref.c), t <= 0 or NaN */
static float exp_c(float t) {
    if (t != t) {
        return t;
    }
    if (t < SCG_CUTOFF) {
        return 0.0f;
    }
    const float n = rintf(t * SCG_LOG2E);
    float r = fmaf(n, -SCG_LN2_HI, t);
    r = fmaf(n, -SCG_LN2_LO, r);
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

/* sigmoid_c: e = exp_c(-|v|), d = 1 + e; 1 / d for v >= 0, e / d otherwise (NaN takes the second branch and stays NaN) */
static float sigmoid_c(float v) {
    const float e = exp_c(-fabsf(v));
    const float d = 1.0f + e;
    return v >= 0.0f ? 1.0f / d : e / d;
}

/* tanh_c: |v| < 0.25: a + a * (s * P(s)) with a = |v|, s = v * v, P the Taylor coefficients of tanh(x) / x - 1 up to x^10, Horner in
 * fmaf; otherwise (1 - e) / (1 + e) with e = exp_c(-2 |v|); either way the sign of v restored (so tanh_c(-0) = -0). */
static float tanh_c(float v) {
    const float a = fabsf(v);
    if (a < SCG_TANH_SMALL) {
        const float s = v * v;
        float p = -0x1.226e36p-7f;       /* -1382 / 155925 */
        p = fmaf(p, s, 0x1.664f48p-6f);  /*    62 / 2835 */
        p = fmaf(p, s, -0x1.ba1ba2p-5f); /*   -17 / 315 */
        p = fmaf(p, s, 0x1.111112p-3f);  /*     2 / 15 */
        p = fmaf(p, s, -0x1.555556p-2f); /*    -1 / 3 */
        return copysignf(fmaf(a, s * p, a), v);
    }
    const float e = exp_c(-2.0f * a);
    const float t = (1.0f - e) / (1.0f + e);
    return copysignf(t, v);
}

float scg_sigmoid_c(float v) { return sigmoid_c(v); }
float scg_tanh_c(float v) { return tanh_c(v); }
float scg_tanh_small(void) { return SCG_TANH_SMALL; }

void scg_sigmoid_c_array(const float *v, int64_t count, float *out) {
    for (int64_t q = 0; q < count; ++q) {
        out[q] = sigmoid_c(v[q]);
    }
}

void scg_tanh_c_array(const float *v, int64_t count, float *out) {
    for (int64_t q = 0; q < count; ++q) {
        out[q] = tanh_c(v[q]);
    }
}

typedef struct {
    const float *const *parts; /* n_parts tensors [B][part_channels[i]][H][W], then `last` [B][Ch][H][W] */
    const int32_t *part_channels;
    int32_t n_parts;
    const float *last;
    int32_t Ch, B, H, W;
} scg_input;

/* channel c of the concatenation at batch item b: a pointer to its H x W plane */
static const float *plane(const scg_input *in, int64_t b, int32_t c) {
    const int64_t HW = (int64_t)in->H * in->W;
    for (int32_t i = 0; i < in->n_parts; ++i) {
        if (c < in->part_channels[i]) {
            return in->parts[i] + (b * in->part_channels[i] + c) * HW;
        }
        c -= in->part_channels[i];
    }
    return in->last + (b * in->Ch + c) * HW;
}

/* the contract's chain at one output channel and pixel: bias, then fmaf over k = c * ks + t ascending */
static float chain(const scg_input *in, int32_t Cin, int32_t ks, int vertical, int variant, const float *w, float bias, int64_t b, int32_t y, int32_t x) {
    const int32_t pad = ks / 2, H = in->H, W = in->W;
    float acc = bias;
    for (int32_t c = 0; c < Cin; ++c) {
        const float *p = plane(in, b, c);
        for (int32_t t = 0; t < ks; ++t) {
            const int32_t shift = variant == 1 ? pad - t : t - pad;
            int32_t yy = vertical ? y + shift : y, xx = vertical ? x : x + shift;
            float v;
            if (yy >= 0 && yy < H && xx >= 0 && xx < W) {
                v = p[(int64_t)yy * W + xx];
            } else if (variant == 5) {
                yy = yy < 0 ? 0 : (yy >= H ? H - 1 : yy);
                xx = xx < 0 ? 0 : (xx >= W ? W - 1 : xx);
                v = p[(int64_t)yy * W + xx];
            } else {
                v = 0.0f;
            }
            acc = fmaf(w[(int64_t)c * ks + t], v, acc);
        }
    }
    return acc;
}

/* one pass: h [B][Ch][H][W] -> out; z and rh are scratch of the same size */
static void pass(const float *const *parts, const int32_t *part_channels, int32_t n_parts, int32_t Cx, int32_t Ch, int32_t ks, int32_t B, int32_t H,
                 int32_t W, int vertical, int variant, const float *wz, const float *bz, const float *wr, const float *br, const float *wq,
                 const float *bq, const float *h, float *z, float *rh, float *out) {
    const int32_t Cin = Cx + Ch;
    const int64_t HW = (int64_t)H * W, K = (int64_t)Cin * ks;
    scg_input in = {parts, part_channels, n_parts, h, Ch, B, H, W};
    if (variant == 2) {
        const float *tw = wz, *tb = bz;
        wz = wr, bz = br, wr = tw, br = tb;
    }
    for (int64_t b = 0; b < B; ++b) {
        for (int32_t co = 0; co < Ch; ++co) {
            for (int32_t y = 0; y < H; ++y) {
                for (int32_t x = 0; x < W; ++x) {
                    const int64_t o = (b * Ch + co) * HW + (int64_t)y * W + x;
                    z[o] = sigmoid_c(chain(&in, Cin, ks, vertical, variant, wz + co * K, bz[co], b, y, x));
                    const float r = sigmoid_c(chain(&in, Cin, ks, vertical, variant, wr + co * K, br[co], b, y, x));
                    rh[o] = r * h[o];
                }
            }
        }
    }
    in.last = rh;
    for (int64_t b = 0; b < B; ++b) {
        for (int32_t co = 0; co < Ch; ++co) {
            for (int32_t y = 0; y < H; ++y) {
                for (int32_t x = 0; x < W; ++x) {
                    const int64_t o = (b * Ch + co) * HW + (int64_t)y * W + x;
                    const float q = tanh_c(chain(&in, Cin, ks, vertical, variant, wq + co * K, bq[co], b, y, x));
                    const float zz = variant == 4 ? 1.0f - z[o] : z[o];
                    const float a = 1.0f - zz;
                    const float u = a * h[o];
                    const float v = zz * q;
                    out[o] = u + v;
                }
            }
        }
    }
}

/* weights / biases: z, r, q of the horizontal pass, then z, r, q of the vertical pass; each weight [Ch][Cx + Ch][ks] */
int scg_forward(const float *const *parts, const int32_t *part_channels, int32_t n_parts, const float *h, const float *const *weights,
                const float *const *biases, int32_t Ch, int32_t ks, int32_t B, int32_t H, int32_t W, int32_t variant, float *out) {
    if (!parts || !part_channels || n_parts < 1 || !h || !weights || !biases || !out || Ch < 1 || (ks != 3 && ks != 5) || B < 1 || H < 1 || W < 1 ||
        variant < 0 || variant > 5) {
        return -1;
    }
    int32_t Cx = 0;
    for (int32_t i = 0; i < n_parts; ++i) {
        if (part_channels[i] < 1) {
            return -1;
        }
        Cx += part_channels[i];
    }
    const size_t n = (size_t)B * Ch * H * W;
    float *z = malloc(n * sizeof(float)), *rh = malloc(n * sizeof(float)), *mid = malloc(n * sizeof(float));
    if (!z || !rh || !mid) {
        free(z), free(rh), free(mid);
        return -2;
    }
    const int first = variant == 3 ? 1 : 0; /* 0: horizontal first (the contract) */
    for (int step = 0; step < 2; ++step) {
        const int vertical = step == 0 ? first : 1 - first;
        const int g = 3 * vertical;
        pass(parts, part_channels, n_parts, Cx, Ch, ks, B, H, W, vertical, variant, weights[g], biases[g], weights[g + 1], biases[g + 1], weights[g + 2],
             biases[g + 2], step == 0 ? h : mid, z, rh, step == 0 ? mid : out);
    }
    free(z), free(rh), free(mid);
    return 0;
}
