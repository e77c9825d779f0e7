/* raft_encoder_ref.c — scalar CPU restatement of the layers of RAFT's encoders (src/nn_optical_flow_tracker/raft/encoder.py:4-68) and of
 * the image normalisation of model.py:70-71, as DESIGN.md 5.15 states them, next to raft_conv_ref.c (compiled together with this file, and
 * with sep_conv_gru_ref.c; tests/raft_encoder_ref.py composes the networks from these pieces and from the other restatements).
 * TEST INFRASTRUCTURE ONLY: independent code, it includes nothing from feature_tracker_amd/ and nothing there may use it.
 * Compile with -ffp-contract=off: every operation below is one correctly rounded float32 operation, the fused ones are written as fmaf.
 *
 * Normalisation: n = 2.0f * (x / 255.0f) - 1.0f, image pixels only: the padding of the layer that reads the image is +0 AFTER it.
 * BatchNorm in eval mode, folded: s = gamma / sqrtf(var + eps); w'[co][k] = w[co][k] * s; b' = beta - mean * s.
 * One layer: acc = b'[co]; for k = (c * ks + ty) * ks + tx ascending acc = fmaf(w'[co][k], in[c][S y + ty - pad][S x + tx - pad], acc), a tap
 * outside the image a multiplied +0; the output is ceil(H / S) x ceil(W / S).  Then v = acc + res[co][y][x] where a residual is given, then
 * v = (v < 0) ? +0 : v if relu (a NaN and -0 pass), then out = scale * v.
 *
 * `variant` is a test-only argument: 0 the contract, and the mutants that the float64 comparison of tests/test_raft_encoder_cpu.py must
 * reject (the others are made by tests/raft_encoder_ref.py from these pieces): re_conv2d: 1 the stride tap at S y + ty without - pad;
 * 5 the residual added after the ReLU; 8 the padding normalised with the image (-1 instead of +0).  re_fold: 3 var + eps without the
 * square root; 4 eps dropped. */
#include <math.h>
#include <stdint.h>

/* tests/raft_conv_ref.c */
int rc_conv2d(const float *const *parts, const int32_t *part_channels, int32_t n_parts, const float *weight, const float *bias, int32_t Cout, int32_t ks,
              int32_t relu, float scale, int32_t B, int32_t H, int32_t W, int32_t variant, float *out);

float re_normalise(float x) {
    const float q = x / 255.0f;
    return 2.0f * q - 1.0f; /* the doubling is exact: one rounded division, one rounded subtraction */
}

int re_fold(const float *w, const float *gamma, const float *beta, const float *mean, const float *var, float eps, int32_t Cout, int64_t K,
            int32_t variant, float *w_out, float *b_out) {
    if (!w || !gamma || !beta || !mean || !var || !w_out || !b_out || Cout < 1 || K < 1) {
        return -1;
    }
    for (int32_t co = 0; co < Cout; ++co) {
        const float shifted = variant == 4 ? var[co] : var[co] + eps;
        const float s = gamma[co] / (variant == 3 ? shifted : sqrtf(shifted));
        for (int64_t k = 0; k < K; ++k) {
            w_out[co * K + k] = w[co * K + k] * s;
        }
        const float ms = mean[co] * s;
        b_out[co] = beta[co] - ms;
    }
    return 0;
}

/* in: [B][Cin][H][W]; out and res (may be NULL): [B][Cout][ceil(H / S)][ceil(W / S)].  With stride 1, no residual, no normalisation and
 * variant 0 this is rc_conv2d over one part, and is computed by it. */
int re_conv2d(const float *in, int32_t Cin, const float *weight, const float *bias, int32_t Cout, int32_t ks, int32_t stride, const float *res,
              int32_t relu, float scale, int32_t normalise, int32_t B, int32_t H, int32_t W, int32_t variant, float *out) {
    if (!in || !weight || !bias || !out || Cin < 1 || Cout < 1 || (ks != 1 && ks != 3 && ks != 7) || (stride != 1 && stride != 2) || B < 1 || H < 1 ||
        W < 1) {
        return -1;
    }
    if (stride == 1 && !res && !normalise && variant == 0) {
        const float *parts[] = {in};
        const int32_t channels[] = {Cin};
        return rc_conv2d(parts, channels, 1, weight, bias, Cout, ks, relu, scale, B, H, W, 0, out);
    }
    const int32_t pad = ks / 2, tap_pad = (variant == 1 && stride == 2) ? 0 : pad;
    const int32_t OH = (H + stride - 1) / stride, OW = (W + stride - 1) / stride;
    const int64_t HW = (int64_t)H * W, OHW = (int64_t)OH * OW, K = (int64_t)Cin * ks * ks;
    const float outside = (variant == 8 && normalise) ? re_normalise(0.0f) : 0.0f;
    for (int64_t b = 0; b < B; ++b) {
        for (int32_t co = 0; co < Cout; ++co) {
            const float *w = weight + co * K;
            for (int32_t y = 0; y < OH; ++y) {
                for (int32_t x = 0; x < OW; ++x) {
                    float acc = bias[co];
                    for (int32_t c = 0; c < Cin; ++c) {
                        const float *p = in + (b * Cin + c) * HW;
                        for (int32_t ty = 0; ty < ks; ++ty) {
                            for (int32_t tx = 0; tx < ks; ++tx) {
                                const int32_t yy = stride * y + ty - tap_pad, xx = stride * x + tx - tap_pad;
                                float v = outside;
                                if (yy >= 0 && yy < H && xx >= 0 && xx < W) {
                                    v = p[(int64_t)yy * W + xx];
                                    if (normalise) {
                                        v = re_normalise(v);
                                    }
                                }
                                acc = fmaf(w[((int64_t)c * ks + ty) * ks + tx], v, acc);
                            }
                        }
                    }
                    const int64_t o = (b * Cout + co) * OHW + (int64_t)y * OW + x;
                    float v = acc;
                    if (res && variant != 5) {
                        v = acc + res[o];
                    }
                    if (relu) {
                        v = (v < 0.0f) ? 0.0f : v;
                    }
                    if (res && variant == 5) {
                        v = v + res[o];
                    }
                    out[o] = scale * v;
                }
            }
        }
    }
    return 0;
}
