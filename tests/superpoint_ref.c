/* superpoint_ref.c — scalar CPU restatement of what SuperPoint's forward pass adds to the conv layer of tests/raft_conv_ref.c (compiled
 * together with this file), as DESIGN.md 5.25 states it: the 2 x 2 max-pool in the layer's epilogue and the channel-wise L2 normalisation of
 * the dense descriptor map with its change of layout.  TEST INFRASTRUCTURE ONLY: independent code, it includes nothing from
 * feature_tracker_amd/ and nothing there may use it.  Compile with -ffp-contract=off: every operation is one correctly rounded float32
 * operation, the fused one is written as fmaf.
 *
 * The pool: out[oy][ox] over the window rows 2 oy, 2 oy + 1 and columns 2 ox, 2 ox + 1 of v (the layer's value after its ReLU), for oy <
 * H / 2, ox < W / 2 (a last odd row or column is dropped): pick(m, x) = (x > m || x != x) ? x : m, out = pick(pick(v00, v01), pick(v10,
 * v11)): a NaN propagates, and among equal maxima (+0 and -0 are equal) the first in the order (0,0), (0,1), (1,0), (1,1) wins.
 *
 * The normalisation: x [D][cells] to y [cells][D]; n2 = fmaf(x_c, x_c, n2) over ascending c from +0, den = fmaxf(sqrtf(n2), 1e-12f), y_c =
 * x_c / den.
 *
 * `variant` is a test-only argument: 0 the contract; 1 the pooling window shifted by one pixel (rows 2 oy + 1, 2 oy + 2, columns likewise,
 * clamped to the image); 2 the pool as fmaxf of the four (a NaN is dropped, the sign of a zero is fmaxf's); 3 the normalisation without
 * the 1e-12 floor (a zero cell becomes 0 / 0).  (4, the two heads' halves exchanged, lives in the composition of tests/superpoint_ref.py.) */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>

/* tests/raft_conv_ref.c */
int rc_conv2d(const float *const *parts, const int32_t *part_channels, int32_t n_parts, const float *weight, const float *bias, int32_t Cout, int32_t ks,
              int32_t relu, float scale, int32_t B, int32_t H, int32_t W, int32_t variant, float *out);

static float pick(float m, float x) { return (x > m || x != x) ? x : m; }

/* planes [n][H][W] to [n][H / 2][W / 2] */
int sp_max_pool(const float *in, int64_t planes, int32_t H, int32_t W, int32_t variant, float *out) {
    if (!in || !out || planes < 1 || H < 2 || W < 2 || variant < 0 || variant > 4) {
        return -1;
    }
    const int32_t PH = H / 2, PW = W / 2;
    for (int64_t n = 0; n < planes; ++n) {
        const float *p = in + n * (int64_t)H * W;
        float *q = out + n * (int64_t)PH * PW;
        for (int32_t oy = 0; oy < PH; ++oy) {
            for (int32_t ox = 0; ox < PW; ++ox) {
                int32_t y0 = 2 * oy, y1 = 2 * oy + 1, x0 = 2 * ox, x1 = 2 * ox + 1;
                if (variant == 1) {
                    y0 += 1, x0 += 1;
                    y1 = y1 + 1 < H ? y1 + 1 : H - 1;
                    x1 = x1 + 1 < W ? x1 + 1 : W - 1;
                }
                const float v00 = p[(int64_t)y0 * W + x0], v01 = p[(int64_t)y0 * W + x1], v10 = p[(int64_t)y1 * W + x0], v11 = p[(int64_t)y1 * W + x1];
                q[(int64_t)oy * PW + ox] = variant == 2 ? fmaxf(fmaxf(v00, v01), fmaxf(v10, v11)) : pick(pick(v00, v01), pick(v10, v11));
            }
        }
    }
    return 0;
}

/* the layer of rc_conv2d (no scale) and the pool after it; *pre (may be NULL) receives the tensor before the pool, [B][Cout][H][W] */
int sp_conv2d_pool(const float *const *parts, const int32_t *part_channels, int32_t n_parts, const float *weight, const float *bias, int32_t Cout, int32_t ks,
                   int32_t relu, int32_t B, int32_t H, int32_t W, int32_t variant, float *pre, float *out) {
    if (!out || B < 1 || Cout < 1 || H < 2 || W < 2 || (ks != 1 && ks != 3)) {
        return -1;
    }
    float *tmp = pre ? pre : (float *)malloc(sizeof(float) * (size_t)B * Cout * H * W);
    if (!tmp) {
        return -2;
    }
    int rc = rc_conv2d(parts, part_channels, n_parts, weight, bias, Cout, ks, relu, 1.0f, B, H, W, 0, tmp);
    if (rc == 0) {
        rc = sp_max_pool(tmp, (int64_t)B * Cout, H, W, variant, out);
    }
    if (!pre) {
        free(tmp);
    }
    return rc;
}

int sp_channel_normalise(const float *x, int32_t D, int64_t cells, int32_t variant, float *y) {
    if (!x || !y || D < 1 || cells < 1 || variant < 0 || variant > 4) {
        return -1;
    }
    for (int64_t i = 0; i < cells; ++i) {
        float n2 = 0.0f;
        for (int32_t c = 0; c < D; ++c) {
            const float v = x[c * cells + i];
            n2 = fmaf(v, v, n2);
        }
        const float den = variant == 3 ? sqrtf(n2) : fmaxf(sqrtf(n2), 1e-12f);
        for (int32_t c = 0; c < D; ++c) {
            y[i * D + c] = x[c * cells + i] / den;
        }
    }
    return 0;
}
