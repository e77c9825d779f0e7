/* raft_corr_ref.c — scalar CPU restatement of RAFT's CorrelationPyramid (correlation_volumes.py:3-83), the yardstick of
 * raft_corr_kernels.hip.  It implements DESIGN.md 5.10 literally: level 0 an fmaf chain over the channels in ascending order from
 * +0 divided by (float)sqrt((double)C); level l the 2x2 pool (((a00 + a01) + a10) + a11) / 4 of level l - 1; the lookup the
 * normalise (:7-9) / unnormalise (grid_sample, align_corners=True) / zero-padded bilinear sampler written out there.
 * Compiled with -ffp-contract=off: every float operation is the one written.  Volume layout as ftk_corr_pyramid_layout. */
#include <math.h>
#include <stdint.h>

static int32_t level_dims(int32_t H, int32_t W, int32_t levels, int64_t B, int64_t *off, int32_t *lh, int32_t *lw) {
    int64_t total = 0;
    int32_t h = H, w = W;
    for (int32_t l = 0; l < levels; ++l) {
        if (h == 0 || w == 0) {
            return -1;
        }
        off[l] = total;
        lh[l] = h;
        lw[l] = w;
        total += B * H * W * (int64_t)h * w;
        h /= 2;
        w /= 2;
    }
    return 0;
}

/* one level-0 row: corr0[b][p][0 .. H*W) */
void rcr_row(const float *f0, const float *f1, int32_t C, int32_t H, int32_t W, int32_t b, int64_t p, float *row) {
    const int64_t HW = (int64_t)H * W;
    const float d = (float)sqrt((double)C);
    const float *a = f0 + (int64_t)b * C * HW;
    const float *bb = f1 + (int64_t)b * C * HW;
    /* channel-outer so the q loop vectorises; each row[q] is still the chain c = 0, 1, ... from +0 */
    for (int64_t q = 0; q < HW; ++q) {
        row[q] = 0.0f;
    }
    for (int32_t c = 0; c < C; ++c) {
        const float ac = a[(int64_t)c * HW + p];
        const float *bc = bb + (int64_t)c * HW;
        for (int64_t q = 0; q < HW; ++q) {
            row[q] = fmaf(ac, bc[q], row[q]);
        }
    }
    for (int64_t q = 0; q < HW; ++q) {
        row[q] = row[q] / d;
    }
}

/* n slabs of hin x win -> hout x wout (floor halves) */
void rcr_pool(const float *src, int64_t n, int32_t hin, int32_t win, float *dst) {
    const int32_t hout = hin / 2, wout = win / 2;
    for (int64_t k = 0; k < n; ++k) {
        const float *s = src + k * hin * (int64_t)win;
        float *o = dst + k * hout * (int64_t)wout;
        for (int32_t y = 0; y < hout; ++y) {
            for (int32_t x = 0; x < wout; ++x) {
                const float *t = s + (int64_t)(2 * y) * win + 2 * x;
                o[(int64_t)y * wout + x] = (((t[0] + t[1]) + t[win]) + t[win + 1]) / 4.0f;
            }
        }
    }
}

/* the whole pyramid; returns -1 when a level would be empty */
int32_t rcr_build(const float *f0, const float *f1, int32_t B, int32_t C, int32_t H, int32_t W, int32_t levels, float *vol) {
    int64_t off[64];
    int32_t lh[64], lw[64];
    if (levels < 1 || levels > 64 || level_dims(H, W, levels, B, off, lh, lw) != 0) {
        return -1;
    }
    const int64_t HW = (int64_t)H * W;
    for (int32_t b = 0; b < B; ++b) {
        for (int64_t p = 0; p < HW; ++p) {
            rcr_row(f0, f1, C, H, W, b, p, vol + ((int64_t)b * HW + p) * HW);
        }
    }
    for (int32_t l = 1; l < levels; ++l) {
        rcr_pool(vol + off[l - 1], (int64_t)B * HW, lh[l - 1], lw[l - 1], vol + off[l]);
    }
    return 0;
}

static float corner(const float *slab, int32_t h, int32_t w, float fy, float fx) {
    if (fy >= 0.0f && fy < (float)h && fx >= 0.0f && fx < (float)w) {
        return slab[(int64_t)(int32_t)fy * w + (int32_t)fx];
    }
    return 0.0f;
}

/* one sample of a level (slab h x w) at window offset (di, dj) around (x, y) / 2^level */
float rcr_sample(const float *slab, int32_t h, int32_t w, int32_t level, float x, float y, int32_t di, int32_t dj) {
    const float scale = (float)(1 << level);
    const float cx = x / scale + (float)dj, cy = y / scale + (float)di;
    const float gx = 2.0f * cx / (float)(w - 1) - 1.0f, gy = 2.0f * cy / (float)(h - 1) - 1.0f;
    const float ix = (gx + 1.0f) * ((float)(w - 1) / 2.0f), iy = (gy + 1.0f) * ((float)(h - 1) / 2.0f);
    const float x_w = floorf(ix), y_n = floorf(iy);
    const float we = ix - x_w, e = 1.0f - we, n = iy - y_n, s = 1.0f - n;
    const float nw = s * e, ne = s * we, sw = n * e, se = n * we;
    const float v_nw = corner(slab, h, w, y_n, x_w), v_ne = corner(slab, h, w, y_n, x_w + 1.0f);
    const float v_sw = corner(slab, h, w, y_n + 1.0f, x_w), v_se = corner(slab, h, w, y_n + 1.0f, x_w + 1.0f);
    return fmaf(v_se, se, fmaf(v_sw, sw, fmaf(v_ne, ne, v_nw * nw)));
}

/* out: [B][levels * K][H][W], K = (2r + 1)^2, channel l * K + i * (2r + 1) + j at offset (i - r, j - r) */
int32_t rcr_lookup(const float *vol, int32_t B, int32_t H, int32_t W, int32_t levels, int32_t r, const float *coords, float *out) {
    int64_t off[64];
    int32_t lh[64], lw[64];
    if (levels < 1 || levels > 64 || r < 0 || level_dims(H, W, levels, B, off, lh, lw) != 0) {
        return -1;
    }
    const int64_t HW = (int64_t)H * W;
    const int32_t side = 2 * r + 1, K = side * side;
    for (int32_t b = 0; b < B; ++b) {
        for (int64_t p = 0; p < HW; ++p) {
            const float x = coords[(int64_t)b * 2 * HW + p], y = coords[((int64_t)b * 2 + 1) * HW + p];
            for (int32_t l = 0; l < levels; ++l) {
                const float *slab = vol + off[l] + ((int64_t)b * HW + p) * lh[l] * (int64_t)lw[l];
                for (int32_t i = 0; i < side; ++i) {
                    for (int32_t j = 0; j < side; ++j) {
                        out[((int64_t)b * levels * K + (int64_t)l * K + i * side + j) * HW + p] = rcr_sample(slab, lh[l], lw[l], l, x, y, i - r, j - r);
                    }
                }
            }
        }
    }
    return 0;
}
