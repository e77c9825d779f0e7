/* raft_corr_ondemand_ref.c — scalar CPU restatement of RAFT's on-demand correlation, the yardstick of
 * raft_corr_ondemand_kernels.hip.  No correlation value is stored between samples and nothing is shared: fmap1 is pooled level by level
 * with (((a00 + a01) + a10) + a11) / 4 (floor halves, chained); for a query pixel p and a level, the correlation with every position of
 * the pooled map is tests/raft_corr_ref.c::rcr_row's level-0 rule applied to that map (an fmaf chain over the channels in ascending order
 * from +0, divided by (float)sqrt((double)C)) into a per-pixel row; every window sample then takes its four corners from that row by
 * rcr_sample's arithmetic, positions outside the level giving 0.  Feature maps stay channel-first as the caller has them: no lattice,
 * no transposed layout.  Compiled with -ffp-contract=off: every float operation is the one written. */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>

/* fmap [n planes][hin][win] -> [n planes][hin / 2][win / 2] */
void rco_pool(const float *src, int64_t n, int32_t hin, int32_t win, float *dst) {
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

/* the correlation of query pixel p (of f0, [B][C][HW]) with every position of a level of fmap1 (f1l, [B][C][hw]): row[0 .. hw) */
void rco_row(const float *f0, const float *f1l, int32_t C, int64_t HW, int64_t hw, int32_t b, int64_t p, float *row) {
    const float d = (float)sqrt((double)C);
    const float *a = f0 + (int64_t)b * C * HW;
    const float *bb = f1l + (int64_t)b * C * hw;
    /* channel-outer so the q loop vectorises; each row[q] is still the chain c = 0, 1, ... from +0 */
    for (int64_t q = 0; q < hw; ++q) {
        row[q] = 0.0f;
    }
    for (int32_t c = 0; c < C; ++c) {
        const float ac = a[(int64_t)c * HW + p];
        const float *bc = bb + (int64_t)c * hw;
        for (int64_t q = 0; q < hw; ++q) {
            row[q] = fmaf(ac, bc[q], row[q]);
        }
    }
    for (int64_t q = 0; q < hw; ++q) {
        row[q] = row[q] / d;
    }
}

static float corner(const float *slab, int32_t h, int32_t w, float fy, float fx) {
    if (fy >= 0.0f && fy < (float)h && fx >= 0.0f && fx < (float)w) {
        return slab[(int64_t)(int32_t)fy * w + (int32_t)fx];
    }
    return 0.0f;
}

/* one sample of a level (the per-pixel row as a slab h x w) at window offset (di, dj) around (x, y) / 2^level: rcr_sample */
float rco_sample(const float *slab, int32_t h, int32_t w, int32_t level, float x, float y, int32_t di, int32_t dj) {
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

/* floor(ix) of the sampler above for n coordinates x at offset dj in a level of width w: the x half of rco_sample's coordinate lines.
 * The lattice-trap search of tests/test_raft_corr_ondemand_cpu.py reads it. */
void rco_floor_ix(int32_t w, int32_t level, const float *xs, int64_t n, int32_t dj, float *out) {
    const float scale = (float)(1 << level);
    for (int64_t k = 0; k < n; ++k) {
        const float x = xs[k];
        const float cx = x / scale + (float)dj;
        const float gx = 2.0f * cx / (float)(w - 1) - 1.0f;
        const float ix = (gx + 1.0f) * ((float)(w - 1) / 2.0f);
        out[k] = floorf(ix);
    }
}

/* out: [B][levels * K][H][W], K = (2r + 1)^2, channel l * K + i * (2r + 1) + j at offset (i - r, j - r); -1 when a level would be empty */
int32_t rco_lookup(const float *f0, const float *f1, int32_t B, int32_t C, int32_t H, int32_t W, int32_t levels, int32_t r, const float *coords,
                   float *out) {
    if (levels < 1 || levels > 64 || r < 0 || B < 1 || C < 1 || H < 1 || W < 1) {
        return -1;
    }
    int32_t lh[64], lw[64];
    float *maps[64];
    int32_t h = H, w = W;
    for (int32_t l = 0; l < levels; ++l) {
        if (h == 0 || w == 0) {
            return -1;
        }
        lh[l] = h;
        lw[l] = w;
        h /= 2;
        w /= 2;
    }
    const int64_t HW = (int64_t)H * W;
    maps[0] = (float *)f1;
    for (int32_t l = 1; l < levels; ++l) {
        maps[l] = (float *)malloc(sizeof(float) * (size_t)((int64_t)B * C * lh[l] * lw[l]));
        rco_pool(maps[l - 1], (int64_t)B * C, lh[l - 1], lw[l - 1], maps[l]);
    }
    float *row = (float *)malloc(sizeof(float) * (size_t)HW);
    const int32_t side = 2 * r + 1, K = side * side;
    for (int32_t b = 0; b < B; ++b) {
        for (int64_t p = 0; p < HW; ++p) {
            const float x = coords[(int64_t)b * 2 * HW + p], y = coords[((int64_t)b * 2 + 1) * HW + p];
            for (int32_t l = 0; l < levels; ++l) {
                rco_row(f0, maps[l], C, HW, (int64_t)lh[l] * lw[l], b, p, row);
                for (int32_t i = 0; i < side; ++i) {
                    for (int32_t j = 0; j < side; ++j) {
                        out[((int64_t)b * levels * K + (int64_t)l * K + i * side + j) * HW + p] = rco_sample(row, lh[l], lw[l], l, x, y, i - r, j - r);
                    }
                }
            }
        }
    }
    free(row);
    for (int32_t l = 1; l < levels; ++l) {
        free(maps[l]);
    }
    return 0;
}
