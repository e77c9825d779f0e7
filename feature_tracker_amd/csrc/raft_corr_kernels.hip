// raft_corr_kernels.hip — RAFT's all-pairs correlation pyramid and its windowed lookup
// (CorrelationPyramid, src/nn_optical_flow_tracker/raft/correlation_volumes.py:3-83) on gfx950.
//
// Three kernels:
//   corr_build_kernel   level 0 = f0^T f1 / sqrt(C) per batch item on the f32-input matrix cores (v_mfma_f32_32x32x2_f32), one
//                       wave per 32 (p) x 128 (q) tile whose q range is an 8 x 16 block of the second image, so the epilogue
//                       also emits pooled levels 1..3 of that block from the rounded level-0 values it holds (cross-lane sums,
//                       no re-read of level 0).
//   corr_pool_kernel    level l from level l - 1 for the levels the build's epilogue does not reach (l >= 4).
//   corr_lookup_kernel  every level's (2r+1)^2 bilinear window per pixel, one thread per (pixel, level, window row), written
//                       straight into [B, L*K, H, W] (or the reference's per-level [B, H, W, K]).
// Level 0 is an fmaf chain over the channels in ascending order from +0, then one correctly rounded division; a pooled value is
// (((a00 + a01) + a10) + a11) / 4; the sampler is torch CPU grid_sample's arithmetic as DESIGN.md 5.10 writes it out.  With -ffp-contract=off the results are
// bit-identical to the scalar restatement (tests/raft_corr_ref.c).  Every index is 64-bit; coordinates are compared as floats
// before any conversion to int, so NaN / inf / huge coordinates never address memory.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ftk_device.h"

namespace ftk {
namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int kTileRows = 8;   // q block: 8 rows x 16 columns of the second image = 4 MFMA column tiles of 2 rows x 16
constexpr int kTileCols = 16;
constexpr int kWavesPerGroup = 4;  // 4 waves share one q block (their B fragments hit in L1), each has its own 32 p

// One wave: rows p0 .. p0 + 31 of the volume (pixels of the first image) against the 8 x 16 q block (ty, tx) of the second.
__global__ __launch_bounds__(64 * kWavesPerGroup) void corr_build_kernel(CorrBuildParams prm) {
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int b = blockIdx.z;
    const int H = prm.H, W = prm.W, C = prm.C;
    const int64_t HW = (int64_t)H * W;
    const int64_t p0 = ((int64_t)blockIdx.x * kWavesPerGroup + wave) * 32;
    if (p0 >= HW) {
        return;
    }
    const int tiles_x = (W + kTileCols - 1) / kTileCols;
    const int ty = blockIdx.y / tiles_x, tx = blockIdx.y % tiles_x;
    const int j = lane & 31;  // column of the 32 x 32 tile (q); row of the A fragment (p)
    const int kh = lane >> 5;  // which of the two channels of a k-step this lane feeds
    // A operand: f0[b][c][p0 + j]; B operand of column tile t: f1[b][c][q_t(j)], q_t(j) = (8 ty + 2 t + j / 16) * W + 16 tx + j % 16.
    // Out-of-range p / q read a valid pixel (0) and are never stored.
    const int64_t pa = (p0 + j < HW) ? p0 + j : 0;
    int64_t qb[4];
    bool qok[4];
    const int qx = tx * kTileCols + (j & 15);
    for (int t = 0; t < 4; ++t) {
        const int qy = ty * kTileRows + 2 * t + (j >> 4);
        qok[t] = qy < H && qx < W;
        qb[t] = qok[t] ? (int64_t)qy * W + qx : 0;
    }
    const float *f0 = prm.f0 + (int64_t)b * C * HW;
    const float *f1 = prm.f1 + (int64_t)b * C * HW;
    f32x16 acc[4];
    for (int t = 0; t < 4; ++t) {
        for (int r = 0; r < 16; ++r) {
            acc[t][r] = 0.0f;
        }
    }
    // k-step s covers channels 2s (lanes 0-31) and 2s + 1 (lanes 32-63).  The MFMA adds them to the accumulator in that order, one
    // rounding per product (an fmaf chain).  An odd C pads the last step with (-0) * (+0) = -0, which leaves every accumulator
    // exactly as it is (x + -0 = x, -0 included).
    const int steps = (C + 1) >> 1;
    auto load = [&](int s, float &a, float (&bv)[4]) {
        const int c = 2 * s + kh;
        if (c < C) {
            const int64_t row = (int64_t)c * HW;
            a = f0[row + pa];
            for (int t = 0; t < 4; ++t) {
                bv[t] = f1[row + qb[t]];
            }
        } else {
            a = -0.0f;
            for (int t = 0; t < 4; ++t) {
                bv[t] = 0.0f;
            }
        }
    };
    float a_cur, b_cur[4];
    load(0, a_cur, b_cur);
    for (int s = 0; s < steps; ++s) {
        float a_nxt = 0.0f, b_nxt[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        if (s + 1 < steps) {
            load(s + 1, a_nxt, b_nxt);
        }
        for (int t = 0; t < 4; ++t) {
            acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a_cur, b_cur[t], acc[t], 0, 0, 0);
        }
        a_cur = a_nxt;
        for (int t = 0; t < 4; ++t) {
            b_cur[t] = b_nxt[t];
        }
    }
    // Epilogue.  Accumulator register r of column tile t holds (p, q) with p = p0 + (r & 3) + 8 (r >> 2) + 4 (lane >> 5) and
    // q = q_t(j).  Level 0 is stored; levels 1..fused are pooled across lanes: in a column tile, lane j's x / y neighbours are lanes
    // j ^ 1 / j ^ 16; level-1 rows 2u, 2u + 1 of the block come from tiles 2u, 2u + 1 (same lane), x neighbours at j ^ 2; level-2
    // rows 0 / 1 from the two halves, x neighbours at j ^ 4.
    const float d = prm.divisor;
    float *vol = prm.volume;
    const int64_t hw1 = prm.level_h[1] * (int64_t)prm.level_w[1];
    const int64_t hw2 = prm.level_h[2] * (int64_t)prm.level_w[2];
    const int64_t hw3 = prm.level_h[3] * (int64_t)prm.level_w[3];
    for (int r = 0; r < 16; ++r) {
        const int64_t p = p0 + (r & 3) + 8 * (r >> 2) + 4 * kh;
        const bool pok = p < HW;
        const int64_t slab = (int64_t)b * HW + p;
        float v[4];
        for (int t = 0; t < 4; ++t) {
            v[t] = acc[t][r] / d;
            if (pok && qok[t]) {
                vol[slab * HW + qb[t]] = v[t];
            }
        }
        if (prm.fused < 1) {
            continue;
        }
        float s1[4];
        for (int t = 0; t < 4; ++t) {
            const float x01 = __shfl_xor(v[t], 1), x10 = __shfl_xor(v[t], 16), x11 = __shfl_xor(v[t], 17);
            s1[t] = (((v[t] + x01) + x10) + x11) / 4.0f;
            const int y1 = ty * (kTileRows / 2) + t, x1 = tx * (kTileCols / 2) + ((j & 15) >> 1);
            if (pok && (j & 17) == 0 && y1 < prm.level_h[1] && x1 < prm.level_w[1]) {
                vol[prm.level_offset[1] + slab * hw1 + (int64_t)y1 * prm.level_w[1] + x1] = s1[t];
            }
        }
        if (prm.fused < 2) {
            continue;
        }
        float s2[2];
        for (int u = 0; u < 2; ++u) {
            const float a01 = __shfl_xor(s1[2 * u], 2), a11 = __shfl_xor(s1[2 * u + 1], 2);
            s2[u] = (((s1[2 * u] + a01) + s1[2 * u + 1]) + a11) / 4.0f;
            const int y2 = ty * (kTileRows / 4) + u, x2 = tx * (kTileCols / 4) + ((j & 15) >> 2);
            if (pok && (j & 19) == 0 && y2 < prm.level_h[2] && x2 < prm.level_w[2]) {
                vol[prm.level_offset[2] + slab * hw2 + (int64_t)y2 * prm.level_w[2] + x2] = s2[u];
            }
        }
        if (prm.fused < 3) {
            continue;
        }
        const float b01 = __shfl_xor(s2[0], 4), b11 = __shfl_xor(s2[1], 4);
        const float s3 = (((s2[0] + b01) + s2[1]) + b11) / 4.0f;
        const int y3 = ty, x3 = tx * (kTileCols / 8) + ((j & 15) >> 3);
        if (pok && (j & 23) == 0 && y3 < prm.level_h[3] && x3 < prm.level_w[3]) {
            vol[prm.level_offset[3] + slab * hw3 + (int64_t)y3 * prm.level_w[3] + x3] = s3;
        }
    }
}

// level `level` from level - 1: one thread per output value
__global__ void corr_pool_kernel(const float *src, float *dst, int64_t slabs, int hin, int win, int hout, int wout) {
    const int64_t per = (int64_t)hout * wout;
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= slabs * per) {
        return;
    }
    const int64_t n = idx / per;
    const int rem = (int)(idx - n * per);
    const int y = rem / wout, x = rem % wout;
    const float *s = src + n * ((int64_t)hin * win) + (int64_t)(2 * y) * win + 2 * x;
    dst[idx] = (((s[0] + s[1]) + s[win]) + s[win + 1]) / 4.0f;
}

__device__ __forceinline__ float corner(const float *slab, int h, int w, float fy, float fx) {
    // fy / fx are integral floats (or NaN / inf): compared as floats, converted only when inside the level
    if (fy >= 0.0f && fy < (float)h && fx >= 0.0f && fx < (float)w) {
        return slab[(int64_t)(int)fy * w + (int)fx];
    }
    return 0.0f;
}

// One thread per (pixel, level, window row i): the 2r + 1 samples j of that row.  Lanes run along the pixels, so every store
// of the channels-first layout is coalesced.
__global__ void corr_lookup_kernel(CorrLookupParams prm) {
    const int64_t HW = (int64_t)prm.H * prm.W;
    const int64_t pix = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (pix >= HW) {
        return;
    }
    const int b = blockIdx.z;
    const int side = 2 * prm.radius + 1;
    const int K = side * side;
    const int level = blockIdx.y / side, i = blockIdx.y % side;
    const int h = prm.level_h[level], w = prm.level_w[level];
    const float *slab = prm.volume + prm.level_offset[level] + ((int64_t)b * HW + pix) * ((int64_t)h * w);
    const float x = prm.coords[((int64_t)b * 2) * HW + pix];
    const float y = prm.coords[((int64_t)b * 2 + 1) * HW + pix];
    const float scale = (float)(1 << level);
    // correlation_volumes.py:7-9 (normalise) and grid_sample(align_corners=True)'s unnormalise
    const float hx = (float)(w - 1) / 2.0f, hy = (float)(h - 1) / 2.0f;
    const float cy = y / scale + (float)(i - prm.radius);
    const float gy = 2.0f * cy / (float)(h - 1) - 1.0f;
    const float iy = (gy + 1.0f) * hy;
    const float y_n = floorf(iy);
    const float n = iy - y_n, s = 1.0f - n;
    for (int jj = 0; jj < side; ++jj) {
        const float cx = x / scale + (float)(jj - prm.radius);
        const float gx = 2.0f * cx / (float)(w - 1) - 1.0f;
        const float ix = (gx + 1.0f) * hx;
        const float x_w = floorf(ix);
        const float we = ix - x_w, e = 1.0f - we;
        const float nw = s * e, ne = s * we, sw = n * e, se = n * we;
        const float v_nw = corner(slab, h, w, y_n, x_w), v_ne = corner(slab, h, w, y_n, x_w + 1.0f);
        const float v_sw = corner(slab, h, w, y_n + 1.0f, x_w), v_se = corner(slab, h, w, y_n + 1.0f, x_w + 1.0f);
        const float out = fmaf(v_se, se, fmaf(v_sw, sw, fmaf(v_ne, ne, v_nw * nw)));
        const int ch = i * side + jj;
        if (prm.per_level) {
            // level l's [B, H, W, K] block at l * B * H * W * K
            prm.out[(int64_t)level * prm.B * HW * K + ((int64_t)b * HW + pix) * K + ch] = out;
        } else {
            prm.out[((int64_t)b * prm.levels * K + (int64_t)level * K + ch) * HW + pix] = out;
        }
    }
}

}  // namespace

int corr_fused_levels() { return 3; }

hipError_t corr_build_launch(const CorrBuildParams &p, hipStream_t stream) {
    const int64_t HW = (int64_t)p.H * p.W;
    const int64_t pgroups = (HW + 32 * kWavesPerGroup - 1) / (32 * kWavesPerGroup);
    const int64_t qtiles = (int64_t)((p.H + kTileRows - 1) / kTileRows) * ((p.W + kTileCols - 1) / kTileCols);
    if (pgroups > 0x7fffffff || qtiles > 65535 || p.B > 65535) {
        return hipErrorInvalidValue;
    }
    hipLaunchKernelGGL(corr_build_kernel, dim3((unsigned)pgroups, (unsigned)qtiles, (unsigned)p.B), dim3(64 * kWavesPerGroup), 0, stream, p);
    return hipGetLastError();
}

hipError_t corr_pool_launch(const float *src, float *dst, int64_t slabs, int hin, int win, int hout, int wout, hipStream_t stream) {
    const int64_t total = slabs * hout * wout;
    const int64_t blocks = (total + 255) / 256;
    if (blocks > 0x7fffffff) {
        return hipErrorInvalidValue;
    }
    hipLaunchKernelGGL(corr_pool_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, src, dst, slabs, hin, win, hout, wout);
    return hipGetLastError();
}

hipError_t corr_lookup_launch(const CorrLookupParams &p, hipStream_t stream) {
    const int64_t HW = (int64_t)p.H * p.W;
    const int64_t rows = (int64_t)p.levels * (2 * p.radius + 1);
    if ((HW + 255) / 256 > 0x7fffffff || rows > 65535 || p.B > 65535) {
        return hipErrorInvalidValue;
    }
    hipLaunchKernelGGL(corr_lookup_kernel, dim3((unsigned)((HW + 255) / 256), (unsigned)rows, (unsigned)p.B), dim3(256), 0, stream, p);
    return hipGetLastError();
}

}  // namespace ftk
