// raft_corr_ondemand_kernels.hip — RAFT's correlation lookups without the all-pairs volume (OnDemandCorrelation) on gfx950.
//
// Three kernels:
//   corr_od_transpose_kernel  fmap0 and fmap1 [B][C][H * W] -> [B][H * W][C] (fmap1's is its level 0), through a 32 x 32 LDS tile so that
//                             reads and writes are both along the fast axis.
//   corr_od_pool_kernel       fmap1's level l from level l - 1, channel-last, (((a00 + a01) + a10) + a11) / 4, one thread per value.
//   corr_od_lookup_kernel     one wave per (query pixel, level).  The wave first evaluates the correlation at the (2r+2)^2 integer lattice
//                             under its window, one lattice point per lane: the serial fmaf chain over the channels in ascending order from
//                             +0 of fmap0[b, c, p] * fmap1_l[b, c, y2, x2], divided by (float)sqrt((double)C); the point's C values are one
//                             contiguous row (16-byte loads), fmap0's are the same for every lane.  No cross-lane reduction: the chain order
//                             is the definition's.  Then one lane per window sample runs tests/raft_corr_ref.c::rcr_sample's arithmetic and
//                             takes its four corners from the lattice.
// Every sample goes through its own normalise / unnormalise round trip, so floor(ix) at offset dj + 1 is not always floor(ix) at dj plus
// one: a corner can fall outside the lattice.  corner() therefore never assumes it is inside: a corner inside the level but outside the
// lattice is evaluated directly by the lane that needs it (the same chain: the correlation at a position is a pure function of
// (b, p, l, y2, x2)).  Windows wider than the lattice LDS holds (radius > 7) evaluate every corner that way.  Coordinates are compared as
// floats before any conversion to int, so NaN / inf / huge coordinates never address memory; every index is 64-bit.
// With -ffp-contract=off the results are bit-identical to the scalar restatement (tests/raft_corr_ondemand_ref.c).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ftk_device.h"
#include "raft_corr_ondemand_plan.h"

namespace ftk {
namespace {

// z = map * B + b; x / y: the tile of 32 pixels / 32 channels
__global__ __launch_bounds__(kCorrOdTile * 8) void corr_od_transpose_kernel(CorrOdTransposeParams prm) {
    __shared__ float tile[kCorrOdTile][kCorrOdTile + 1];
    const int map = blockIdx.z / prm.B, b = blockIdx.z % prm.B;
    const float *in = (map == 0 ? prm.f0 : prm.f1) + (int64_t)b * prm.C * prm.HW;
    float *out = (map == 0 ? prm.out0 : prm.out1) + (int64_t)b * prm.C * prm.HW;
    const int64_t p0 = (int64_t)blockIdx.x * kCorrOdTile;
    const int c0 = blockIdx.y * kCorrOdTile;
    const int tx = threadIdx.x, ty = threadIdx.y;
    for (int k = 0; k < kCorrOdTile; k += 8) {
        const int c = c0 + ty + k;
        const int64_t p = p0 + tx;
        if (c < prm.C && p < prm.HW) {
            tile[ty + k][tx] = in[(int64_t)c * prm.HW + p];
        }
    }
    __syncthreads();
    for (int k = 0; k < kCorrOdTile; k += 8) {
        const int64_t p = p0 + ty + k;
        const int c = c0 + tx;
        if (p < prm.HW && c < prm.C) {
            out[p * prm.C + c] = tile[tx][ty + k];
        }
    }
}

// one thread per output value, the channel fastest
__global__ __launch_bounds__(kCorrOdPoolBlock) void corr_od_pool_kernel(CorrOdPoolParams prm) {
    const int hout = prm.hin / 2, wout = prm.win / 2;
    const int64_t C = prm.C;
    const int64_t total = (int64_t)prm.B * hout * wout * C;
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= total) {
        return;
    }
    const int64_t c = idx % C;
    const int64_t pos = idx / C;  // (b * hout + y) * wout + x
    const int64_t x = pos % wout;
    const int64_t by = pos / wout;
    const int64_t y = by % hout, b = by / hout;
    const float *s = prm.src + (((b * prm.hin + 2 * y) * prm.win) + 2 * x) * C + c;
    const int64_t down = (int64_t)prm.win * C;
    prm.dst[idx] = (((s[0] + s[C]) + s[down]) + s[down + C]) / 4.0f;
}

// the definition: the fmaf chain over c = 0, 1, ... from +0 of a[c] * row[c], then the division
template <bool kVector>
__device__ __forceinline__ float corr_at(const float *a, const float *row, int C, float divisor) {
    float acc = 0.0f;
    if (kVector) {
        const float4 *a4 = reinterpret_cast<const float4 *>(a);
        const float4 *r4 = reinterpret_cast<const float4 *>(row);
        for (int k = 0; k < C / 4; ++k) {
            const float4 u = a4[k], v = r4[k];
            acc = fmaf(u.x, v.x, acc);
            acc = fmaf(u.y, v.y, acc);
            acc = fmaf(u.z, v.z, acc);
            acc = fmaf(u.w, v.w, acc);
        }
    } else {
        for (int c = 0; c < C; ++c) {
            acc = fmaf(a[c], row[c], acc);
        }
    }
    return acc / divisor;
}

// What a wave knows about its lattice: rows y0 .. y0 + side - 1, columns x0 .. x0 + side - 1 of the level, in `values` (LDS)
struct Lattice {
    const float *values;
    int y0, x0, side;  // side 0: there is none
};

template <bool kVector>
__device__ __forceinline__ float corner(const Lattice &lat, const float *a, const float *level, int h, int w, int C, float divisor, float fy, float fx) {
    // fy / fx are integral floats (or NaN / inf): compared as floats, converted only when inside the level
    if (fy >= 0.0f && fy < (float)h && fx >= 0.0f && fx < (float)w) {
        const int yi = (int)fy, xi = (int)fx;
        const int u = yi - lat.y0, v = xi - lat.x0;  // both operands within (-side, h) / (-side, w): no overflow
        if (u >= 0 && u < lat.side && v >= 0 && v < lat.side) {
            return lat.values[u * lat.side + v];
        }
        return corr_at<kVector>(a, level + ((int64_t)yi * w + xi) * C, C, divisor);  // outside the lattice: never assumed away
    }
    return 0.0f;
}

template <bool kVector>
__device__ __forceinline__ void lookup_body(const CorrOdLookupParams &prm, float *lattice_values) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int64_t HW = (int64_t)prm.H * prm.W;
    const int64_t pix = (int64_t)blockIdx.x * kCorrOdWaves + wave;
    const bool active = pix < HW;  // wave-uniform; an inactive wave only keeps the barrier company
    const int level = blockIdx.y, b = blockIdx.z;
    const int h = prm.level_h[level], w = prm.level_w[level];
    const int C = prm.C, r = prm.radius, side = 2 * r + 1;
    const float *a = prm.workspace + ((int64_t)b * HW + (active ? pix : 0)) * C;
    const float *lvl = prm.workspace + prm.level_offset[level] + (int64_t)b * h * w * C;
    const float x = active ? prm.coords[((int64_t)b * 2) * HW + pix] : 0.0f;
    const float y = active ? prm.coords[((int64_t)b * 2 + 1) * HW + pix] : 0.0f;
    const float scale = (float)(1 << level);
    float *mine = lattice_values + wave * kCorrOdLatticeFloats;
    Lattice lat{mine, 0, 0, 0};
    if (prm.lattice_side > 0) {
        // the lattice starts at the north-west corner of the window's first sample (di = dj = -r); ix and iy grow with the offset
        const float cx = x / scale + (float)(-r), cy = y / scale + (float)(-r);
        const float gx = 2.0f * cx / (float)(w - 1) - 1.0f, gy = 2.0f * cy / (float)(h - 1) - 1.0f;
        const float ix = (gx + 1.0f) * ((float)(w - 1) / 2.0f), iy = (gy + 1.0f) * ((float)(h - 1) / 2.0f);
        const float x0f = floorf(ix), y0f = floorf(iy);
        const int S = prm.lattice_side;
        // a lattice that does not meet the level (or whose origin is NaN / inf / huge) is not built: every corner is then outside the level
        // or is evaluated directly
        if (active && y0f > -(float)S && y0f < (float)h && x0f > -(float)S && x0f < (float)w) {
            lat.y0 = (int)y0f;
            lat.x0 = (int)x0f;
            lat.side = S;
            for (int pt = lane; pt < S * S; pt += 64) {
                const int64_t yi = (int64_t)lat.y0 + pt / S, xi = (int64_t)lat.x0 + pt % S;
                float v = 0.0f;  // outside the level: never read through corner(), which checks the level first
                if (yi >= 0 && yi < h && xi >= 0 && xi < w) {
                    v = corr_at<kVector>(a, lvl + (yi * w + xi) * C, C, prm.divisor);
                }
                mine[pt] = v;
            }
        }
        __syncthreads();  // the lattice is read by other lanes than wrote it
    }
    if (!active) {
        return;
    }
    const int K = side * side;
    for (int smp = lane; smp < K; smp += 64) {
        const int i = smp / side, j = smp % side;
        const int di = i - r, dj = j - r;
        // tests/raft_corr_ref.c::rcr_sample, operation for operation
        const float cx = x / scale + (float)dj, cy = y / scale + (float)di;
        const float gx = 2.0f * cx / (float)(w - 1) - 1.0f, gy = 2.0f * cy / (float)(h - 1) - 1.0f;
        const float ix = (gx + 1.0f) * ((float)(w - 1) / 2.0f), iy = (gy + 1.0f) * ((float)(h - 1) / 2.0f);
        const float x_w = floorf(ix), y_n = floorf(iy);
        const float we = ix - x_w, e = 1.0f - we, n = iy - y_n, s = 1.0f - n;
        const float nw = s * e, ne = s * we, sw = n * e, se = n * we;
        const float v_nw = corner<kVector>(lat, a, lvl, h, w, C, prm.divisor, y_n, x_w);
        const float v_ne = corner<kVector>(lat, a, lvl, h, w, C, prm.divisor, y_n, x_w + 1.0f);
        const float v_sw = corner<kVector>(lat, a, lvl, h, w, C, prm.divisor, y_n + 1.0f, x_w);
        const float v_se = corner<kVector>(lat, a, lvl, h, w, C, prm.divisor, y_n + 1.0f, x_w + 1.0f);
        const float out = fmaf(v_se, se, fmaf(v_sw, sw, fmaf(v_ne, ne, v_nw * nw)));
        if (prm.per_level) {
            // level l's [B, H, W, K] block at l * B * H * W * K
            prm.out[(int64_t)level * prm.B * HW * K + ((int64_t)b * HW + pix) * K + smp] = out;
        } else {
            prm.out[((int64_t)b * prm.levels * K + (int64_t)level * K + smp) * HW + pix] = out;
        }
    }
}

__global__ __launch_bounds__(64 * kCorrOdWaves) void corr_od_lookup_kernel(CorrOdLookupParams prm) {
    __shared__ float lattice_values[kCorrOdWaves * kCorrOdLatticeFloats];
    if (prm.vector) {
        lookup_body<true>(prm, lattice_values);
    } else {
        lookup_body<false>(prm, lattice_values);
    }
}

}  // namespace

hipError_t corr_od_transpose_launch(const CorrOdTransposeParams &p, dim3 grid, dim3 block, hipStream_t stream) {
    hipLaunchKernelGGL(corr_od_transpose_kernel, grid, block, 0, stream, p);
    return hipGetLastError();
}

hipError_t corr_od_pool_launch(const CorrOdPoolParams &p, int64_t blocks, hipStream_t stream) {
    if (blocks < 1 || blocks > 0x7fffffff) {
        return hipErrorInvalidValue;
    }
    hipLaunchKernelGGL(corr_od_pool_kernel, dim3((unsigned)blocks), dim3(kCorrOdPoolBlock), 0, stream, p);
    return hipGetLastError();
}

hipError_t corr_od_lookup_launch(const CorrOdLookupParams &p, dim3 grid, dim3 block, hipStream_t stream) {
    if (p.lattice_side > kCorrOdMaxLatticeSide) {
        return hipErrorInvalidValue;
    }
    hipLaunchKernelGGL(corr_od_lookup_kernel, grid, block, 0, stream, p);
    return hipGetLastError();
}

}  // namespace ftk
