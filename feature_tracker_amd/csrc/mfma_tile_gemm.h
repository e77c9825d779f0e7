// mfma_tile_gemm.h — the device functions MatchAssignment's and the transformer layer's kernels share (match_assignment_kernels.hip,
// transformer_kernels.hip): the wave-level GEMM tile on v_mfma_f32_32x32x2_f32 whose result is a k-ordered fmaf
// chain, the count clamp, and the maximum and the xor rounds of 5.23 step 3.  Every float operation is written out; the library is compiled with
// -ffp-contract=off.
#pragma once

#include "ftk_device.h"
#include "raft_math.h"

namespace ftk {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int kColTiles = 4;  // 32-column MFMA tiles of a wave's GEMM tile: 128 columns

// One wave's 32 x 128 tile: acc[t][r] += sum over c ascending of a[c] b_t[c], where this lane's `a` is row (lane & 31) of the 32 and
// `b[t]` column 32 t + (lane & 31) of the 128, both as rows of `dim` floats.  Afterwards acc[t][r] belongs to row
// (r & 3) + 8 (r >> 2) + 4 (lane >> 5) and column 32 t + (lane & 31).  k-step s feeds channel 2 s from lanes 0-31 and 2 s + 1 from lanes
// 32-63; the matrix core adds them in that order with one rounding per product.  An odd dim pads the last step with (-0) * (+0) = -0,
// which leaves every accumulator as it is.
template <bool kVec>
__device__ __forceinline__ void tile_gemm(const float *a, const float *(&b)[kColTiles], int dim, float scale, int kh, f32x16 (&acc)[kColTiles]) {
    if (kVec) {
        const int chunks = dim >> 2;
        const float4 *a4 = reinterpret_cast<const float4 *>(a);
        const float4 *b4[kColTiles];
#pragma unroll
        for (int t = 0; t < kColTiles; ++t) {
            b4[t] = reinterpret_cast<const float4 *>(b[t]);
        }
        float4 a_cur = a4[0], b_cur[kColTiles];
#pragma unroll
        for (int t = 0; t < kColTiles; ++t) {
            b_cur[t] = b4[t][0];
        }
        for (int u = 0; u < chunks; ++u) {
            float4 a_nxt = a_cur, b_nxt[kColTiles];
            const int un = u + 1 < chunks ? u + 1 : u;
            a_nxt = a4[un];
#pragma unroll
            for (int t = 0; t < kColTiles; ++t) {
                b_nxt[t] = b4[t][un];
            }
            const float a0 = __fmul_rn(kh ? a_cur.y : a_cur.x, scale), a1 = __fmul_rn(kh ? a_cur.w : a_cur.z, scale);
#pragma unroll
            for (int t = 0; t < kColTiles; ++t) {
                acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, __fmul_rn(kh ? b_cur[t].y : b_cur[t].x, scale), acc[t], 0, 0, 0);
            }
#pragma unroll
            for (int t = 0; t < kColTiles; ++t) {
                acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, __fmul_rn(kh ? b_cur[t].w : b_cur[t].z, scale), acc[t], 0, 0, 0);
            }
            a_cur = a_nxt;
#pragma unroll
            for (int t = 0; t < kColTiles; ++t) {
                b_cur[t] = b_nxt[t];
            }
        }
    } else {
        const int steps = (dim + 1) >> 1;
        for (int s = 0; s < steps; ++s) {
            const int c = 2 * s + kh;
            const bool in = c < dim;
            const float av = in ? __fmul_rn(a[c], scale) : -0.0f;
#pragma unroll
            for (int t = 0; t < kColTiles; ++t) {
                const float bv = in ? __fmul_rn(b[t][c], scale) : 0.0f;
                acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv, acc[t], 0, 0, 0);
            }
        }
    }
}

__device__ __forceinline__ int valid_count(const int32_t *count, int extent) {
    return count ? min(max(count[0], 0), extent) : extent;
}

// m of 5.23 step 3 from the first valid entry and the greatest entry that is no NaN: the scan `m = x_0; if (x > m) m = x` ends at x_0
// when that is NaN and at the greatest comparable entry otherwise (which of two zeros it ends at changes no later bit).
__device__ __forceinline__ float scan_maximum(float first, float greatest) { return first != first ? first : greatest; }

// The xor rounds of 5.23 step 3 from lane distance kFrom down to kTo: the greatest comparable value, and the sum p[l] + p[l ^ off] round
// by round.  With 32 .. 1 every lane ends with the value of all 64; with 16 .. 1 each half of the wave with its own 32.
template <int kFrom = 32, int kTo = 1>
__device__ __forceinline__ float xor_greatest(float v) {
#pragma unroll
    for (int off = kFrom; off >= kTo; off >>= 1) {
        const float o = __shfl_xor(v, off);
        if (o > v) {
            v = o;
        }
    }
    return v;
}

template <int kFrom = 32, int kTo = 1>
__device__ __forceinline__ float xor_sum(float v) {
#pragma unroll
    for (int off = kFrom; off >= kTo; off >>= 1) {
        v = __fadd_rn(v, __shfl_xor(v, off));
    }
    return v;
}

}  // namespace ftk
