// keypoint_decode_kernels.hip — the two ends of the keypoint decoder on gfx950 (KeypointDecoder): from a SuperPoint-style
// network's head tensors to what the matchers read, with no copy to the host.
//
//  * keypoint_score_kernel: the softmax over each cell's 65 logits and the depth-to-space shuffle, straight into the key plane that
//    5.19's suppression and selection read (score bits << 32 | ~pixel index).  One lane per cell, one wave per tile of 64 cells along a
//    cell row: every logit plane is read as 64 consecutive floats.  The 64 scores of every cell of the tile pass through LDS, so that keys
//    (and the optional heatmap) leave as whole fine rows of 512 pixels.
//  * keypoint_describe_kernel: one wave per output row; the bilinear sample of the coarse descriptor map at the keypoint (cell-centre
//    alignment, weights exact multiples of 1/64) and its L2 normalisation, lanes owning channels l, l + 64, ...; the squared norm is
//    summed per lane and then over six cross-lane rounds.  A wave whose row lies behind the device-side count writes zeros.
//
// Between them run the window-maximum, blocking, collect and rank launches of masked Harris detection (feature_kernels.hip
// key_plane_select_launch, track_table_kernels.hip harris_rank_launch), unchanged: they are generic over the key plane.
#include "keypoint_decode_plan.h"
#include "raft_math.h"

namespace ftk {
namespace {

// (feature_kernels.hip's sortable_bits: the order of the unsigned values is the order of the floats)
__device__ __forceinline__ unsigned keypoint_sortable_bits(float v) {
    const unsigned u = __float_as_uint(v);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__global__ void __launch_bounds__(kKeypointScoreTile) keypoint_score_kernel(const KeypointScoreParams p) {
    __shared__ float tile[64 * kKeypointScoreStride];  // [logit k][cell of the tile], rows padded (keypoint_decode_plan.h)
    const int lane = threadIdx.x;
    const int cy = blockIdx.y, cx0 = blockIdx.x * kKeypointScoreTile;
    // a lane behind the row's last cell computes that cell again; what it computes never leaves LDS
    const int cx = min(cx0 + lane, p.cell_cols - 1);
    const size_t plane = (size_t)p.cell_rows * p.cell_cols;
    const float *x = p.semi + (size_t)cy * p.cell_cols + cx;
    float v[kKeypointLogits];
#pragma unroll
    for (int k = 0; k < kKeypointLogits; ++k) {
        v[k] = x[k * plane];
    }
    float m = v[0];
#pragma unroll
    for (int k = 1; k < kKeypointLogits; ++k) {
        if (v[k] > m) {
            m = v[k];
        }
    }
#pragma unroll
    for (int k = 0; k < kKeypointLogits; ++k) {
        v[k] = exp_c(__fsub_rn(v[k], m));
    }
    float sum = v[0];
#pragma unroll
    for (int k = 1; k < kKeypointLogits; ++k) {
        sum = __fadd_rn(sum, v[k]);
    }
#pragma unroll
    for (int k = 0; k < 64; ++k) {
        tile[k * kKeypointScoreStride + lane] = __fdiv_rn(v[k], sum);
    }
    __syncthreads();
    const int rows = p.cell_rows * kKeypointCell, cols = p.cell_cols * kKeypointCell;
    const int px0 = cx0 * kKeypointCell;
    const int sub = lane & 7, cell = lane >> 3;  // pixel lane of a fine row: column `sub` of cell j * 8 + `cell` of the tile
    for (int fy = 0; fy < kKeypointCell; ++fy) {
        const int y = cy * kKeypointCell + fy;
        const bool row_inside = y >= p.border && y < rows - p.border;
        const float *src = tile + (fy * kKeypointCell + sub) * kKeypointScoreStride + cell;
#pragma unroll
        for (int j = 0; j < kKeypointCell; ++j) {
            const int xpix = px0 + j * 64 + lane;
            if (xpix < cols) {
                const float s = src[j * 8];
                const size_t i = (size_t)y * cols + xpix;
                unsigned long long key = 0ull;
                if (s > p.min_score && row_inside && xpix >= p.border && xpix < cols - p.border) {
                    key = ((unsigned long long)keypoint_sortable_bits(s) << 32) | (unsigned long long)(0xFFFFFFFFu - (unsigned)i);
                }
                p.key[i] = key;
                if (p.heatmap) {
                    p.heatmap[i] = s;
                }
            }
        }
    }
}

__global__ void __launch_bounds__(64 * kKeypointDescribeWaves) keypoint_describe_kernel(const KeypointDescribeParams p) {
    const int lane = threadIdx.x & 63;
    const int r = blockIdx.x * kKeypointDescribeWaves + (threadIdx.x >> 6);  // wave-uniform, as everything derived from it
    if (r >= p.max_keypoints) {
        return;
    }
    float *out = p.descriptors + (size_t)r * p.channels;
    if (r >= p.count[0]) {
        for (int c = lane; c < p.channels; c += 64) {
            out[c] = 0.0f;
        }
        return;
    }
    const float2 uv = reinterpret_cast<const float2 *>(p.uv)[r];
    const float xc = fminf(fmaxf(__fmul_rn(__fsub_rn(uv.x, 3.5f), 0.125f), 0.0f), (float)(p.cell_cols - 1));
    const float yc = fminf(fmaxf(__fmul_rn(__fsub_rn(uv.y, 3.5f), 0.125f), 0.0f), (float)(p.cell_rows - 1));
    const int x0 = (int)xc, y0 = (int)yc;
    const int x1 = min(x0 + 1, p.cell_cols - 1), y1 = min(y0 + 1, p.cell_rows - 1);
    const float fx = __fsub_rn(xc, (float)x0), fy = __fsub_rn(yc, (float)y0);
    const float gx = __fsub_rn(1.0f, fx), gy = __fsub_rn(1.0f, fy);
    const float w00 = __fmul_rn(gx, gy), w01 = __fmul_rn(fx, gy), w10 = __fmul_rn(gx, fy), w11 = __fmul_rn(fx, fy);
    const float *d00 = p.desc + y0 * p.stride_y + x0 * p.stride_x;
    const float *d01 = p.desc + y0 * p.stride_y + x1 * p.stride_x;
    const float *d10 = p.desc + y1 * p.stride_y + x0 * p.stride_x;
    const float *d11 = p.desc + y1 * p.stride_y + x1 * p.stride_x;
    float v[kKeypointLaneChannels];
    float n2 = 0.0f;
#pragma unroll
    for (int i = 0; i < kKeypointLaneChannels; ++i) {
        const int c = lane + 64 * i;
        v[i] = 0.0f;
        if (c < p.channels) {
            const long long at = c * p.stride_c;
            const float top = __fadd_rn(__fmul_rn(w00, d00[at]), __fmul_rn(w01, d01[at]));
            v[i] = __fadd_rn(__fadd_rn(top, __fmul_rn(w10, d10[at])), __fmul_rn(w11, d11[at]));
            n2 = fmaf(v[i], v[i], n2);
        }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        n2 = __fadd_rn(n2, __shfl_xor(n2, off));
    }
    const float den = fmaxf(sqrtf(n2), 1e-12f);  // (correctly rounded by the build's flags; __fsqrt_rn is the native one)
#pragma unroll
    for (int i = 0; i < kKeypointLaneChannels; ++i) {
        const int c = lane + 64 * i;
        if (c < p.channels) {
            out[c] = __fdiv_rn(v[i], den);
        }
    }
}

}  // namespace

hipError_t keypoint_decode_launch(const KeypointDecodePlan &plan, const KeypointDecodeParams &p, hipStream_t stream) {
    const size_t k = (size_t)p.rank.max_count;
    hipError_t e = hipMemsetAsync(p.rank.uv_out, 0, sizeof(float) * 2 * k, stream);  // the zeros behind the rows
    if (e != hipSuccess) {
        return e;
    }
    e = hipMemsetAsync(p.rank.score_out, 0, sizeof(float) * k, stream);
    if (e != hipSuccess) {
        return e;
    }
    hipLaunchKernelGGL(keypoint_score_kernel, dim3(plan.score_grid_x, plan.score_grid_y), dim3(kKeypointScoreTile), 0, stream, p.score);
    e = key_plane_select_launch(p.select, p.occupied, stream);
    if (e != hipSuccess) {
        return e;
    }
    e = harris_rank_launch(plan.rank_blocks, p.rank, stream);
    if (e != hipSuccess) {
        return e;
    }
    hipLaunchKernelGGL(keypoint_describe_kernel, dim3(plan.describe_blocks), dim3(64 * kKeypointDescribeWaves), 0, stream, p.describe);
    return hipGetLastError();
}

}  // namespace ftk
