// superpoint_kernels.hip — what SuperPoint's forward pass needs besides conv2d_kernel (raft_conv_kernels.hip, whose pooled form is its
// max-pool): channel_normalise_kernel, the L2 normalisation of the dense descriptor map over its channels with the change of layout
// KeypointDecoder reads fastest.
//
// x is [D][cells] (cells = Hc * Wc, the network's layout), y is [cells][D].  Per cell: n2 = fmaf(x_c, x_c, n2) over ascending c from +0,
// den = fmaxf(sqrtf(n2), 1e-12f), y_c = x_c / den: torch.nn.functional.normalize(dim = 1) with one stated summation order; the square
// root and the division are correctly rounded (the library's build flags).  fmaxf is C's: a NaN n2 gives den = 1e-12f.
//
// A workgroup of 4 waves owns 64 consecutive cells.  Wave 0 runs the 64 chains, lane = cell: a load of one channel is 64 consecutive
// floats, the loads do not depend on the chain, only the fmaf does.  Then, per 64 channels, the four waves read the tile [64 c][64
// cells] with the cell lane-fast (coalesced along the cells; mostly L2 hits, wave 0 has just read them), put it into LDS with a row
// pitch of 65 floats (a column read is then conflict-free) and write it with the channel lane-fast: 64 consecutive floats of one cell's
// row of y per wave store.  Every index is 64-bit; no address depends on the data.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ftk_device.h"

namespace ftk {
namespace {

constexpr int kNormCells = 64;     // cells of a workgroup
constexpr int kNormChannels = 64;  // channels of a transposed tile
constexpr int kNormThreads = 256;

__global__ __launch_bounds__(kNormThreads) void channel_normalise_kernel(const float *__restrict__ x, float *__restrict__ y, int D, int64_t cells) {
    __shared__ float s_tile[kNormChannels][kNormCells + 1];
    __shared__ float s_den[kNormCells];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t cell0 = (int64_t)blockIdx.x * kNormCells;
    if (wave == 0) {
        const int64_t cell = cell0 + lane;
        float n2 = 0.0f;
        if (cell < cells) {
            for (int c = 0; c < D; ++c) {
                const float v = x[(int64_t)c * cells + cell];
                n2 = fmaf(v, v, n2);
            }
        }
        s_den[lane] = fmaxf(__fsqrt_rn(n2), 1e-12f);
    }
    for (int c0 = 0; c0 < D; c0 += kNormChannels) {
        __syncthreads();  // s_den is written; the tile of the round before is read
#pragma unroll
        for (int i = 0; i < kNormChannels / 4; ++i) {
            const int c = c0 + wave + 4 * i;
            const int64_t cell = cell0 + lane;
            s_tile[wave + 4 * i][lane] = (c < D && cell < cells) ? x[(int64_t)c * cells + cell] : 0.0f;
        }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < kNormCells / 4; ++i) {
            const int k = wave + 4 * i;  // the cell of this wave's store, lane = channel
            const int64_t cell = cell0 + k;
            const int c = c0 + lane;
            if (cell < cells && c < D) {
                y[cell * D + c] = __fdiv_rn(s_tile[lane][k], s_den[k]);
            }
        }
    }
}

}  // namespace

hipError_t channel_normalise_launch(const float *x, float *y, int32_t D, int64_t cells, hipStream_t stream) {
    const int64_t groups = (cells + kNormCells - 1) / kNormCells;
    if (D < 1 || cells < 1 || groups > 0x7fffffff) {
        return hipErrorInvalidValue;
    }
    hipLaunchKernelGGL(channel_normalise_kernel, dim3((unsigned)groups), dim3(kNormThreads), 0, stream, x, y, D, cells);
    return hipGetLastError();
}

}  // namespace ftk
