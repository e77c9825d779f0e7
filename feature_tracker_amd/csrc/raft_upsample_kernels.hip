// raft_upsample_kernels.hip — RAFT's convex flow upsampling (Raft.UpsampleFlow, src/nn_optical_flow_tracker/raft/model.py:48-64)
// on gfx950: softmax over the 9 logits of every fine pixel, the weighted sum of the 3 x 3 neighbourhood of 8 * flow, and the
// [B, 2, 8, 8, H, W] -> [B, 2, 8H, 8W] shuffle, in ONE kernel.
//
// A workgroup of 256 threads owns kTile = 32 consecutive coarse pixels of one coarse row and kRows = 2 of the 8 fine rows i:
//   stage    8 * flow of the 3 x (kTile + 2) padded neighbourhood, both channels, into LDS (+0 outside the image);
//   compute  thread (t = tid % 32, j = tid / 32) takes pixel x0 + t, fine column j and the kRows fine rows: per row 9 mask loads
//            (lanes run along the coarse x of one mask channel: each wave instruction reads two 128-byte segments, and all 18 loads
//            of a thread are independent), the softmax, and the two channels' sums, written to LDS at [c][row][9 t + j];
//   store    the kRows x 2 fine rows of the tile, each 8 * kTile = 256 consecutive floats: thread tid stores float tid of each, so a
//            wave instruction writes 256 contiguous bytes.
// The pitch of 9 floats per pixel makes the compute phase's LDS writes conflict-free (9 is odd: 32 lanes with consecutive t fall
// on 32 different banks) and costs the store phase's reads at most a 2-way conflict.
// Arithmetic: exactly the contract's sequence of correctly rounded float32 operations (exp_c included); with -ffp-contract=off the
// results are bit-identical to the scalar restatement (tests/flow_upsample_ref.c).  Every index is 64-bit; the only data-dependent
// quantity that becomes an integer is exp_c's n, which is -126 .. 0 by the cutoff test before it; no address depends on the data.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ftk_device.h"
#include "raft_math.h"

namespace ftk {
namespace {

constexpr int kTile = kFlowUpsampleTile;
constexpr int kRows = 2;              // fine rows per workgroup
constexpr int kRowGroups = 8 / kRows;
constexpr int kPitch = 9;             // LDS floats per coarse pixel of one fine row: 8 + 1
constexpr int kThreads = 256;
static_assert(kTile == FTK_FLOW_UPSAMPLE_TILE, "include/ftk.h states the tile width");
static_assert(kThreads == 8 * kTile, "one thread per (pixel of the tile, fine column)");

__global__ __launch_bounds__(kThreads) void flow_upsample_kernel(FlowUpsampleParams prm, int tiles_x) {
    __shared__ float s_flow[2][3][kTile + 2];
    __shared__ float s_out[2][kRows][kTile * kPitch];
    const int tid = threadIdx.x;
    const int H = prm.H, W = prm.W;
    // blockIdx.x = tile + tiles_x * (row group + kRowGroups * (y + H * b))
    int64_t g = blockIdx.x;
    const int tile = (int)(g % tiles_x);
    g /= tiles_x;
    const int i0 = (int)(g % kRowGroups) * kRows;
    g /= kRowGroups;
    const int y = (int)(g % H);
    const int64_t b = g / H;
    const int x0 = tile * kTile;
    const int64_t HW = (int64_t)H * W;

    // stage: contract step 5
    if (tid < 2 * 3 * (kTile + 2)) {
        const int c = tid / (3 * (kTile + 2)), rem = tid % (3 * (kTile + 2));
        const int dy = rem / (kTile + 2), dx = rem % (kTile + 2);
        const int yy = y + dy - 1;
        const int64_t xx = (int64_t)x0 + dx - 1;
        float v = 0.0f;
        if (yy >= 0 && yy < H && xx >= 0 && xx < W) {
            v = 8.0f * prm.flow[(b * 2 + c) * HW + (int64_t)yy * W + xx];
        }
        s_flow[c][dy][dx] = v;
    }
    __syncthreads();

    const int t = tid & (kTile - 1), j = tid / kTile;
    if ((int64_t)x0 + t < W) {
        const float *mp = prm.mask + (b * 576) * HW + (int64_t)y * W + x0 + t;
        float xs[kRows][9];
        for (int r = 0; r < kRows; ++r) {
            for (int k = 0; k < 9; ++k) {
                xs[r][k] = mp[(int64_t)(k * 64 + (i0 + r) * 8 + j) * HW] * prm.mask_scale;  // step 1
            }
        }
        float f[2][9];
        for (int c = 0; c < 2; ++c) {
            for (int k = 0; k < 9; ++k) {
                f[c][k] = s_flow[c][k / 3][t + k % 3];
            }
        }
        for (int r = 0; r < kRows; ++r) {
            float m = xs[r][0];  // step 2
            for (int k = 1; k < 9; ++k) {
                if (xs[r][k] > m) {
                    m = xs[r][k];
                }
            }
            float e[9];
            for (int k = 0; k < 9; ++k) {
                e[k] = exp_c(xs[r][k] - m);  // step 3
            }
            float s = e[0] + e[1];  // step 4
            for (int k = 2; k < 9; ++k) {
                s = s + e[k];
            }
            float a0 = 0.0f, a1 = 0.0f;
            for (int k = 0; k < 9; ++k) {  // step 6
                const float w = e[k] / s;
                const float p0 = f[0][k] * w, p1 = f[1][k] * w;
                a0 = k == 0 ? p0 : a0 + p0;
                a1 = k == 0 ? p1 : a1 + p1;
            }
            s_out[0][r][t * kPitch + j] = a0;
            s_out[1][r][t * kPitch + j] = a1;
        }
    }
    __syncthreads();

    // store: fine row (c, r) of the tile is out[b][c][8 y + i0 + r][8 x0 .. 8 x0 + 8 kTile - 1]
    const int64_t W8 = 8 * (int64_t)W;
    const int64_t gx = 8 * (int64_t)x0 + tid;
    if (gx < W8) {
        const int src = (tid >> 3) * kPitch + (tid & 7);
        for (int c = 0; c < 2; ++c) {
            for (int r = 0; r < kRows; ++r) {
                prm.out[((b * 2 + c) * 8 * H + 8 * (int64_t)y + i0 + r) * W8 + gx] = s_out[c][r][src];
            }
        }
    }
}

}  // namespace

hipError_t flow_upsample_launch(const FlowUpsampleParams &p, hipStream_t stream) {
    const int64_t tiles_x = ((int64_t)p.W + kTile - 1) / kTile;
    const int64_t groups = tiles_x * kRowGroups * p.H * p.B;  // <= B * H * W / 8 + 4 * B * H, and the entry has held 2304 * B * H * W to int64
    if (groups < 1 || groups > 0x7fffffff) {
        return hipErrorInvalidValue;
    }
    hipLaunchKernelGGL(flow_upsample_kernel, dim3((unsigned)groups), dim3(kThreads), 0, stream, p, (int)tiles_x);
    return hipGetLastError();
}

}  // namespace ftk
