// raft_conv_plan.h — the launch plan of conv2d_kernel (raft_conv_kernels.hip), as sep_conv_gru_plan.h is the GRU's: a
// pure function of values (no context, no environment, no HIP call; tests/test_update_block_cpu.py walks it without a device through
// host/build/raft_conv_plan_cli).  ftk_raft_layers.cpp plans, the launcher carries the plan out.  The wave split, the tile counts and
// the grid are raft_gemm_plan.h's, shared with sep_conv_gru_plan.h.
#pragma once

#include "ftk_device.h"
#include "raft_gemm_plan.h"

namespace ftk {

constexpr int kConvMaxParts = 3;           // FTK_CONV2D_MAX_PARTS: tensors of the input
constexpr int kConvMaxOutChannels = 1024;  // FTK_CONV2D_MAX_OUT_CHANNELS
constexpr int kConvMaxInChannels = 4096;   // FTK_CONV2D_MAX_IN_CHANNELS: the channels of all parts
// Input channels staged in LDS at a time (FTK_CONV2D_CHUNK_1 / _3 / _7): chosen so that a chunk is whole k-steps, close to the GRU's 40
// per chunk: 16, 36 and 49.  Each is a divisor or a multiple of kGemmWaves (the staging splits a chunk over the waves).
constexpr int conv_chunk(int kernel_size) { return kernel_size == 1 ? 32 : kernel_size == 3 ? 8 : 2; }
constexpr int conv_steps(int kernel_size) { return conv_chunk(kernel_size) * kernel_size * kernel_size / 2; }
// LDS floats per staged channel: (wn + 2 pad) rows of (32 + 2 pad); the static array of the kernel holds a chunk at wn = kGemmWaves
constexpr int conv_row(int kernel_size) { return kGemmTile + 2 * (kernel_size / 2); }
constexpr int conv_pitch(int kernel_size, int wn) { return (wn + 2 * (kernel_size / 2)) * conv_row(kernel_size); }
constexpr int conv_lds_floats(int kernel_size) { return conv_chunk(kernel_size) * conv_pitch(kernel_size, kGemmWaves); }
// Stride 2 (kernel sizes 1 and 3): a workgroup still owns 32 output pixels x wn output rows and the chunk is the same, so
// the packed weights are.  A 3 x 3 strip is 2 (wn - 1) + 3 input rows of 63 + 2 + 1 input columns, the even columns of a row in one plane
// of 32 + pad floats and the odd ones in a second plane behind it: tap tx of output pixel j is staged column 2 j + tx, float j + tx / 2 of
// plane tx % 2, so the 32 lanes of a tap read 32 consecutive floats.  A 1 x 1 reads even rows and even columns only: it keeps just those,
// wn rows of one plane.
constexpr int conv_s2_plane(int kernel_size) { return kGemmTile + kernel_size / 2; }
constexpr int conv_s2_row(int kernel_size) { return kernel_size == 1 ? kGemmTile : 2 * conv_s2_plane(kernel_size); }
constexpr int conv_s2_rows(int kernel_size, int wn) { return kernel_size == 1 ? wn : 2 * (wn - 1) + kernel_size; }
constexpr int conv_s2_pitch(int kernel_size, int wn) { return conv_s2_rows(kernel_size, wn) * conv_s2_row(kernel_size); }
constexpr int conv_s2_lds_floats(int kernel_size) { return conv_chunk(kernel_size) * conv_s2_pitch(kernel_size, kGemmWaves); }

struct ConvPlanInput {
    int32_t out_channels, in_channels, kernel_size;
    int32_t B, H, W;     // of the input
    int32_t stride = 1;  // 1 or 2 (2: kernel sizes 1 and 3); the output is ceil(H / stride) x ceil(W / stride)
    int32_t pool = 0;    // 1: a 2 x 2 max-pool in the epilogue (stride 1, kernel sizes 1 and 3, H, W >= 2); the output is
                         // floor(H / 2) x floor(W / 2).  0: every field of the plan is what it was without this member
};
enum class ConvRefusal { None, KernelSize, OutChannels, InChannels, Sizes, Grid, Stride, Pool };
struct ConvPlan {
    ConvRefusal refused;  // not None: nothing else is set
    int32_t m_tiles;      // 32-row tiles of the weight matrix
    int32_t wm, wn;       // wm * wn = kGemmWaves; a workgroup owns wm tiles of output channels and wn rows of 32 pixels
    int32_t m_groups;     // grid.y: ceil(m_tiles / wm)
    int32_t stride, out_h, out_w;  // the input's; the output's sizes, which the tiles partition
    int32_t pool;              // the input's.  1: wm = min(m_tiles, 2), so wn and with it a workgroup's first row ty * wn are even
    int32_t tile_w, tile_h;    // output pixels of a workgroup: 32 x wn (pool 1: convolution pixels, 16 x wn / 2 outputs)
    int32_t tiles_x, tiles_y;  // grid.x = tiles_x * tiles_y * B, x fastest
    int32_t chunk, chunks, steps_per_chunk, k_steps;  // conv_chunk; ceil(in_channels / chunk); conv_steps; chunks * steps_per_chunk
    int32_t pitch;        // LDS floats per staged channel: the strip and its halo on all four sides (rows * row)
    int32_t rows, row;    // staged rows of a channel and LDS floats of one
    int32_t strip_h, strip_w;  // input rows and columns a workgroup's taps span, from (stride * y0 - pad, stride * x0 - pad)
    size_t lds;           // bytes the kernel uses: chunk * pitch * 4 (its static array is conv_lds_floats / conv_s2_lds_floats)
    dim3 grid, block;
    const char *mfma;     // the MFMA form
};
const char *conv_refusal_name(ConvRefusal r);
ConvPlan raft_conv_plan(const ConvPlanInput &in);
// floats of the packed weight matrix: ceil(out_channels / 32) * k_steps * 64 (k_steps as the plan's); 0 for a kernel size the plan refuses
int64_t raft_conv_packed_elements(int32_t out_channels, int32_t in_channels, int32_t kernel_size);

}  // namespace ftk
