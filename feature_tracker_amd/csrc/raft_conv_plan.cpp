// raft_conv_plan.cpp — raft_conv_plan (raft_conv_plan.h): which tile, chunk and grid a conv2d_kernel launch gets.
#include "raft_conv_plan.h"

namespace ftk {

const char *conv_refusal_name(ConvRefusal r) {
    switch (r) {
    case ConvRefusal::None: return "none";
    case ConvRefusal::KernelSize: return "kernel_size";
    case ConvRefusal::OutChannels: return "out_channels";
    case ConvRefusal::InChannels: return "in_channels";
    case ConvRefusal::Sizes: return "sizes";
    case ConvRefusal::Grid: return "grid";
    case ConvRefusal::Stride: return "stride";
    case ConvRefusal::Pool: return "pool";
    }
    return "?";
}

int64_t raft_conv_packed_elements(int32_t out_channels, int32_t in_channels, int32_t kernel_size) {
    if (kernel_size != 1 && kernel_size != 3 && kernel_size != 7) {
        return 0;
    }
    return gemm_packed_elements(out_channels, in_channels, conv_chunk(kernel_size), conv_steps(kernel_size));
}

ConvPlan raft_conv_plan(const ConvPlanInput &in) {
    ConvPlan p{};
    p.refused = ConvRefusal::None;
    if (in.pool != 0 && in.pool != 1) {
        p.refused = ConvRefusal::Pool;
    } else if ((in.kernel_size != 1 && in.kernel_size != 3 && in.kernel_size != 7) || (in.pool == 1 && in.kernel_size == 7)) {
        p.refused = ConvRefusal::KernelSize;
    } else if ((in.stride != 1 && in.stride != 2) || (in.stride == 2 && in.kernel_size == 7) || (in.pool == 1 && in.stride != 1)) {
        p.refused = ConvRefusal::Stride;
    } else if (in.out_channels < 1 || in.out_channels > kConvMaxOutChannels) {
        p.refused = ConvRefusal::OutChannels;
    } else if (in.in_channels < 1 || in.in_channels > kConvMaxInChannels) {
        p.refused = ConvRefusal::InChannels;
    } else if (in.B < 1 || in.H < 1 || in.W < 1 || (in.pool == 1 && (in.H < 2 || in.W < 2))) {
        p.refused = ConvRefusal::Sizes;
    }
    if (p.refused != ConvRefusal::None) {
        return p;
    }
    GemmWaveSplit split = gemm_wave_split(in.out_channels);
    if (in.pool == 1) {
        // a vertical pooling pair is two waves of one workgroup: an even number of rows, so never wm 4 (128 channels run as two groups of wm 2)
        split.wm = split.m_tiles < 2 ? split.m_tiles : 2;
        split.wn = kGemmWaves / split.wm;
        split.m_groups = (split.m_tiles + split.wm - 1) / split.wm;
    }
    p.m_tiles = split.m_tiles, p.wm = split.wm, p.wn = split.wn, p.m_groups = split.m_groups;
    p.tile_w = kGemmTile;
    p.tile_h = p.wn;
    p.stride = in.stride;
    p.pool = in.pool;
    p.out_h = in.pool == 1 ? in.H / 2 : gemm_tiles(in.H, in.stride);
    p.out_w = in.pool == 1 ? in.W / 2 : gemm_tiles(in.W, in.stride);
    // the tiles partition the output; the pooled form's tiles are of convolution pixels, 2 out_w x 2 out_h of them (a dropped odd row or
    // column belongs to no tile)
    p.tiles_x = gemm_tiles(in.pool == 1 ? 2 * p.out_w : p.out_w, p.tile_w);
    p.tiles_y = gemm_tiles(in.pool == 1 ? 2 * p.out_h : p.out_h, p.tile_h);
    p.chunk = conv_chunk(in.kernel_size);
    p.chunks = gemm_chunks(in.in_channels, p.chunk);
    p.steps_per_chunk = conv_steps(in.kernel_size);
    p.k_steps = p.chunks * p.steps_per_chunk;
    const int32_t pad = in.kernel_size / 2;
    p.rows = in.stride == 1 ? p.wn + 2 * pad : conv_s2_rows(in.kernel_size, p.wn);
    p.row = in.stride == 1 ? conv_row(in.kernel_size) : conv_s2_row(in.kernel_size);
    p.pitch = p.rows * p.row;  // stride 1: conv_pitch
    p.strip_h = in.stride * (p.wn - 1) + in.kernel_size;
    p.strip_w = in.stride == 1 ? conv_row(in.kernel_size) : 2 * (kGemmTile - 1) + in.kernel_size + 1;
    p.lds = (size_t)p.chunk * p.pitch * sizeof(float);
    const int64_t groups = gemm_groups(p.tiles_x, p.tiles_y, in.B);
    if (groups < 0) {
        p = ConvPlan{};
        p.refused = ConvRefusal::Grid;
        return p;
    }
    p.grid = dim3((unsigned)groups, (unsigned)p.m_groups);
    p.block = dim3(64 * kGemmWaves);
    p.mfma = "32x32x2_f32";
    return p;
}

}  // namespace ftk
