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
    }
    return "?";
}

int64_t raft_conv_packed_elements(int32_t out_channels, int32_t in_channels, int32_t kernel_size) {
    if (kernel_size != 1 && kernel_size != 3 && kernel_size != 7) {
        return 0;
    }
    const int64_t m_tiles = ((int64_t)out_channels + kConvTile - 1) / kConvTile;
    const int64_t chunks = ((int64_t)in_channels + conv_chunk(kernel_size) - 1) / conv_chunk(kernel_size);
    return m_tiles * chunks * conv_steps(kernel_size) * 64;
}

ConvPlan raft_conv_plan(const ConvPlanInput &in) {
    ConvPlan p{};
    p.refused = ConvRefusal::None;
    if (in.kernel_size != 1 && in.kernel_size != 3 && in.kernel_size != 7) {
        p.refused = ConvRefusal::KernelSize;
    } else if ((in.stride != 1 && in.stride != 2) || (in.stride == 2 && in.kernel_size == 7)) {
        p.refused = ConvRefusal::Stride;
    } else if (in.out_channels < 1 || in.out_channels > kConvMaxOutChannels) {
        p.refused = ConvRefusal::OutChannels;
    } else if (in.in_channels < 1 || in.in_channels > kConvMaxInChannels) {
        p.refused = ConvRefusal::InChannels;
    } else if (in.B < 1 || in.H < 1 || in.W < 1) {
        p.refused = ConvRefusal::Sizes;
    }
    if (p.refused != ConvRefusal::None) {
        return p;
    }
    p.m_tiles = (in.out_channels + kConvTile - 1) / kConvTile;
    // As in sep_conv_gru_plan: the waves share the staged input, as many of them along the output channels as there are tiles (3 tiles: 4
    // waves, one idle in the matrix loop), the rest along the rows.
    p.wm = p.m_tiles >= 3 ? 4 : p.m_tiles;
    p.wn = kConvWaves / p.wm;
    p.m_groups = (p.m_tiles + p.wm - 1) / p.wm;
    p.tile_w = kConvTile;
    p.tile_h = p.wn;
    p.stride = in.stride;
    p.out_h = (int32_t)(((int64_t)in.H + in.stride - 1) / in.stride);
    p.out_w = (int32_t)(((int64_t)in.W + in.stride - 1) / in.stride);
    p.tiles_x = (int32_t)(((int64_t)p.out_w + p.tile_w - 1) / p.tile_w);  // 64-bit: W + 31 may pass 2^31
    p.tiles_y = (int32_t)(((int64_t)p.out_h + p.tile_h - 1) / p.tile_h);
    p.chunk = conv_chunk(in.kernel_size);
    p.chunks = (in.in_channels + p.chunk - 1) / p.chunk;
    p.steps_per_chunk = conv_steps(in.kernel_size);
    p.k_steps = p.chunks * p.steps_per_chunk;
    const int32_t pad = in.kernel_size / 2;
    p.rows = in.stride == 1 ? p.wn + 2 * pad : conv_s2_rows(in.kernel_size, p.wn);
    p.row = in.stride == 1 ? conv_row(in.kernel_size) : conv_s2_row(in.kernel_size);
    p.pitch = p.rows * p.row;  // stride 1: conv_pitch
    p.strip_h = in.stride * (p.wn - 1) + in.kernel_size;
    p.strip_w = in.stride == 1 ? conv_row(in.kernel_size) : 2 * (kConvTile - 1) + in.kernel_size + 1;
    p.lds = (size_t)p.chunk * p.pitch * sizeof(float);
    const int64_t tiles = (int64_t)p.tiles_x * p.tiles_y;  // below 2^57; times B only once it is known to be below 2^31
    const int64_t groups = tiles > 0x7fffffff ? tiles : tiles * in.B;
    if (groups > 0x7fffffff) {
        p = ConvPlan{};
        p.refused = ConvRefusal::Grid;
        return p;
    }
    p.grid = dim3((unsigned)groups, (unsigned)p.m_groups);
    p.block = dim3(64 * kConvWaves);
    p.mfma = "32x32x2_f32";
    return p;
}

}  // namespace ftk
