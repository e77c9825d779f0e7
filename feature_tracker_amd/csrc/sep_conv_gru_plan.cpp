// sep_conv_gru_plan.cpp — sep_conv_gru_plan (sep_conv_gru_plan.h): which tile, chunk and grid a SepConvGru kernel gets.
#include "sep_conv_gru_plan.h"

namespace ftk {

const char *gru_refusal_name(GruRefusal r) {
    switch (r) {
    case GruRefusal::None: return "none";
    case GruRefusal::KernelSize: return "kernel_size";
    case GruRefusal::HChannels: return "h_channels";
    case GruRefusal::InChannels: return "in_channels";
    case GruRefusal::Sizes: return "sizes";
    case GruRefusal::Grid: return "grid";
    }
    return "?";
}

int64_t sep_conv_gru_packed_elements(int32_t out_channels, int32_t in_channels, int32_t kernel_size) {
    const int64_t m_tiles = ((int64_t)out_channels + kGruTile - 1) / kGruTile;
    const int64_t chunks = ((int64_t)in_channels + kGruChunk - 1) / kGruChunk;
    return m_tiles * chunks * (kGruChunk * kernel_size / 2) * 64;
}

SepConvGruPlan sep_conv_gru_plan(const SepConvGruPlanInput &in) {
    SepConvGruPlan p{};
    p.refused = GruRefusal::None;
    if (in.kernel_size != 3 && in.kernel_size != 5) {
        p.refused = GruRefusal::KernelSize;
    } else if (in.h_channels < 1 || in.h_channels > kGruMaxHChannels) {
        p.refused = GruRefusal::HChannels;
    } else if (in.in_channels <= in.h_channels || in.in_channels > kGruMaxInChannels) {
        p.refused = GruRefusal::InChannels;
    } else if (in.B < 1 || in.H < 1 || in.W < 1) {
        p.refused = GruRefusal::Sizes;
    }
    if (p.refused != GruRefusal::None) {
        return p;
    }
    const int pad = in.kernel_size / 2;
    p.out_channels = in.gates ? 2 * in.h_channels : in.h_channels;
    p.m_tiles = (p.out_channels + kGruTile - 1) / kGruTile;
    // Waves share the staged input: as many of them along the output channels as there are tiles (3 tiles: 4 waves, one idle in the
    // matrix loop), the rest along the pixels.
    p.wm = p.m_tiles >= 3 ? 4 : p.m_tiles;
    p.wn = kGruWaves / p.wm;
    p.m_groups = (p.m_tiles + p.wm - 1) / p.wm;
    p.tile_w = in.vertical ? kGruTile : kGruTile * p.wn;
    p.tile_h = in.vertical ? p.wn : 1;
    p.tiles_x = (in.W + p.tile_w - 1) / p.tile_w;
    p.tiles_y = (in.H + p.tile_h - 1) / p.tile_h;
    p.chunks = (in.in_channels + kGruChunk - 1) / kGruChunk;
    p.steps_per_chunk = kGruChunk * in.kernel_size / 2;
    p.k_steps = p.chunks * p.steps_per_chunk;
    p.pitch = in.vertical ? (p.wn + 2 * pad) * kGruTile : kGruTile * p.wn + 2 * pad;
    p.lds = (size_t)kGruChunk * p.pitch * sizeof(float);
    const int64_t groups = (int64_t)p.tiles_x * p.tiles_y * in.B;
    if (groups > 0x7fffffff) {
        p = SepConvGruPlan{};
        p.refused = GruRefusal::Grid;
        return p;
    }
    p.grid = dim3((unsigned)groups, (unsigned)p.m_groups);
    p.block = dim3(64 * kGruWaves);
    p.mfma = "32x32x2_f32";
    return p;
}

}  // namespace ftk
