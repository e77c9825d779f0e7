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
    return gemm_packed_elements(out_channels, in_channels, kGruChunk, kGruChunk * kernel_size / 2);
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
    const GemmWaveSplit split = gemm_wave_split(p.out_channels);
    p.m_tiles = split.m_tiles, p.wm = split.wm, p.wn = split.wn, p.m_groups = split.m_groups;
    p.tile_w = in.vertical ? kGemmTile : kGemmTile * p.wn;
    p.tile_h = in.vertical ? p.wn : 1;
    p.tiles_x = gemm_tiles(in.W, p.tile_w);
    p.tiles_y = gemm_tiles(in.H, p.tile_h);
    p.chunks = gemm_chunks(in.in_channels, kGruChunk);
    p.steps_per_chunk = kGruChunk * in.kernel_size / 2;
    p.k_steps = p.chunks * p.steps_per_chunk;
    p.pitch = in.vertical ? (p.wn + 2 * pad) * kGemmTile : kGemmTile * p.wn + 2 * pad;
    p.lds = (size_t)kGruChunk * p.pitch * sizeof(float);
    const int64_t groups = gemm_groups(p.tiles_x, p.tiles_y, in.B);
    if (groups < 0) {
        p = SepConvGruPlan{};
        p.refused = GruRefusal::Grid;
        return p;
    }
    p.grid = dim3((unsigned)groups, (unsigned)p.m_groups);
    p.block = dim3(64 * kGemmWaves);
    p.mfma = "32x32x2_f32";
    return p;
}

}  // namespace ftk
