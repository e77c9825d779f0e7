// sep_conv_gru_plan.h — the launch plan of the two SepConvGru kernels (raft_gru_kernels.hip), as match_plan.h is the
// matchers': a pure function of values (no context, no environment, no HIP call; tests/test_sep_conv_gru_cpu.py walks it without a
// device through host/build/sep_conv_gru_plan_cli).  ftk_raft_layers.cpp plans, the launcher carries the plan out.  The wave split, the
// tile counts and the grid are raft_gemm_plan.h's, shared with raft_conv_plan.h.
#pragma once

#include "ftk_device.h"
#include "raft_gemm_plan.h"

namespace ftk {

constexpr int kGruMaxParts = 3;            // FTK_SEP_CONV_GRU_MAX_PARTS: tensors of x
constexpr int kGruMaxHChannels = 1024;     // FTK_SEP_CONV_GRU_MAX_H_CHANNELS
constexpr int kGruMaxInChannels = 4096;    // FTK_SEP_CONV_GRU_MAX_IN_CHANNELS: x_channels + h_channels
constexpr int kGruChunk = 16;              // FTK_SEP_CONV_GRU_CHUNK: input channels staged in LDS at a time (even: a chunk is whole k-steps)
constexpr int kGruLdsFloats = kGruChunk * (kGemmWaves + 4) * kGemmTile;  // the widest strip: vertical, ks 5, wn 4 (4 + 4 rows of 32)

struct SepConvGruPlanInput {
    int32_t h_channels, in_channels;  // in_channels = x_channels + h_channels
    int32_t kernel_size, vertical, gates;  // gates 1: the stacked z | r matrix (2 h_channels rows), 0: the candidate's (h_channels rows)
    int32_t B, H, W;
};
enum class GruRefusal { None, KernelSize, HChannels, InChannels, Sizes, Grid };
struct SepConvGruPlan {
    GruRefusal refused;  // not None: nothing else is set
    int32_t out_channels, m_tiles;  // rows of the weight matrix and its 32-row tiles
    int32_t wm, wn;                 // wm * wn = kGemmWaves; a workgroup owns wm tiles of output channels and wn tiles of pixels
    int32_t m_groups;               // grid.y: ceil(m_tiles / wm)
    int32_t tile_w, tile_h;         // pixels of a workgroup: 32 wn x 1 (horizontal pass), 32 x wn (vertical pass)
    int32_t tiles_x, tiles_y;       // grid.x = tiles_x * tiles_y * B, x fastest
    int32_t chunks, steps_per_chunk, k_steps;  // ceil(in_channels / kGruChunk); kGruChunk * ks / 2; their product (the packed matrix's k-steps)
    int32_t pitch;                  // LDS floats per staged channel: the strip and its halo of 2 (ks / 2) along the pass direction
    size_t lds;                     // bytes the kernel uses: kGruChunk * pitch * 4 (its static array is kGruLdsFloats)
    dim3 grid, block;
    const char *mfma;               // the MFMA form
};
const char *gru_refusal_name(GruRefusal r);
SepConvGruPlan sep_conv_gru_plan(const SepConvGruPlanInput &in);
// floats of the packed weight matrix of `out_channels` rows: ceil(out_channels / 32) * k_steps * 64 (k_steps as the plan's)
int64_t sep_conv_gru_packed_elements(int32_t out_channels, int32_t in_channels, int32_t kernel_size);

}  // namespace ftk
