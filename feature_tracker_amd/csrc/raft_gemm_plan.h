// raft_gemm_plan.h — what the launch plans of RAFT's implicit-GEMM kernels (raft_gemm_core.h: sep_conv_gru_plan.h for the GRU,
// raft_conv_plan.h for the conv layers) have in common, stated once: the split of a workgroup's waves, the tile counts, the grid with
// its refusal and the size of a packed weight matrix.  Pure functions of values, like the plans; DESIGN.md 5.13.
#pragma once

#include <stdint.h>

namespace ftk {

constexpr int kGemmWaves = 4;  // waves of a workgroup, arranged wm (output-channel tiles) x wn (pixel tiles)
constexpr int kGemmTile = 32;  // the MFMA tile: 32 output channels x 32 pixels

// The waves share the staged input: as many of them along the output channels as there are tiles (3 tiles: 4 waves, one idle in the
// matrix loop), the rest along the pixels.
struct GemmWaveSplit {
    int32_t m_tiles;   // 32-row tiles of the weight matrix
    int32_t wm, wn;    // wm * wn = kGemmWaves
    int32_t m_groups;  // grid.y: ceil(m_tiles / wm)
};
inline GemmWaveSplit gemm_wave_split(int32_t out_channels) {
    GemmWaveSplit s{};
    s.m_tiles = (out_channels + kGemmTile - 1) / kGemmTile;
    s.wm = s.m_tiles >= 3 ? 4 : s.m_tiles;
    s.wn = kGemmWaves / s.wm;
    s.m_groups = (s.m_tiles + s.wm - 1) / s.wm;
    return s;
}

// ceil(extent / tile) in 64 bits: extent + tile - 1 may pass 2^31
inline int32_t gemm_tiles(int32_t extent, int32_t tile) { return (int32_t)(((int64_t)extent + tile - 1) / tile); }

// grid.x = tiles_x * tiles_y * B, x fastest; -1 when that passes 2^31 - 1 (the plan then refuses with its Grid)
inline int64_t gemm_groups(int32_t tiles_x, int32_t tiles_y, int32_t B) {
    const int64_t tiles = (int64_t)tiles_x * tiles_y;  // below 2^62; times B only once it is known to be below 2^31
    if (tiles > 0x7fffffff || tiles * B > 0x7fffffff) {
        return -1;
    }
    return tiles * B;
}

inline int32_t gemm_chunks(int32_t in_channels, int32_t chunk) { return (in_channels + chunk - 1) / chunk; }

// floats of a packed weight matrix [m_tiles][k_steps][64]: whole row tiles, whole chunks of `chunk` input channels of `steps_per_chunk`
// k-steps each
inline int64_t gemm_packed_elements(int32_t out_channels, int32_t in_channels, int32_t chunk, int32_t steps_per_chunk) {
    const int64_t m_tiles = ((int64_t)out_channels + kGemmTile - 1) / kGemmTile;
    const int64_t chunks = ((int64_t)in_channels + chunk - 1) / chunk;
    return m_tiles * chunks * steps_per_chunk * 64;
}

}  // namespace ftk
