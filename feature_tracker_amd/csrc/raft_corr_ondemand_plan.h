// raft_corr_ondemand_plan.h — the launch plan of the on-demand correlation kernels (raft_corr_ondemand_kernels.hip), as
// raft_conv_plan.h is conv2d_kernel's: a pure function of values (no context, no environment, no HIP call;
// tests/test_raft_corr_ondemand_cpu.py walks it without a device through host/build/corr_ondemand_plan_cli).  ftk_corr_ondemand.cpp plans,
// the launchers carry the plan out.
#pragma once

#include "ftk_device.h"

namespace ftk {

constexpr int kCorrOdWaves = 4;            // waves of a lookup workgroup: one query pixel each, all of one level and batch item
constexpr int kCorrOdMaxLatticeSide = 16;  // widest lattice a wave keeps in LDS (2r + 2 <= 16: radius <= 7); wider windows evaluate every corner directly
constexpr int kCorrOdLatticeFloats = kCorrOdMaxLatticeSide * kCorrOdMaxLatticeSide;  // per wave
constexpr int kCorrOdTile = 32;            // the transpose's tile: 32 pixels x 32 channels, a block of 32 x 8 threads
constexpr int kCorrOdPoolBlock = 256;      // threads of a pool workgroup, one output value each

struct CorrOdPlanInput {
    int32_t B, C, H, W, levels, radius;
    int32_t aligned16;  // the workspace pointer is 16-byte aligned (with C % 4 == 0: the chain reads 16 bytes at a time)
};
enum class CorrOdRefusal { None, Sizes, Channels, Levels, EmptyLevel, Radius, Overflow, Grid };
struct CorrOdPlan {
    CorrOdRefusal refused;  // not None: nothing else is set
    int32_t empty_level;    // EmptyLevel: the first level that would be empty
    int64_t elements;       // floats of the workspace: B * C * (H * W + sum_l H_l * W_l)
    int64_t level_offset[kCorrMaxLevels];  // of fmap1's level l, [B][H_l][W_l][C]; fmap0 transposed, [B][H * W][C], is at 0
    int32_t level_h[kCorrMaxLevels], level_w[kCorrMaxLevels];
    // prepare: one transpose launch over both maps, then one pool launch per level >= 1
    dim3 transpose_grid, transpose_block;  // x: tiles of 32 pixels, y: tiles of 32 channels, z: 2 * B (fmap0's items, then fmap1's)
    int64_t pool_blocks[kCorrMaxLevels];   // [0] unused
    // lookup
    int32_t side;            // window side 2r + 1
    int32_t samples;         // K = side^2
    int32_t sample_passes;   // ceil(K / 64): a lane owns samples lane, lane + 64, ...
    int32_t lattice_side;    // 2r + 2, or 0: no lattice (radius above 7), every corner of every sample is evaluated directly
    int32_t lattice_points;  // lattice_side^2
    int32_t lattice_passes;  // ceil(lattice_points / 64)
    int32_t vector;          // the channel chain loads 16 bytes at a time (C % 4 == 0 and an aligned workspace); else 4
    size_t lds;              // bytes of the lookup kernel's static array
    dim3 lookup_grid, lookup_block;  // x: ceil(H * W / 4), y: levels, z: B
};
const char *corr_od_refusal_name(CorrOdRefusal r);
CorrOdPlan raft_corr_ondemand_plan(const CorrOdPlanInput &in);

}  // namespace ftk
