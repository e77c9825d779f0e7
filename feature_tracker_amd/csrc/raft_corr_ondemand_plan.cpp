// raft_corr_ondemand_plan.cpp — raft_corr_ondemand_plan (raft_corr_ondemand_plan.h): the workspace layout and the grids of the on-demand
// correlation's prepare and lookup launches.
#include "raft_corr_ondemand_plan.h"

#include <stdint.h>

namespace ftk {

const char *corr_od_refusal_name(CorrOdRefusal r) {
    switch (r) {
    case CorrOdRefusal::None: return "none";
    case CorrOdRefusal::Sizes: return "sizes";
    case CorrOdRefusal::Channels: return "channels";
    case CorrOdRefusal::Levels: return "levels";
    case CorrOdRefusal::EmptyLevel: return "empty_level";
    case CorrOdRefusal::Radius: return "radius";
    case CorrOdRefusal::Overflow: return "overflow";
    case CorrOdRefusal::Grid: return "grid";
    }
    return "?";
}

static CorrOdPlan refuse(CorrOdRefusal r, int32_t level = 0) {
    CorrOdPlan p{};
    p.refused = r;
    p.empty_level = level;
    return p;
}

CorrOdPlan raft_corr_ondemand_plan(const CorrOdPlanInput &in) {
    if (in.B < 1 || in.H < 1 || in.W < 1) {
        return refuse(CorrOdRefusal::Sizes);
    }
    if (in.C < 1) {
        return refuse(CorrOdRefusal::Channels);
    }
    if (in.levels < 1 || in.levels > kCorrMaxLevels) {
        return refuse(CorrOdRefusal::Levels);
    }
    if (in.radius < 0 || in.radius > 64) {  // FTK_CORR_MAX_RADIUS
        return refuse(CorrOdRefusal::Radius);
    }
    CorrOdPlan p{};
    p.refused = CorrOdRefusal::None;
    const int64_t HW = (int64_t)in.H * in.W;  // < 2^62
    const int64_t BC = (int64_t)in.B * in.C;  // < 2^62
    const int64_t limit = INT64_MAX / 4;      // the workspace has a byte count
    if (HW > limit / BC) {
        return refuse(CorrOdRefusal::Overflow);
    }
    int64_t total = BC * HW;  // fmap0 transposed
    int32_t h = in.H, w = in.W;
    for (int32_t l = 0; l < in.levels; ++l) {
        if (h == 0 || w == 0) {
            return refuse(CorrOdRefusal::EmptyLevel, l);
        }
        const int64_t hw = (int64_t)h * w;
        if (hw > (limit - total) / BC) {
            return refuse(CorrOdRefusal::Overflow);
        }
        p.level_offset[l] = total;
        p.level_h[l] = h;
        p.level_w[l] = w;
        p.pool_blocks[l] = l == 0 ? 0 : (BC * hw + kCorrOdPoolBlock - 1) / kCorrOdPoolBlock;
        if (p.pool_blocks[l] > 0x7fffffff) {
            return refuse(CorrOdRefusal::Grid);
        }
        total += BC * hw;
        h /= 2;
        w /= 2;
    }
    p.elements = total;
    const int64_t pixel_tiles = (HW + kCorrOdTile - 1) / kCorrOdTile;
    const int64_t channel_tiles = ((int64_t)in.C + kCorrOdTile - 1) / kCorrOdTile;
    const int64_t pixel_groups = (HW + kCorrOdWaves - 1) / kCorrOdWaves;
    if (pixel_tiles > 0x7fffffff || channel_tiles > 65535 || 2 * (int64_t)in.B > 65535 || pixel_groups > 0x7fffffff) {
        return refuse(CorrOdRefusal::Grid);
    }
    p.transpose_grid = dim3((unsigned)pixel_tiles, (unsigned)channel_tiles, (unsigned)(2 * in.B));
    p.transpose_block = dim3(kCorrOdTile, 8);
    p.side = 2 * in.radius + 1;
    p.samples = p.side * p.side;
    p.sample_passes = (p.samples + 63) / 64;
    p.lattice_side = p.side + 1 <= kCorrOdMaxLatticeSide ? p.side + 1 : 0;
    p.lattice_points = p.lattice_side * p.lattice_side;
    p.lattice_passes = (p.lattice_points + 63) / 64;
    p.vector = (in.C % 4 == 0 && in.aligned16) ? 1 : 0;
    p.lds = sizeof(float) * kCorrOdWaves * kCorrOdLatticeFloats;
    p.lookup_grid = dim3((unsigned)pixel_groups, (unsigned)in.levels, (unsigned)in.B);
    p.lookup_block = dim3(64 * kCorrOdWaves);
    return p;
}

}  // namespace ftk
