// track_table_plan.cpp — track_table_plan.h's pure function.
#include "track_table_plan.h"

namespace ftk {

const char *track_table_refusal_name(TrackTableRefusal r) {
    switch (r) {
        case TrackTableRefusal::None: return "none";
        case TrackTableRefusal::Sizes: return "sizes";
        case TrackTableRefusal::Survivors: return "survivors";
        case TrackTableRefusal::Slots: return "slots";
    }
    return "?";
}

TrackTablePlan track_table_plan(const TrackTablePlanInput &in) {
    TrackTablePlan p{};
    if (in.rows < 1 || in.cols < 1 || in.n_occupied < 0 || (int64_t)in.rows * in.cols >= (1ll << 32)) {
        p.refused = TrackTableRefusal::Sizes;
        return p;
    }
    if (in.n_slots < 0 || in.n_slots > kTrackTableMaxSlots) {
        p.refused = TrackTableRefusal::Slots;
        return p;
    }
    const int32_t d = in.min_distance > 1 ? in.min_distance : 1;
    // survivors are pairwise at Chebyshev distance >= d: at most one per d x d cell of the image
    const int64_t bound = (((int64_t)in.rows + d - 1) / d) * (((int64_t)in.cols + d - 1) / d);
    const bool has_centre = in.rows >= kHarrisMinSide && in.cols >= kHarrisMinSide;
    if (has_centre && bound > kHarrisDeviceMaxSurvivors) {
        p.refused = TrackTableRefusal::Survivors;
        return p;
    }
    p.refused = TrackTableRefusal::None;
    p.distance = d;
    p.reach = d - 1;
    p.capacity = has_centre ? (int32_t)bound : 0;
    p.image_blocks = (uint32_t)(((int64_t)in.rows * in.cols + 255) / 256);
    p.stamp_blocks = (uint32_t)((in.n_occupied + 255) / 256);
    p.rank_blocks = (uint32_t)((p.capacity + kHarrisRankTile - 1) / kHarrisRankTile);
    p.rank_lds = sizeof(unsigned long long) * kHarrisRankTile;
    p.retire_per_thread = (in.n_slots + kTrackRetireBlock - 1) / kTrackRetireBlock;
    p.retire_lds = sizeof(int32_t) * kTrackRetireBlock;
    return p;
}

}  // namespace ftk
