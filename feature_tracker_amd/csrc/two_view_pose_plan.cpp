// two_view_pose_plan.cpp — two_view_pose_plan.h's pure function.
#include "two_view_pose_plan.h"

namespace ftk {

const char *two_view_pose_refusal_name(TwoViewPoseRefusal r) {
    switch (r) {
        case TwoViewPoseRefusal::None: return "none";
        case TwoViewPoseRefusal::Sizes: return "sizes";
        case TwoViewPoseRefusal::Points: return "points";
    }
    return "?";
}

TwoViewPosePlan two_view_pose_plan(const TwoViewPosePlanInput &in) {
    TwoViewPosePlan p{};
    if (in.n < 1) {
        p.refused = TwoViewPoseRefusal::Sizes;
        return p;
    }
    if (in.n > kEpipolarMaxPoints) {
        p.refused = TwoViewPoseRefusal::Points;
        return p;
    }
    const auto up16 = [](size_t v) { return (v + 15) & ~(size_t)15; };
    p.refused = TwoViewPoseRefusal::None;
    p.launches = 5;
    p.scan_per_thread = (in.n + kEpipolarScanBlock - 1) / kEpipolarScanBlock;
    p.tiles = (uint32_t)((in.n + kPoseTile - 1) / kPoseTile);
    p.moment_lds = sizeof(float) * kPoseMoments * kPoseTile;
    p.off_points = 16;
    p.off_totals = p.off_points + up16(sizeof(float) * 4 * (size_t)in.n);
    p.off_model = p.off_totals + up16(sizeof(float) * kPoseMoments * (size_t)p.tiles);
    p.bytes = p.off_model + sizeof(float) * kPoseModelFloats;
    return p;
}

}  // namespace ftk
