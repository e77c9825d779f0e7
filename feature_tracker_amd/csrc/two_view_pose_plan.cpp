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
    p.refused = TwoViewPoseRefusal::None;
    p.launches = 5;
    p.scan_per_thread = (in.n + kEpipolarScanBlock - 1) / kEpipolarScanBlock;
    p.tiles = (uint32_t)((in.n + kPoseTile - 1) / kPoseTile);
    p.moment_lds = sizeof(float) * kPoseMoments * kPoseTile;
    ftk_layout16 ws;  // cannot wrap: n <= 2^16
    p.m = ws.take<int32_t>(1);
    p.points = ws.take<float4>((size_t)in.n);
    p.totals = ws.take<float>(kPoseMoments * (size_t)p.tiles);
    p.model = ws.take<float>(kPoseModelFloats);
    p.bytes = ws.bytes();
    return p;
}

}  // namespace ftk
