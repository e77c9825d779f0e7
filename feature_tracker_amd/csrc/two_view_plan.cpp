// two_view_plan.cpp — two_view_plan.h's pure function.
#include "two_view_plan.h"

namespace ftk {

const char *two_view_refusal_name(TwoViewRefusal r) {
    switch (r) {
        case TwoViewRefusal::None: return "none";
        case TwoViewRefusal::Sizes: return "sizes";
        case TwoViewRefusal::Points: return "points";
        case TwoViewRefusal::Hypotheses: return "hypotheses";
        case TwoViewRefusal::Mode: return "mode";
        case TwoViewRefusal::Prefer: return "prefer";
    }
    return "?";
}

TwoViewPlan two_view_plan(const TwoViewPlanInput &in) {
    TwoViewPlan p{};
    if (in.mode < kTwoViewFundamental || in.mode > (in.slots == 1 ? kTwoViewFundamental : kTwoViewAuto)) {
        p.refused = TwoViewRefusal::Mode;
        return p;
    }
    if (in.prefer_permille < 0 || in.prefer_permille > kTwoViewMaxPermille) {
        p.refused = TwoViewRefusal::Prefer;
        return p;
    }
    if (in.n < 1 || in.hypotheses < 1 || in.image_rows < 1 || in.image_cols < 1 || in.image_rows > kEpipolarMaxSide || in.image_cols > kEpipolarMaxSide ||
        in.slots < 1 || in.slots > kTwoViewMaxSlots) {
        p.refused = TwoViewRefusal::Sizes;
        return p;
    }
    if (in.n > kEpipolarMaxPoints) {
        p.refused = TwoViewRefusal::Points;
        return p;
    }
    if (in.hypotheses > kEpipolarMaxHypotheses) {
        p.refused = TwoViewRefusal::Hypotheses;
        return p;
    }
    const auto up16 = [](size_t v) { return (v + 15) & ~(size_t)15; };
    const size_t slots = (size_t)in.slots;
    p.refused = TwoViewRefusal::None;
    p.slots = in.slots;
    p.run_fundamental = in.mode != kTwoViewHomography;
    p.run_homography = in.mode != kTwoViewFundamental;
    p.launches = 2 + 2 * (p.run_fundamental + p.run_homography);
    p.scan_per_thread = (in.n + kEpipolarScanBlock - 1) / kEpipolarScanBlock;
    p.scan_lds = sizeof(int32_t) * kEpipolarScanBlock;
    p.hyp_blocks = (uint32_t)((in.hypotheses + kEpipolarHypBlock - 1) / kEpipolarHypBlock);
    p.hyp_lds = sizeof(float) * kEpipolarHypLdsFloats * kEpipolarHypBlock;
    p.score_tiles = (uint32_t)((in.n + kEpipolarScoreTile - 1) / kEpipolarScoreTile);
    p.score_groups = (uint32_t)((in.hypotheses + kEpipolarScoreGroup - 1) / kEpipolarScoreGroup);
    p.score_lds = sizeof(float) * 4 * kEpipolarScoreTile;
    p.select_per_thread = (in.hypotheses + kEpipolarScanBlock - 1) / kEpipolarScanBlock;
    p.off_points = 16;
    p.off_list = p.off_points + up16(sizeof(float) * 4 * (size_t)in.n);
    p.off_counts = p.off_list + up16(sizeof(int32_t) * (size_t)in.n);
    p.off_models = p.off_counts + up16(sizeof(int32_t) * slots * (size_t)in.hypotheses);
    p.off_valid = p.off_models + up16(sizeof(float) * 9 * slots * (size_t)in.hypotheses);
    p.bytes = p.off_valid + up16(slots * (size_t)in.hypotheses);
    return p;
}

}  // namespace ftk
