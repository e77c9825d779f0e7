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
    const size_t n = (size_t)in.n, k = (size_t)in.slots * (size_t)in.hypotheses;
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
    ftk_layout16 ws;  // cannot wrap: the limits hold every count below 2^17
    p.m = ws.take<int32_t>(1);
    p.points = ws.take<float4>(n);
    p.list = ws.take<int32_t>(n);
    p.counts = ws.take<int32_t>(k);
    p.models = ws.take<float>(9 * k);
    p.valid = ws.take<uint8_t>(k);
    p.bytes = ws.bytes();
    return p;
}

}  // namespace ftk
