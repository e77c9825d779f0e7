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
    if (in.mode < kTwoViewFundamental || in.mode > kTwoViewAuto) {
        p.refused = TwoViewRefusal::Mode;
        return p;
    }
    if (in.prefer_permille < 0 || in.prefer_permille > kTwoViewMaxPermille) {
        p.refused = TwoViewRefusal::Prefer;
        return p;
    }
    EpipolarPlanInput ein{};
    ein.n = in.n;
    ein.hypotheses = in.hypotheses;
    ein.image_rows = in.image_rows;
    ein.image_cols = in.image_cols;
    const EpipolarPlan e = epipolar_plan(ein);  // the sizes' limits and the launch shapes are 5.20's
    switch (e.refused) {
        case EpipolarRefusal::None: break;
        case EpipolarRefusal::Points: p.refused = TwoViewRefusal::Points; return p;
        case EpipolarRefusal::Hypotheses: p.refused = TwoViewRefusal::Hypotheses; return p;
        default: p.refused = TwoViewRefusal::Sizes; return p;
    }
    const auto up16 = [](size_t v) { return (v + 15) & ~(size_t)15; };
    p.refused = TwoViewRefusal::None;
    p.run_fundamental = in.mode != kTwoViewHomography;
    p.run_homography = in.mode != kTwoViewFundamental;
    p.launches = 2 + 2 * (p.run_fundamental + p.run_homography);
    p.scan_per_thread = e.scan_per_thread;
    p.hyp_blocks = e.hyp_blocks;
    p.hyp_lds = e.hyp_lds;
    p.score_tiles = e.score_tiles;
    p.score_groups = e.score_groups;
    p.score_lds = e.score_lds;
    p.select_per_thread = e.select_per_thread;
    p.off_points = 16;
    p.off_list = p.off_points + up16(sizeof(float) * 4 * (size_t)in.n);
    p.off_counts = p.off_list + up16(sizeof(int32_t) * (size_t)in.n);
    p.off_models = p.off_counts + up16(sizeof(int32_t) * 2 * (size_t)in.hypotheses);
    p.off_valid = p.off_models + up16(sizeof(float) * 18 * (size_t)in.hypotheses);
    p.bytes = p.off_valid + up16(2 * (size_t)in.hypotheses);
    return p;
}

}  // namespace ftk
