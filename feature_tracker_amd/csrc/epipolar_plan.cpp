// epipolar_plan.cpp — epipolar_plan.h's pure function.
#include "epipolar_plan.h"

namespace ftk {

const char *epipolar_refusal_name(EpipolarRefusal r) {
    switch (r) {
        case EpipolarRefusal::None: return "none";
        case EpipolarRefusal::Sizes: return "sizes";
        case EpipolarRefusal::Points: return "points";
        case EpipolarRefusal::Hypotheses: return "hypotheses";
    }
    return "?";
}

EpipolarPlan epipolar_plan(const EpipolarPlanInput &in) {
    EpipolarPlan p{};
    if (in.n < 1 || in.hypotheses < 1 || in.image_rows < 1 || in.image_cols < 1 || in.image_rows > kEpipolarMaxSide || in.image_cols > kEpipolarMaxSide) {
        p.refused = EpipolarRefusal::Sizes;
        return p;
    }
    if (in.n > kEpipolarMaxPoints) {
        p.refused = EpipolarRefusal::Points;
        return p;
    }
    if (in.hypotheses > kEpipolarMaxHypotheses) {
        p.refused = EpipolarRefusal::Hypotheses;
        return p;
    }
    const auto up16 = [](size_t v) { return (v + 15) & ~(size_t)15; };
    p.refused = EpipolarRefusal::None;
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
    p.off_models = p.off_counts + up16(sizeof(int32_t) * (size_t)in.hypotheses);
    p.off_valid = p.off_models + up16(sizeof(float) * 9 * (size_t)in.hypotheses);
    p.bytes = p.off_valid + up16((size_t)in.hypotheses);
    return p;
}

}  // namespace ftk
