// pnp_plan.cpp — pnp_plan.h's pure function.
#include "pnp_plan.h"

namespace ftk {

const char *pnp_refusal_name(PnpRefusal r) {
    switch (r) {
        case PnpRefusal::None: return "none";
        case PnpRefusal::Sizes: return "sizes";
        case PnpRefusal::Points: return "points";
        case PnpRefusal::Hypotheses: return "hypotheses";
        case PnpRefusal::Refine: return "refine";
        case PnpRefusal::Sampler: return "sampler";
    }
    return "?";
}

PnpPlan pnp_plan(const PnpPlanInput &in) {
    PnpPlan p{};
    if (in.n < 1 || in.hypotheses < 1 || in.refine_iterations < 0) {
        p.refused = PnpRefusal::Sizes;
        return p;
    }
    if (in.refine_iterations > kPnpMaxRefine) {
        p.refused = PnpRefusal::Refine;
        return p;
    }
    if (in.n > kEpipolarMaxPoints) {
        p.refused = PnpRefusal::Points;
        return p;
    }
    if (in.hypotheses > kEpipolarMaxHypotheses) {
        p.refused = PnpRefusal::Hypotheses;
        return p;
    }
    if (in.sampler != PnpSample::Dlt6 && in.sampler != PnpSample::P3p) {
        p.refused = PnpRefusal::Sampler;
        return p;
    }
    p.refused = PnpRefusal::None;
    p.sampler = in.sampler;
    p.sample = in.sampler == PnpSample::P3p ? kP3pSample : kPnpSample;
    p.refine_iterations = in.refine_iterations;
    p.launches = 5 + 2 * in.refine_iterations;
    p.scan_per_thread = (in.n + kEpipolarScanBlock - 1) / kEpipolarScanBlock;
    p.hyp_blocks = (uint32_t)((in.hypotheses + kEpipolarHypBlock - 1) / kEpipolarHypBlock);
    p.hyp_lds = in.sampler == PnpSample::P3p ? 0 : sizeof(float) * kPnpHypLdsFloats * kEpipolarHypBlock;
    p.score_tiles = (uint32_t)((in.n + kEpipolarScoreTile - 1) / kEpipolarScoreTile);
    p.score_groups = (uint32_t)((in.hypotheses + kEpipolarScoreGroup - 1) / kEpipolarScoreGroup);
    p.select_per_thread = (in.hypotheses + kEpipolarScanBlock - 1) / kEpipolarScanBlock;
    p.tiles = (uint32_t)((in.n + kPoseTile - 1) / kPoseTile);
    p.sums_lds = sizeof(float) * kPnpSums * kPoseTile;
    const size_t n = (size_t)in.n, k = (size_t)in.hypotheses;
    ftk_layout16 ws;  // cannot wrap: n <= 2^16, hypotheses <= 2^12
    p.m = ws.take<int32_t>(1);
    p.points = ws.take<float4>(n);
    p.depth = ws.take<float>(n);
    p.list = ws.take<int32_t>(n);
    p.counts = ws.take<int32_t>(k);
    p.models = ws.take<float>(kPnpModelFloats * k);
    p.valid = ws.take<uint8_t>(k);
    p.totals = ws.take<float>(kPnpSums * (size_t)p.tiles);
    p.tile_counts = ws.take<int32_t>(p.tiles);
    p.state = ws.take<float>(kPnpStateFloats);
    p.flags = ws.take<int32_t>(kPnpFlags);
    p.bytes = ws.bytes();
    return p;
}

}  // namespace ftk
