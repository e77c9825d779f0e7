// lightglue_adaptive_plan.cpp — lightglue_adaptive_plan.h's pure functions.
#include "lightglue_adaptive_plan.h"

#include "match_assignment_plan.h"
#include "transformer_plan.h"

namespace ftk {

const char *lightglue_adaptive_refusal_name(LightglueAdaptiveRefusal r) {
    switch (r) {
        case LightglueAdaptiveRefusal::None: return "none";
        case LightglueAdaptiveRefusal::Layer: return "layer";
        case LightglueAdaptiveRefusal::Assignment: return "assignment";
    }
    return "?";
}

uint32_t lightglue_confidence_blocks(int64_t rows) { return (uint32_t)((rows + kAdaptiveConfThreads - 1) / kAdaptiveConfThreads); }

LightglueAdaptivePlan lightglue_adaptive_plan(const LightglueAdaptivePlanInput &in) {
    LightglueAdaptivePlan p{};
    const TransformerPlan layer = transformer_plan(TransformerPlanInput{in.rows0, in.rows1, in.dim, in.heads, 0});
    if (layer.refused != TransformerRefusal::None) {
        p.refused = LightglueAdaptiveRefusal::Layer;
        return p;
    }
    MatchAssignmentPlanInput head{};
    head.rows0 = in.rows0, head.rows1 = in.rows1, head.dim = in.dim, head.with_weights = 1;
    const MatchAssignmentPlan assign = match_assignment_plan(head);
    if (assign.refused != MatchAssignmentRefusal::None) {
        p.refused = LightglueAdaptiveRefusal::Assignment;
        return p;
    }
    p.refused = LightglueAdaptiveRefusal::None;
    const auto tiles = [](size_t n, size_t per) { return (uint32_t)((n + per - 1) / per); };
    const size_t m = (size_t)in.rows0, n = (size_t)in.rows1, r = m + n, d = (size_t)in.dim;
    p.conf_blocks = lightglue_confidence_blocks((int64_t)r);
    p.decide_blocks = 1;
    p.gather_blocks = (uint32_t)r;
    const uint32_t select = tiles((d + 1) * d + d + 1 + m, kAdaptiveCopyThreads);
    p.select_blocks = select < (uint32_t)kAdaptiveCopyMaxBlocks ? select : (uint32_t)kAdaptiveCopyMaxBlocks;
    p.remap_blocks = tiles(r, kAdaptiveCopyThreads);
    p.step_launches = 3;
    p.finish_launches = 2;
    ftk_layout16 ws;  // cannot wrap: the two plans accepted these sizes, and theirs are the largest blocks
    p.layer = ws.take<uint8_t>(layer.bytes);
    p.assign = ws.take<uint8_t>(assign.bytes);
    p.head_w = ws.take<float>((d + 1) * d);
    p.head_b = ws.take<float>(d + 1);
    p.src0 = ws.take<int32_t>(m);
    p.src1 = ws.take<int32_t>(n);
    p.match = ws.take<int32_t>(m);
    p.status = ws.take<uint8_t>(m);
    p.bytes = ws.bytes();
    return p;
}

}  // namespace ftk
