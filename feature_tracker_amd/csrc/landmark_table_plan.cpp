// landmark_table_plan.cpp — landmark_table_plan.h's pure function.
#include "landmark_table_plan.h"

namespace ftk {

const char *landmark_refusal_name(LandmarkRefusal r) {
    switch (r) {
        case LandmarkRefusal::None: return "none";
        case LandmarkRefusal::Sizes: return "sizes";
        case LandmarkRefusal::Slots: return "slots";
    }
    return "?";
}

LandmarkPlan landmark_table_plan(int32_t n) {
    LandmarkPlan p{};
    if (n < 1) {
        p.refused = LandmarkRefusal::Sizes;
        return p;
    }
    if (n > kTrackTableMaxSlots) {
        p.refused = LandmarkRefusal::Slots;
        return p;
    }
    p.refused = LandmarkRefusal::None;
    p.launches = 1;
    p.blocks = (uint32_t)((n + kLandmarkBlock - 1) / kLandmarkBlock);
    return p;
}

}  // namespace ftk
