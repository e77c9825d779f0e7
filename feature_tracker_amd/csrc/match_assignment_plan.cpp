// match_assignment_plan.cpp — match_assignment_plan.h's pure function.
#include "match_assignment_plan.h"

namespace ftk {

const char *match_assignment_refusal_name(MatchAssignmentRefusal r) {
    switch (r) {
        case MatchAssignmentRefusal::None: return "none";
        case MatchAssignmentRefusal::Rows: return "rows";
        case MatchAssignmentRefusal::Dim: return "dim";
        case MatchAssignmentRefusal::Stride: return "stride";
    }
    return "?";
}

MatchAssignmentPlan match_assignment_plan(const MatchAssignmentPlanInput &in) {
    MatchAssignmentPlan p{};
    if (in.rows0 < 1 || in.rows1 < 1 || in.rows0 > kAssignMaxRows || in.rows1 > kAssignMaxRows) {
        p.refused = MatchAssignmentRefusal::Rows;
        return p;
    }
    if (in.dim < 1 || in.dim > kAssignMaxDim) {
        p.refused = MatchAssignmentRefusal::Dim;
        return p;
    }
    // (a stride beyond 2^24 floats has no use and would let (M + 1) * stride leave 2^36)
    if (in.row_stride != 0 && (in.row_stride < (int64_t)in.rows1 + 1 || in.row_stride > (int64_t)1 << 24)) {
        p.refused = MatchAssignmentRefusal::Stride;
        return p;
    }
    const auto tiles = [](int64_t n, int64_t per) { return (uint32_t)((n + per - 1) / per); };
    const size_t m = (size_t)in.rows0, n = (size_t)in.rows1, d = (size_t)in.dim;
    const bool w = in.with_weights != 0;
    p.refused = MatchAssignmentRefusal::None;
    p.row_stride = in.row_stride != 0 ? in.row_stride : (int64_t)in.rows1 + 1;
    p.vec = (in.dim % 4 == 0 && in.aligned16 != 0) ? 1 : 0;
    p.project_grid_x = w ? tiles(in.rows0 + in.rows1, kAssignGemmTileRows) : 0;
    p.project_grid_y = w ? tiles(in.dim + 1, kAssignGemmTileCols) : 0;
    p.sim_grid_x = tiles(in.rows0, kAssignGemmTileRows);
    p.sim_grid_y = tiles(in.rows1, kAssignGemmTileCols);
    p.norm_row_blocks = (uint32_t)in.rows0;
    p.norm_col_blocks = tiles(in.rows1, kAssignNormCols);
    p.norm_lds = sizeof(float) * 64 * kAssignNormLdsStride;
    p.finish_grid_x = tiles(in.rows1 + 1, kAssignFinishThreads);
    p.finish_grid_y = tiles(in.rows0 + 1, kAssignFinishRows);
    p.launches = w ? 4 : 3;
    ftk_layout16 ws;  // cannot wrap: (M + N) D <= 2^23
    p.md = ws.take<float>(w ? (m + n) * d : 0);
    p.z = ws.take<float>(w ? m + n : 0);
    p.lse_row = ws.take<float>(m);
    p.lse_col = ws.take<float>(n);
    p.ls0 = ws.take<float>(w ? 2 * m : 0);
    p.ls1 = ws.take<float>(w ? 2 * n : 0);
    p.bytes = ws.bytes();
    return p;
}

}  // namespace ftk
