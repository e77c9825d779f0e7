// match_assignment_plan_cli — prints the launch plan and workspace layout of the assignment head (csrc/match_assignment_plan.h) without a
// device.  One case per line on stdin:
//   rows0 rows1 dim with_weights row_stride aligned16
// one line of key=value pairs per case on stdout.  tests/test_match_assignment_args_cpu.py drives it.
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>

#include "match_assignment_plan.h"

int main() {
    std::string text;
    while (std::getline(std::cin, text)) {
        std::istringstream line(text);
        long long v[6] = {0, 0, 0, 0, 0, 0};
        for (long long &e : v) {
            line >> e;
        }
        ftk::MatchAssignmentPlanInput in{};
        in.rows0 = (int32_t)v[0], in.rows1 = (int32_t)v[1], in.dim = (int32_t)v[2], in.with_weights = (int32_t)v[3];
        in.row_stride = (int64_t)v[4], in.aligned16 = (int32_t)v[5];
        const ftk::MatchAssignmentPlan p = ftk::match_assignment_plan(in);
        printf("refused=%s", ftk::match_assignment_refusal_name(p.refused));
        if (p.refused == ftk::MatchAssignmentRefusal::None) {
            printf(" row_stride=%lld vec=%d gemm_threads=%d project_grid_x=%u project_grid_y=%u sim_grid_x=%u sim_grid_y=%u norm_threads=%d"
                   " norm_row_blocks=%u norm_col_blocks=%u norm_lds=%zu finish_threads=%d finish_grid_x=%u finish_grid_y=%u launches=%d off_md=%zu"
                   " off_z=%zu off_lse_row=%zu off_lse_col=%zu off_ls0=%zu off_ls1=%zu bytes=%zu",
                   (long long)p.row_stride, p.vec, 64 * ftk::kAssignGemmWaves, p.project_grid_x, p.project_grid_y, p.sim_grid_x, p.sim_grid_y,
                   ftk::kAssignNormThreads, p.norm_row_blocks, p.norm_col_blocks, p.norm_lds, ftk::kAssignFinishThreads, p.finish_grid_x,
                   p.finish_grid_y, p.launches, p.md.offset, p.z.offset, p.lse_row.offset, p.lse_col.offset, p.ls0.offset, p.ls1.offset, p.bytes);
        }
        printf("\n");
    }
    return 0;
}
