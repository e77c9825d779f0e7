// two_view_plan_cli — prints the launch plan and workspace layout of two-view outlier rejection with a choice of model
// (csrc/two_view_plan.h, with two slots) without a device.  One case per line on stdin:
//   n hypotheses image_rows image_cols mode prefer_permille
// one line of key=value pairs per case on stdout.  tests/test_two_view_args_cpu.py drives it.
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>

#include "two_view_plan.h"

int main() {
    std::string text;
    while (std::getline(std::cin, text)) {
        std::istringstream line(text);
        long long v[6] = {0, 0, 0, 0, 0, 0};
        for (long long &e : v) {
            line >> e;
        }
        ftk::TwoViewPlanInput in{};
        in.n = (int32_t)v[0], in.hypotheses = (int32_t)v[1], in.image_rows = (int32_t)v[2], in.image_cols = (int32_t)v[3];
        in.slots = 2, in.mode = (int32_t)v[4], in.prefer_permille = (int32_t)v[5];
        const ftk::TwoViewPlan p = ftk::two_view_plan(in);
        printf("refused=%s", ftk::two_view_refusal_name(p.refused));
        if (p.refused == ftk::TwoViewRefusal::None) {
            printf(" run_fundamental=%d run_homography=%d launches=%d scan_block=%d scan_per_thread=%d hyp_block=%d hyp_blocks=%u hyp_lds=%zu score_tile=%d"
                   " score_group=%d score_tiles=%u score_groups=%u score_lds=%zu select_per_thread=%d off_points=%zu off_list=%zu off_counts=%zu"
                   " off_models=%zu off_valid=%zu bytes=%zu",
                   p.run_fundamental, p.run_homography, p.launches, ftk::kEpipolarScanBlock, p.scan_per_thread, ftk::kEpipolarHypBlock, p.hyp_blocks,
                   p.hyp_lds, ftk::kEpipolarScoreTile, ftk::kEpipolarScoreGroup, p.score_tiles, p.score_groups, p.score_lds, p.select_per_thread,
                   p.points.offset, p.list.offset, p.counts.offset, p.models.offset, p.valid.offset, p.bytes);
        }
        printf("\n");
    }
    return 0;
}
