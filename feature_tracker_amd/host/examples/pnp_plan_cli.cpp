// pnp_plan_cli — prints the launch plan and workspace layout of PnpRansac (csrc/pnp_plan.h) without a device.  One case per line on stdin:
//   n hypotheses refine_iterations [sampler]
// one line of key=value pairs per case on stdout; with a sampler (0: dlt6, 1: p3p) the line also ends in sampler= and sample=.  tests/test_pnp_args_cpu.py drives it.
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>

#include "pnp_plan.h"

int main() {
    std::string text;
    while (std::getline(std::cin, text)) {
        std::istringstream line(text);
        long long v[3] = {0, 0, 0};
        for (long long &e : v) {
            line >> e;
        }
        long long sampler = 0;
        const bool sampled = static_cast<bool>(line >> sampler);
        ftk::PnpPlanInput in{};
        in.n = (int32_t)v[0], in.hypotheses = (int32_t)v[1], in.refine_iterations = (int32_t)v[2];
        in.sampler = static_cast<ftk::PnpSample>((int32_t)sampler);
        const ftk::PnpPlan p = ftk::pnp_plan(in);
        printf("refused=%s", ftk::pnp_refusal_name(p.refused));
        if (p.refused == ftk::PnpRefusal::None) {
            printf(" launches=%d scan_block=%d scan_per_thread=%d hyp_block=%d hyp_blocks=%u hyp_lds=%zu score_tile=%d score_group=%d score_tiles=%u"
                   " score_groups=%u select_per_thread=%d tile=%d tiles=%u sums_lds=%zu off_points=%zu off_depth=%zu off_list=%zu off_counts=%zu"
                   " off_models=%zu off_valid=%zu off_totals=%zu off_tile_counts=%zu off_state=%zu off_flags=%zu bytes=%zu",
                   p.launches, ftk::kEpipolarScanBlock, p.scan_per_thread, ftk::kEpipolarHypBlock, p.hyp_blocks, p.hyp_lds, ftk::kEpipolarScoreTile,
                   ftk::kEpipolarScoreGroup, p.score_tiles, p.score_groups, p.select_per_thread, ftk::kPoseTile, p.tiles, p.sums_lds, p.points.offset,
                   p.depth.offset, p.list.offset, p.counts.offset, p.models.offset, p.valid.offset, p.totals.offset, p.tile_counts.offset, p.state.offset,
                   p.flags.offset, p.bytes);
            if (sampled) {
                printf(" sampler=%d sample=%d", (int)p.sampler, p.sample);
            }
        }
        printf("\n");
    }
    return 0;
}
