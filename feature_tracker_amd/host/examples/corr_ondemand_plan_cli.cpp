// corr_ondemand_plan_cli — prints the workspace layout and launch plan of the on-demand correlation (csrc/raft_corr_ondemand_plan.h) without a
// device.  One case per line on stdin:
//   B C H W levels radius [aligned16]
// (aligned16 defaults to 1) one line of key=value pairs per case on stdout.  tests/test_raft_corr_ondemand_cpu.py drives it.
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>

#include "raft_corr_ondemand_plan.h"

int main() {
    std::string text;
    while (std::getline(std::cin, text)) {
        std::istringstream line(text);
        long long v[6] = {0, 0, 0, 0, 0, 0}, aligned = 1;
        for (long long &e : v) {
            line >> e;
        }
        long long seventh = 0;
        if (line >> seventh) {
            aligned = seventh;
        }
        ftk::CorrOdPlanInput in{};
        in.B = (int32_t)v[0], in.C = (int32_t)v[1], in.H = (int32_t)v[2], in.W = (int32_t)v[3], in.levels = (int32_t)v[4], in.radius = (int32_t)v[5];
        in.aligned16 = (int32_t)aligned;
        const ftk::CorrOdPlan p = ftk::raft_corr_ondemand_plan(in);
        printf("refused=%s", ftk::corr_od_refusal_name(p.refused));
        if (p.refused == ftk::CorrOdRefusal::EmptyLevel) {
            printf(" empty_level=%d", p.empty_level);
        }
        if (p.refused == ftk::CorrOdRefusal::None) {
            printf(" elements=%lld side=%d samples=%d sample_passes=%d lattice_side=%d lattice_points=%d lattice_passes=%d vector=%d lds=%zu"
                   " lattice_floats=%d transpose_grid=%ux%ux%u transpose_block=%ux%u lookup_grid=%ux%ux%u lookup_block=%u",
                   (long long)p.elements, p.side, p.samples, p.sample_passes, p.lattice_side, p.lattice_points, p.lattice_passes, p.vector, p.lds,
                   ftk::kCorrOdLatticeFloats, p.transpose_grid.x, p.transpose_grid.y, p.transpose_grid.z, p.transpose_block.x, p.transpose_block.y,
                   p.lookup_grid.x, p.lookup_grid.y, p.lookup_grid.z, p.lookup_block.x);
            for (int l = 0; l < in.levels; ++l) {
                printf(" level%d=%dx%d@%lld/%lld", l, p.level_h[l], p.level_w[l], (long long)p.level_offset[l], (long long)p.pool_blocks[l]);
            }
        }
        printf("\n");
    }
    return 0;
}
