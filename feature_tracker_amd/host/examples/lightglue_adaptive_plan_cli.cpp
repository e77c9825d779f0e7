// lightglue_adaptive_plan_cli — prints the launch plan and workspace layout of LightGlue's adaptive pass
// (csrc/lightglue_adaptive_plan.h) without a device.  One case per line on stdin:
//   rows0 rows1 dim heads
// one line of key=value pairs per case on stdout.  tests/test_lightglue_adaptive_args_cpu.py drives it.
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>

#include "lightglue_adaptive_plan.h"

int main() {
    std::string text;
    while (std::getline(std::cin, text)) {
        std::istringstream line(text);
        long long v[4] = {0, 0, 0, 0};
        for (long long &e : v) {
            line >> e;
        }
        const ftk::LightglueAdaptivePlan p =
            ftk::lightglue_adaptive_plan(ftk::LightglueAdaptivePlanInput{(int32_t)v[0], (int32_t)v[1], (int32_t)v[2], (int32_t)v[3]});
        printf("refused=%s", ftk::lightglue_adaptive_refusal_name(p.refused));
        if (p.refused == ftk::LightglueAdaptiveRefusal::None) {
            printf(" conf_threads=%d conf_blocks=%u decide_threads=%d decide_blocks=%u gather_threads=%d gather_blocks=%u copy_threads=%d"
                   " select_blocks=%u remap_blocks=%u step_launches=%d finish_launches=%d off_layer=%zu off_assign=%zu off_head_w=%zu off_head_b=%zu"
                   " off_src0=%zu off_src1=%zu off_match=%zu off_status=%zu bytes=%zu",
                   ftk::kAdaptiveConfThreads, p.conf_blocks, ftk::kAdaptiveDecideThreads, p.decide_blocks, ftk::kAdaptiveGatherThreads, p.gather_blocks,
                   ftk::kAdaptiveCopyThreads, p.select_blocks, p.remap_blocks, p.step_launches, p.finish_launches, p.layer.offset, p.assign.offset,
                   p.head_w.offset, p.head_b.offset, p.src0.offset, p.src1.offset, p.match.offset, p.status.offset, p.bytes);
        }
        printf("\n");
    }
    return 0;
}
