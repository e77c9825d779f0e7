// landmark_table_plan_cli — prints the launch plan of the landmark table (csrc/landmark_table_plan.h) without a device.  One case per
// line on stdin:
//   n
// one line of key=value pairs per case on stdout.  tests/test_track_odometry_args_cpu.py drives it.
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>

#include "landmark_table_plan.h"

int main() {
    std::string text;
    while (std::getline(std::cin, text)) {
        std::istringstream line(text);
        long long n = 0;
        line >> n;
        const ftk::LandmarkPlan p = ftk::landmark_table_plan((int32_t)n);
        printf("refused=%s", ftk::landmark_refusal_name(p.refused));
        if (p.refused == ftk::LandmarkRefusal::None) {
            printf(" launches=%d block=%d blocks=%u counters=%d", p.launches, ftk::kLandmarkBlock, p.blocks, ftk::kLandmarkCounters);
        }
        printf("\n");
    }
    return 0;
}
