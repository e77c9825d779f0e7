// track_table_plan_cli — prints the launch plan of masked Harris detection and the track table (csrc/track_table_plan.h) without a device.
// One case per line on stdin:
//   rows cols min_distance n_slots n_occupied
// one line of key=value pairs per case on stdout.  tests/test_klt_video_args_cpu.py drives it.
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>

#include "track_table_plan.h"

int main() {
    std::string text;
    while (std::getline(std::cin, text)) {
        std::istringstream line(text);
        long long v[5] = {0, 0, 0, 0, 0};
        for (long long &e : v) {
            line >> e;
        }
        ftk::TrackTablePlanInput in{};
        in.rows = (int32_t)v[0], in.cols = (int32_t)v[1], in.min_distance = (int32_t)v[2], in.n_slots = (int32_t)v[3], in.n_occupied = (int32_t)v[4];
        const ftk::TrackTablePlan p = ftk::track_table_plan(in);
        printf("refused=%s", ftk::track_table_refusal_name(p.refused));
        if (p.refused == ftk::TrackTableRefusal::None) {
            printf(" distance=%d reach=%d capacity=%d image_blocks=%u stamp_blocks=%u rank_tile=%d rank_blocks=%u rank_lds=%zu retire_block=%d"
                   " retire_per_thread=%d retire_lds=%zu",
                   p.distance, p.reach, p.capacity, p.image_blocks, p.stamp_blocks, ftk::kHarrisRankTile, p.rank_blocks, p.rank_lds, ftk::kTrackRetireBlock,
                   p.retire_per_thread, p.retire_lds);
        }
        printf("\n");
    }
    return 0;
}
