// keypoint_decode_plan_cli — prints the launch plan and workspace layout of the keypoint decoder (csrc/keypoint_decode_plan.h) without a
// device.  One case per line on stdin:
//   cell_rows cell_cols channels max_keypoints min_distance border n_occupied
// one line of key=value pairs per case on stdout.  tests/test_keypoint_decode_args_cpu.py drives it.
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>

#include "keypoint_decode_plan.h"

int main() {
    std::string text;
    while (std::getline(std::cin, text)) {
        std::istringstream line(text);
        long long v[7] = {0, 0, 0, 0, 0, 0, 0};
        for (long long &e : v) {
            line >> e;
        }
        ftk::KeypointDecodePlanInput in{};
        in.cell_rows = (int32_t)v[0], in.cell_cols = (int32_t)v[1], in.channels = (int32_t)v[2], in.max_keypoints = (int32_t)v[3];
        in.min_distance = (int32_t)v[4], in.border = (int32_t)v[5], in.n_occupied = (int32_t)v[6];
        const ftk::KeypointDecodePlan p = ftk::keypoint_decode_plan(in);
        printf("refused=%s", ftk::keypoint_decode_refusal_name(p.refused));
        if (p.refused == ftk::KeypointDecodeRefusal::None) {
            printf(" rows=%d cols=%d distance=%d reach=%d capacity=%d score_tile=%d score_grid_x=%u score_grid_y=%u score_lds=%zu image_blocks=%u"
                   " stamp_blocks=%u rank_tile=%d rank_blocks=%u describe_waves=%d describe_blocks=%u launches=%d memsets=%d off_tmp=%zu off_wmax=%zu"
                   " off_list=%zu off_count=%zu off_plane=%zu off_dilated=%zu bytes=%zu",
                   p.rows, p.cols, p.distance, p.reach, p.capacity, ftk::kKeypointScoreTile, p.score_grid_x, p.score_grid_y, p.score_lds, p.image_blocks,
                   p.stamp_blocks, ftk::kKeypointRankTile, p.rank_blocks, ftk::kKeypointDescribeWaves, p.describe_blocks, p.launches, p.memsets,
                   p.tmp.offset, p.wmax.offset, p.list.offset, p.count.offset, p.plane.offset, p.dilated.offset, p.bytes);
        }
        printf("\n");
    }
    return 0;
}
