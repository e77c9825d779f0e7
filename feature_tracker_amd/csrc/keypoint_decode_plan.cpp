// keypoint_decode_plan.cpp — keypoint_decode_plan.h's pure function.
#include "keypoint_decode_plan.h"

namespace ftk {

const char *keypoint_decode_refusal_name(KeypointDecodeRefusal r) {
    switch (r) {
        case KeypointDecodeRefusal::None: return "none";
        case KeypointDecodeRefusal::Sizes: return "sizes";
        case KeypointDecodeRefusal::Survivors: return "survivors";
        case KeypointDecodeRefusal::Keypoints: return "keypoints";
        case KeypointDecodeRefusal::Channels: return "channels";
    }
    return "?";
}

KeypointDecodePlan keypoint_decode_plan(const KeypointDecodePlanInput &in) {
    KeypointDecodePlan p{};
    constexpr int max_cells = kKeypointMaxSide / kKeypointCell;
    if (in.cell_rows < 1 || in.cell_cols < 1 || in.cell_rows > max_cells || in.cell_cols > max_cells || in.border < 0 || in.n_occupied < 0) {
        p.refused = KeypointDecodeRefusal::Sizes;
        return p;
    }
    if (in.channels < 1 || in.channels > kKeypointMaxChannels) {
        p.refused = KeypointDecodeRefusal::Channels;
        return p;
    }
    if (in.max_keypoints < 1 || in.max_keypoints > kKeypointMaxKeypoints) {
        p.refused = KeypointDecodeRefusal::Keypoints;
        return p;
    }
    const int32_t rows = in.cell_rows * kKeypointCell, cols = in.cell_cols * kKeypointCell;
    const int32_t d = in.min_distance > 1 ? in.min_distance : 1;
    // survivors are pairwise at Chebyshev distance >= d: at most one per d x d cell of the image
    const int64_t bound = (((int64_t)rows + d - 1) / d) * (((int64_t)cols + d - 1) / d);
    if (bound > kKeypointMaxSurvivors) {
        p.refused = KeypointDecodeRefusal::Survivors;
        return p;
    }
    const size_t px = (size_t)rows * cols;
    p.refused = KeypointDecodeRefusal::None;
    p.rows = rows;
    p.cols = cols;
    p.distance = d;
    p.reach = d - 1;
    p.capacity = (int32_t)bound;
    p.score_grid_x = (uint32_t)((in.cell_cols + kKeypointScoreTile - 1) / kKeypointScoreTile);
    p.score_grid_y = (uint32_t)in.cell_rows;
    p.score_lds = sizeof(float) * 64 * kKeypointScoreStride;
    p.image_blocks = (uint32_t)((px + 255) / 256);
    p.stamp_blocks = (uint32_t)((in.n_occupied + 255) / 256);
    p.rank_blocks = (uint32_t)((p.capacity + kKeypointRankTile - 1) / kKeypointRankTile);
    p.describe_blocks = (uint32_t)((in.max_keypoints + kKeypointDescribeWaves - 1) / kKeypointDescribeWaves);
    p.launches = in.n_occupied > 0 ? 10 : 7;
    p.memsets = in.n_occupied > 0 ? 4 : 3;
    const size_t occupied_px = in.n_occupied > 0 ? px : 0;
    ftk_layout16 ws;  // cannot wrap: px <= 2^32
    p.key = ws.take<unsigned long long>(px);
    p.tmp = ws.take<unsigned long long>(px);
    p.wmax = ws.take<unsigned long long>(px);
    p.list = ws.take<unsigned long long>((size_t)p.capacity);
    p.count = ws.take<unsigned>(1);
    p.plane = ws.take<uint8_t>(occupied_px);
    p.dilated = ws.take<uint8_t>(occupied_px);
    p.bytes = ws.bytes();
    return p;
}

}  // namespace ftk
