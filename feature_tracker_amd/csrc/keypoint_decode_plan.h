// keypoint_decode_plan.h — the launch plan and workspace layout of the keypoint decoder (keypoint_decode_kernels.hip), as
// two_view_plan.h is two-view outlier rejection's: a pure function of values (no context, no environment, no HIP call;
// tests/test_keypoint_decode_args_cpu.py walks it without a device through host/build/keypoint_decode_plan_cli).
// ftk_keypoint_decode.cpp plans, the launcher carries the plan out.
#pragma once

#include "ftk_device.h"
#include "ftk_layout.h"

namespace ftk {

constexpr int kKeypointCell = 8;              // FTK_KEYPOINT_DECODE_CELL: fine pixels per cell side
constexpr int kKeypointLogits = 65;           // 64 pixels of a cell and the dustbin
constexpr int kKeypointMaxSide = 65536;       // H, W
constexpr int kKeypointMaxKeypoints = 65536;  // FTK_KEYPOINT_DECODE_MAX_KEYPOINTS
constexpr int kKeypointMaxChannels = 1024;    // FTK_KEYPOINT_DECODE_MAX_CHANNELS
constexpr int kKeypointMaxSurvivors = 65536;  // FTK_HARRIS_DEVICE_MAX_SURVIVORS
constexpr int kKeypointScoreTile = 64;        // cells (lanes) of a score workgroup: one wave along cx
constexpr int kKeypointScoreStride = 68;      // floats between the LDS rows of two logits: 64 cells + 4, so that a transposed read's
                                              // bank (4 (lane % 8) + lane / 8) mod 32 is distinct within each half wave
constexpr int kKeypointDescribeWaves = 4;     // output rows (waves) of a describe workgroup
constexpr int kKeypointRankTile = 256;        // FTK_HARRIS_RANK_TILE
constexpr int kKeypointLaneChannels = kKeypointMaxChannels / 64;

struct KeypointDecodePlanInput {
    int32_t cell_rows, cell_cols;  // Hc, Wc
    int32_t channels;              // D
    int32_t max_keypoints;
    int32_t min_distance;
    int32_t border;
    int32_t n_occupied;            // points that may block candidates; 0: none
};
enum class KeypointDecodeRefusal { None, Sizes, Survivors, Keypoints, Channels };
struct KeypointDecodePlan {
    KeypointDecodeRefusal refused;  // not None: nothing else is set
    int32_t rows, cols;             // H, W
    int32_t distance, reach;        // max(min_distance, 1) and that - 1
    int32_t capacity;               // entries of the survivor list: ceil(H / d) * ceil(W / d)
    uint32_t score_grid_x, score_grid_y;  // workgroups of kKeypointScoreTile threads: tiles of 64 cells along a cell row, cell rows
    size_t score_lds;
    uint32_t image_blocks;          // workgroups of 256 threads of every per-pixel pass
    uint32_t stamp_blocks;          // of the stamp pass (0: no masking)
    uint32_t rank_blocks;           // workgroups of kKeypointRankTile threads of the rank kernel
    uint32_t describe_blocks;       // workgroups of kKeypointDescribeWaves waves: one wave per output row
    int32_t launches;               // kernels: score, [stamp, dilate, block], 2 window maxima, collect, rank, describe: 7 or 10
    int32_t memsets;                // uv, scores, the survivor count, [the stamp plane]: 3 or 4
    // the workspace (ftk_layout.h), in this order: the key plane and the two window-maximum planes [H][W], the survivor list [capacity], its
    // count, and with occupied points (count 0 without) the stamp plane and its row dilation [H][W]
    ftk_slot16<unsigned long long> key, tmp, wmax, list;
    ftk_slot16<unsigned> count;
    ftk_slot16<uint8_t> plane, dilated;
    size_t bytes;
};
const char *keypoint_decode_refusal_name(KeypointDecodeRefusal r);
KeypointDecodePlan keypoint_decode_plan(const KeypointDecodePlanInput &in);

struct KeypointScoreParams {
    const float *semi;             // [65][Hc][Wc]
    int32_t cell_rows, cell_cols;
    float min_score;
    int32_t border;
    unsigned long long *key;       // [H][W]
    float *heatmap;                // [H][W] or null
};
struct KeypointDescribeParams {
    const float *desc;
    long long stride_c, stride_y, stride_x;  // elements
    int32_t cell_rows, cell_cols, channels;
    const float *uv;               // [max_keypoints][2] the rank kernel's rows
    const int32_t *count;          // [1] how many of them are keypoints (device word)
    int32_t max_keypoints;
    float *descriptors;            // [max_keypoints][channels]
};
// One call: the memsets and launches of the plan, in stream order.  `select` and `occupied` carry the workspace pointers.
struct KeypointDecodeParams {
    KeypointScoreParams score;
    KeyPlaneSelectParams select;
    HarrisOccupied occupied;
    HarrisRankParams rank;
    KeypointDescribeParams describe;
};
hipError_t keypoint_decode_launch(const KeypointDecodePlan &plan, const KeypointDecodeParams &p, hipStream_t stream);

}  // namespace ftk
