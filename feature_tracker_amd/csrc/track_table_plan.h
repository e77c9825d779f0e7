// track_table_plan.h — the launch plan of masked Harris detection and the track table (feature_kernels.hip harris_masked_launch,
// track_table_kernels.hip), as match_plan.h is the matchers': a pure function of values (no context, no environment, no
// HIP call; tests/test_klt_video_args_cpu.py walks it without a device through host/build/track_table_plan_cli).  ftk_track_table.cpp
// plans, the launchers carry the plan out.
#pragma once

#include "ftk_device.h"

namespace ftk {

constexpr int kHarrisRankTile = 256;      // survivors per workgroup of the rank kernel and keys per LDS tile (FTK_HARRIS_RANK_TILE)
constexpr int kTrackRetireBlock = 1024;   // threads of the retire kernel's ONE workgroup (FTK_TRACK_TABLE_BLOCK)
constexpr int kHarrisDeviceMaxSurvivors = 65536;  // FTK_HARRIS_DEVICE_MAX_SURVIVORS
constexpr int kTrackTableMaxSlots = 65536;        // FTK_TRACK_TABLE_MAX_SLOTS
constexpr int kHarrisMinSide = 23;        // 2 * border + 1: below it an image has no valid centre

struct TrackTablePlanInput {
    int32_t rows, cols;    // the image level detection runs on
    int32_t min_distance;
    int32_t n_slots;       // slots of the table, or 0: detection alone
    int32_t n_occupied;    // points that may block candidates (the table's slots, or the caller's list)
};
enum class TrackTableRefusal { None, Sizes, Survivors, Slots };
struct TrackTablePlan {
    TrackTableRefusal refused;  // not None: nothing else is set
    int32_t distance;       // max(min_distance, 1)
    int32_t reach;          // distance - 1
    int32_t capacity;       // entries of the survivor list: ceil(rows / d) * ceil(cols / d), or 0 where the image has no valid centre
    uint32_t image_blocks;  // workgroups of 256 threads of every per-pixel pass
    uint32_t stamp_blocks;  // workgroups of 256 threads of the stamp pass (0: no masking)
    uint32_t rank_blocks;   // workgroups of kHarrisRankTile threads of the rank kernel: one survivor each
    size_t rank_lds;        // bytes of its key tile
    int32_t retire_per_thread;  // consecutive slots a thread of the retire workgroup owns (<= 64: its dead slots are one 64-bit mask)
    size_t retire_lds;      // bytes of its scan array
};
const char *track_table_refusal_name(TrackTableRefusal r);
TrackTablePlan track_table_plan(const TrackTablePlanInput &in);

}  // namespace ftk
