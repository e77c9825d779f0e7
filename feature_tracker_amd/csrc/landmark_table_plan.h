// landmark_table_plan.h — the launch plan of the landmark table (landmark_table_kernels.hip), as pnp_plan.h is PnpRansac's:
// a pure function of values (no context, no environment, no HIP call; tests/test_track_odometry_args_cpu.py walks it without a device
// through host/build/landmark_table_plan_cli).  ftk_landmark_table.cpp plans, the launcher carries the plan out.  The table has no
// workspace: its state is the caller's arrays.
#pragma once

#include "track_table_plan.h"

namespace ftk {

constexpr int kLandmarkBlock = 256;   // FTK_LANDMARK_TABLE_BLOCK: slots of a workgroup, one thread each
constexpr int kLandmarkCounters = 8;  // FTK_LANDMARK_TABLE_COUNTERS: the int32 block below, two unused
// the counters (include/ftk.h): the first three are what TrackOdometry's bootstrap reads in one copy
constexpr int kLandmarkValid = 0, kLandmarkNew = 1, kLandmarkAnchored = 2, kLandmarkCount = 3, kLandmarkDropped = 4, kLandmarkLost = 5;
constexpr int kLandmarkSteady = 0, kLandmarkBootstrap = 1;  // FTK_LANDMARK_TABLE_STEADY / _BOOTSTRAP: the end entry's mode

enum class LandmarkRefusal { None, Sizes, Slots };
struct LandmarkPlan {
    LandmarkRefusal refused;  // not None: nothing else is set
    int32_t launches;         // one per entry
    uint32_t blocks;          // workgroups of kLandmarkBlock slots: the grid of both kernels
};
const char *landmark_refusal_name(LandmarkRefusal r);
LandmarkPlan landmark_table_plan(int32_t n);

struct LandmarkParams {
    const int64_t *ids;       // [n] the track table's
    const float *points;      // [n][2] the track table's
    int32_t n;
    int64_t *owner;           // [n]
    float *landmarks;         // [n][3]
    float *anchor_uv;         // [n][2]
    float *anchor_pose;       // [n][7]
    int32_t *anchor_frame;    // [n]
    uint8_t *pnp_status;      // [n] begin writes it
    uint8_t *anchor_status;   // [n] begin writes it
    int32_t *counters;        // [kLandmarkCounters]
    float *pose;              // [7] the table's pose
    // the end entry alone
    const uint8_t *status_in; // [n] (steady mode; may be pnp_status)
    const float *pose_in;     // [7]
    const int32_t *valid_in;  // [1]
    const int32_t *model_in;  // [1] or null: TwoViewRansac's choice, anything but 0 counts as invalid
    int32_t frame, mode;
    float fx, fy, cx, cy;
    float ry, tn2;            // fy / fx, (threshold / fx)^2: PnpRansac's
    float c2;                 // cos^2 of the parallax floor
};
hipError_t landmark_begin_launch(const LandmarkPlan &plan, const LandmarkParams &p, hipStream_t stream);
hipError_t landmark_end_launch(const LandmarkPlan &plan, const LandmarkParams &p, hipStream_t stream);

}  // namespace ftk
