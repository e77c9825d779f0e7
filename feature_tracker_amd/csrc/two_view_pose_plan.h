// two_view_pose_plan.h — the launch plan and workspace layout of TwoViewPose (two_view_pose_kernels.hip), as two_view_plan.h
// is the two filters': a pure function of values (no context, no environment, no HIP call).  ftk_two_view_pose.cpp plans, the launcher
// carries the plan out.
#pragma once

#include "two_view_plan.h"

namespace ftk {

constexpr int kPoseTile = 256;          // participants of a tile of the summation tree = threads of the moment, count and finish kernels
constexpr int kPoseMoments = 45;        // distinct entries of the symmetric 9 x 9 matrix, upper triangle in row-major order
constexpr int kPoseSolveBlock = 64;     // threads of the solve kernel's ONE workgroup: one wave
constexpr int kPoseJacobiSweeps = 7;    // FTK_POSE_JACOBI_SWEEPS
constexpr float kPoseRankFloor = 9.5367431640625e-07f;  // 2^-20: the second-smallest eigenvalue of A must exceed this share of the largest
constexpr int kPoseModelFloats = 32;   // the solve kernel's result in the workspace: Ehat 9, Ra 9, Rb 9, t 3, ok, one unused

struct TwoViewPosePlanInput {
    int32_t n;  // correspondences
};
enum class TwoViewPoseRefusal { None, Sizes, Points };
struct TwoViewPosePlan {
    TwoViewPoseRefusal refused;  // not None: nothing else is set
    int32_t launches;            // scan, moments, solve, count, finish: 5
    int32_t scan_per_thread;     // consecutive points a thread of the scan workgroup owns (<= 64)
    uint32_t tiles;              // grid of the moment, count and finish kernels: tiles of kPoseTile, sized for n (M is on the device)
    size_t moment_lds;           // bytes of a tile's 45 x 256 tree
    // the workspace (ftk_layout.h), in this order: M, the participants' calibrated (x1, y1, x2, y2) [n], the tile totals [tiles][45], the
    // model block [kPoseModelFloats]
    ftk_slot16<int32_t> m;
    ftk_slot16<float4> points;
    ftk_slot16<float> totals, model;
    size_t bytes;
};
const char *two_view_pose_refusal_name(TwoViewPoseRefusal r);
TwoViewPosePlan two_view_pose_plan(const TwoViewPosePlanInput &in);

struct TwoViewPoseParams {
    const float *ref_uv, *cur_uv;  // [n][2]
    uint8_t *status;               // [n]
    int32_t n;
    float fx1, fy1, cx1, cy1;      // the reference view's camera
    float fx2, fy2, cx2, cy2;      // the current view's
    float t2;                      // the squared threshold, pixels
    float baseline;
    int32_t *m;                    // [1] workspace: the number of participants
    float4 *points;                // [n] workspace: participant j's calibrated (x1, y1, x2, y2)
    float *totals;                 // [tiles][45] workspace
    float *model;                  // [kPoseModelFloats] workspace
    float *pose;                   // [7]
    float *landmarks;              // [n][3]
    float *E;                      // [9]
    int32_t *n_front;              // [4]
    int32_t *valid, *n_points;     // [1] each
    int32_t scan_per_thread;
};
hipError_t two_view_pose_launch(const TwoViewPosePlan &plan, const TwoViewPoseParams &p, hipStream_t stream);

}  // namespace ftk
