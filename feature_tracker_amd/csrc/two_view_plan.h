// two_view_plan.h — the launch plan and workspace layout of two-view outlier rejection (two_view_kernels.hip), as
// track_table_plan.h is the track table's: a pure function of values (no context, no environment, no HIP call;
// tests/test_epipolar_args_cpu.py and tests/test_two_view_args_cpu.py walk it without a device through host/build/epipolar_plan_cli and
// host/build/two_view_plan_cli).  ftk_two_view.cpp plans, the launcher carries the plan out.  The fundamental-only entry (5.20) is the
// plan with ONE slot; the entry with a choice of model (5.21) has two.
#pragma once

#include "ftk_device.h"
#include "ftk_layout.h"

namespace ftk {

constexpr int kEpipolarMaxHypotheses = 4096;  // FTK_EPIPOLAR_MAX_HYPOTHESES
constexpr int kEpipolarMaxPoints = 65536;     // FTK_TRACK_TABLE_MAX_SLOTS
constexpr int kEpipolarMaxSide = 65536;       // image rows / cols: W + H is then exact in float32
constexpr int kEpipolarSample = 8;            // FTK_EPIPOLAR_SAMPLE
constexpr int kEpipolarMaxAttempts = 16;      // FTK_EPIPOLAR_MAX_ATTEMPTS
constexpr int kEpipolarScanBlock = 1024;      // threads of the scan kernel's ONE workgroup, and of the select kernel's
constexpr int kEpipolarHypBlock = 64;         // hypotheses (= lanes) per workgroup of the hypothesis kernel: one wave
constexpr int kEpipolarHypLdsFloats = 90;     // per lane: the 8 x 9 matrix, the 9 column indices, the 9 entries of f
constexpr int kEpipolarScoreTile = 256;       // participants per workgroup of the scoring kernel (FTK_EPIPOLAR_SCORE_TILE) = its threads
constexpr int kEpipolarScoreGroup = 16;       // hypotheses per workgroup of the scoring kernel: 4 per wave
constexpr int kTwoViewFundamental = 0;        // FTK_TWO_VIEW_FUNDAMENTAL: the mode, the model chosen and the model's slot
constexpr int kTwoViewHomography = 1;         // FTK_TWO_VIEW_HOMOGRAPHY
constexpr int kTwoViewAuto = 2;               // FTK_TWO_VIEW_AUTO
constexpr int kTwoViewHomSample = 4;          // FTK_TWO_VIEW_HOMOGRAPHY_SAMPLE: correspondences of a homography hypothesis
constexpr int kTwoViewMaxPermille = 1000;
constexpr int kTwoViewMaxSlots = 2;

struct TwoViewPlanInput {
    int32_t n;                       // correspondences
    int32_t hypotheses;
    int32_t image_rows, image_cols;
    int32_t slots;                   // 1: the fundamental matrix alone (its mode only), 2: a slot per model
    int32_t mode;                    // kTwoView*
    int32_t prefer_permille;         // 0 .. 1000
};
enum class TwoViewRefusal { None, Sizes, Points, Hypotheses, Mode, Prefer };
struct TwoViewPlan {
    TwoViewRefusal refused;     // not None: nothing else is set
    int32_t slots;              // models the workspace and the outputs hold
    int32_t run_fundamental;    // 1: the fundamental route's hypothesis and score launches take place (slot 0)
    int32_t run_homography;     // 1: the homography's (slot 1)
    int32_t launches;           // scan + 2 per model that runs + select: 4 or 6
    int32_t scan_per_thread;    // consecutive points a thread of the scan workgroup owns (<= 64: its participants are one 64-bit mask)
    size_t scan_lds;            // bytes of its scan array
    uint32_t hyp_blocks;        // workgroups of kEpipolarHypBlock threads of either hypothesis kernel
    size_t hyp_lds;             // bytes of their matrices
    uint32_t score_tiles;       // grid.x of either scoring kernel: tiles of kEpipolarScoreTile participants, sized for n (M is on the device)
    uint32_t score_groups;      // grid.y: groups of kEpipolarScoreGroup hypotheses
    size_t score_lds;           // bytes of a tile of normalised coordinates
    int32_t select_per_thread;  // hypotheses of ONE model a thread of the select workgroup reduces
    // the workspace (ftk_layout.h), in this order: M, the participants' normalised (x1, y1, x2, y2) [n], their indices [n], counts [slots][K],
    // models [slots][K][9], validity flags [slots][K]; the same for every mode
    ftk_slot16<int32_t> m, list, counts;
    ftk_slot16<float4> points;
    ftk_slot16<float> models;
    ftk_slot16<uint8_t> valid;
    size_t bytes;
};
const char *two_view_refusal_name(TwoViewRefusal r);
TwoViewPlan two_view_plan(const TwoViewPlanInput &in);

// One call (two_view_kernels.hip).  A slot's counts / models point into the workspace or at the caller's arrays.
struct TwoViewSlot {
    int32_t *counts;               // [hypotheses]
    float *models;                 // [hypotheses][9]
    uint8_t *valid;                // [hypotheses] workspace
};
struct TwoViewParams {
    const float *ref_uv, *cur_uv;  // [n][2]
    uint8_t *status;               // [n]
    int32_t n, hypotheses;
    float cx, cy, s, tn2;          // the normalisation and the squared normalised threshold
    uint32_t seed;
    int32_t *m;                    // [1] workspace: the number of participants
    float4 *points;                // [n] workspace: participant j's normalised (x1, y1, x2, y2)
    int32_t *list;                 // [n] workspace: participant j's index
    TwoViewSlot slot[kTwoViewMaxSlots];  // kTwoViewFundamental, kTwoViewHomography (one slot: the first alone)
    int32_t prefer_permille;
    int32_t run[kTwoViewMaxSlots];       // the plan's run_fundamental, run_homography (two slots)
    int32_t *model;                // [1] (two slots)
    int32_t *best, *n_inliers;     // [slots] each
    float *F, *H;                  // [9] each; H with two slots
    int32_t scan_per_thread, select_per_thread;
};
hipError_t two_view_launch(const TwoViewPlan &plan, const TwoViewParams &p, hipStream_t stream);

}  // namespace ftk
