// two_view_plan.h — the launch plan and workspace layout of two-view outlier rejection with a choice of model (two_view_kernels.hip,
// DESIGN.md 5.21), as epipolar_plan.h is the fundamental matrix's: a pure function of values (no context, no environment, no HIP call;
// tests/test_two_view_args_cpu.py walks it without a device through host/build/two_view_plan_cli).  ftk_two_view.cpp plans, the launcher
// carries the plan out.
#pragma once

#include "epipolar_plan.h"

namespace ftk {

constexpr int kTwoViewFundamental = 0;   // FTK_TWO_VIEW_FUNDAMENTAL
constexpr int kTwoViewHomography = 1;    // FTK_TWO_VIEW_HOMOGRAPHY
constexpr int kTwoViewAuto = 2;          // FTK_TWO_VIEW_AUTO
constexpr int kTwoViewHomSample = 4;     // FTK_TWO_VIEW_HOMOGRAPHY_SAMPLE: correspondences of a homography hypothesis
constexpr int kTwoViewMaxPermille = 1000;

struct TwoViewPlanInput {
    int32_t n;                       // correspondences
    int32_t hypotheses;
    int32_t image_rows, image_cols;
    int32_t mode;                    // kTwoView*
    int32_t prefer_permille;         // 0 .. 1000
};
enum class TwoViewRefusal { None, Sizes, Points, Hypotheses, Mode, Prefer };
struct TwoViewPlan {
    TwoViewRefusal refused;     // not None: nothing else is set
    int32_t run_fundamental;    // 1: the fundamental route's hypothesis and score launches take place (slot 0)
    int32_t run_homography;     // 1: the homography's (slot 1)
    int32_t launches;           // scan + 2 per model that runs + select: 4 or 6
    int32_t scan_per_thread;    // as EpipolarPlan's, of the ONE scan launch
    uint32_t hyp_blocks;        // workgroups of kEpipolarHypBlock threads of either hypothesis kernel
    size_t hyp_lds;
    uint32_t score_tiles;       // grid.x of either scoring kernel
    uint32_t score_groups;      // grid.y
    size_t score_lds;
    int32_t select_per_thread;  // hypotheses of ONE model a thread of the select workgroup reduces
    // the workspace, byte offsets (16-byte aligned): M (one int32, padded), the participants' normalised (x1, y1, x2, y2), their indices,
    // counts [2][K], models [2][K][9], validity flags [2][K]; the same for every mode
    size_t off_points, off_list, off_counts, off_models, off_valid, bytes;
};
const char *two_view_refusal_name(TwoViewRefusal r);
TwoViewPlan two_view_plan(const TwoViewPlanInput &in);

// One call (two_view_kernels.hip).  `e` is the fundamental route's (epipolar_kernels.hip): its counts / models / valid are slot 0's and it
// carries everything the two models share (the inputs, the normalisation, the seed, M, points, list).  Slot 1 is the homography's.
struct TwoViewParams {
    EpipolarParams e;
    int32_t *counts_h;             // [hypotheses]
    float *models_h;               // [hypotheses][9]
    uint8_t *valid_h;              // [hypotheses] workspace
    int32_t mode, prefer_permille, run_fundamental, run_homography;
    int32_t *model;                // [1]
    int32_t *best, *n_inliers;     // [2] each
    float *F, *H;                  // [9] each
};
hipError_t two_view_launch(const TwoViewPlan &plan, const TwoViewParams &p, hipStream_t stream);

}  // namespace ftk
