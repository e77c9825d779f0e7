// epipolar_plan.h — the launch plan and workspace layout of two-view outlier rejection (epipolar_kernels.hip), as
// track_table_plan.h is the track table's: a pure function of values (no context, no environment, no HIP call;
// tests/test_epipolar_args_cpu.py walks it without a device through host/build/epipolar_plan_cli).  ftk_epipolar.cpp plans, the launcher
// carries the plan out.
#pragma once

#include "ftk_device.h"

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

struct EpipolarPlanInput {
    int32_t n;                       // correspondences
    int32_t hypotheses;
    int32_t image_rows, image_cols;
};
enum class EpipolarRefusal { None, Sizes, Points, Hypotheses };
struct EpipolarPlan {
    EpipolarRefusal refused;    // not None: nothing else is set
    int32_t scan_per_thread;    // consecutive points a thread of the scan workgroup owns (<= 64: its participants are one 64-bit mask)
    size_t scan_lds;            // bytes of its scan array
    uint32_t hyp_blocks;        // workgroups of kEpipolarHypBlock threads of the hypothesis kernel
    size_t hyp_lds;             // bytes of their matrices
    uint32_t score_tiles;       // grid.x of the scoring kernel: tiles of kEpipolarScoreTile participants, sized for n (M is on the device)
    uint32_t score_groups;      // grid.y: groups of kEpipolarScoreGroup hypotheses
    size_t score_lds;           // bytes of a tile of normalised coordinates
    int32_t select_per_thread;  // hypotheses a thread of the select workgroup reduces
    // the workspace, byte offsets (16-byte aligned): M (one int32, padded), the participants' normalised (x1, y1, x2, y2), their indices,
    // counts, models, validity flags
    size_t off_points, off_list, off_counts, off_models, off_valid, bytes;
};
const char *epipolar_refusal_name(EpipolarRefusal r);
EpipolarPlan epipolar_plan(const EpipolarPlanInput &in);

// One call (epipolar_kernels.hip).  counts / models point into the workspace or at the caller's arrays.
struct EpipolarParams {
    const float *ref_uv, *cur_uv;  // [n][2]
    uint8_t *status;               // [n]
    int32_t n, hypotheses;
    float cx, cy, s, tn2;          // the normalisation and the squared normalised threshold
    uint32_t seed;
    int32_t *m;                    // [1] workspace: the number of participants
    float4 *points;                // [n] workspace: participant j's normalised (x1, y1, x2, y2)
    int32_t *list;                 // [n] workspace: participant j's index
    int32_t *counts;               // [hypotheses]
    float *models;                 // [hypotheses][9]
    uint8_t *valid;                // [hypotheses] workspace
    int32_t *best, *n_inliers;     // [1] each
    float *F;                      // [9]
    int32_t scan_per_thread, select_per_thread;
};
hipError_t epipolar_launch(const EpipolarPlan &plan, const EpipolarParams &p, hipStream_t stream);
// The same kernels one at a time, for the two-view entry (two_view_kernels.hip), which shares the scan between two models and has a
// select kernel of its own.  p carries scan_per_thread; best / n_inliers / F are not read.
void epipolar_launch_scan(const EpipolarParams &p, hipStream_t stream);
void epipolar_launch_hypotheses(uint32_t hyp_blocks, const EpipolarParams &p, hipStream_t stream);
void epipolar_launch_score(uint32_t score_tiles, uint32_t score_groups, const EpipolarParams &p, hipStream_t stream);

}  // namespace ftk
