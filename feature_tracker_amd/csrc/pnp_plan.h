// pnp_plan.h — the launch plan and workspace layout of PnpRansac (pnp_kernels.hip), as two_view_pose_plan.h is
// TwoViewPose's: a pure function of values (no context, no environment, no HIP call; tests/test_pnp_args_cpu.py walks it without a device
// through host/build/pnp_plan_cli).  ftk_pnp.cpp plans, the launcher carries the plan out.
#pragma once

#include "two_view_pose_plan.h"

namespace ftk {

constexpr int kPnpSample = 6;           // FTK_PNP_SAMPLE: participants of a hypothesis
constexpr int kPnpRefitRows = 6;        // a refit step needs this many rows (the six-point sample's size, under either sampler)
constexpr int kP3pSample = 4;           // participants of a "p3p" hypothesis: three to the solver, the fourth chooses
constexpr int kP3pCubicSteps = 64;      // Newton steps on the resolvent cubic from Cauchy's bound
constexpr int kP3pCubicPolish = 4;      // ... and after the deflation
constexpr int kP3pNewtonSteps = 1;      // Newton steps on the three distance equations per root
constexpr float kP3pResidual = 0.0000152587890625f;  // 2^-16: a solution's residuals against the sum of its two squared distances
constexpr int kPnpRows = 11;            // rows of the DLT system that are eliminated (two per participant, the twelfth dropped)
constexpr int kPnpModelFloats = 12;     // FTK_PNP_MODEL_FLOATS: a hypothesis, P = [A | b] row-major
constexpr int kPnpHypLdsFloats = 156;   // per lane: the 11 x 12 matrix, the 12 column indices, the 12 entries of the null vector
constexpr int kPnpSums = 27;            // a refit step's sums: the 21 distinct entries of J^T J, row-major upper triangle, then J^T r
constexpr int kPnpMaxRefine = 16;       // FTK_PNP_MAX_REFINE_ITERATIONS
constexpr int kPnpStateFloats = 8;      // the pose between the kernels: q_rc (w, x, y, z), p_rc, one unused
constexpr int kPnpFlags = 4;            // ok (the select kernel formed a pose), done (the refit has ended), the winner, one unused

enum class PnpSample : int32_t { Dlt6 = 0, P3p = 1 };  // FTK_PNP_SAMPLE_DLT6, FTK_PNP_SAMPLE_P3P
struct PnpPlanInput {
    int32_t n;  // landmarks
    int32_t hypotheses;
    int32_t refine_iterations;
    PnpSample sampler = PnpSample::Dlt6;
};
enum class PnpRefusal { None, Sizes, Points, Hypotheses, Refine, Sampler };
struct PnpPlan {
    PnpRefusal refused;        // not None: nothing else is set
    int32_t launches;          // scan, hypotheses, score, select, two per refit step (sums, step), finish: 5 + 2 refine_iterations
    int32_t refine_iterations;
    PnpSample sampler;         // which hypothesis kernel is launched
    int32_t sample;            // participants of a hypothesis, and the fewest a call needs: 6 (Dlt6) or 4 (P3p)
    int32_t scan_per_thread;   // consecutive points a thread of the scan workgroup owns (<= 64)
    uint32_t hyp_blocks;       // workgroups of kEpipolarHypBlock lanes of the hypothesis kernel
    size_t hyp_lds;            // bytes of their matrices (0 under P3p: its kernel holds none)
    uint32_t score_tiles;      // grid.x of the scoring kernel: tiles of kEpipolarScoreTile participants, sized for n (M is on the device)
    uint32_t score_groups;     // grid.y: groups of kEpipolarScoreGroup hypotheses
    int32_t select_per_thread; // hypotheses a thread of the select workgroup reduces
    uint32_t tiles;            // grid of the sums and finish kernels: tiles of kPoseTile participants, sized for n
    size_t sums_lds;           // bytes of a tile's 27 x 256 tree
    // the workspace (ftk_layout.h), in this order: M, the participants' (x, y, X, Y) [n], their Z [n], their indices [n], counts [K], models
    // [K][12], validity flags [K], the tile totals [tiles][27], the tiles' inlier counts [tiles], the pose, the flags
    ftk_slot16<int32_t> m;
    ftk_slot16<float4> points;
    ftk_slot16<float> depth;
    ftk_slot16<int32_t> list, counts;
    ftk_slot16<float> models;
    ftk_slot16<uint8_t> valid;
    ftk_slot16<float> totals;
    ftk_slot16<int32_t> tile_counts;
    ftk_slot16<float> state;
    ftk_slot16<int32_t> flags;
    size_t bytes;
};
const char *pnp_refusal_name(PnpRefusal r);
PnpPlan pnp_plan(const PnpPlanInput &in);

struct PnpParams {
    const float *landmarks;  // [n][3]
    const float *uv;         // [n][2]
    uint8_t *status;         // [n]
    int32_t n, hypotheses;
    float fx, fy, cx, cy;
    float ry, tn2;           // fy / fx, (threshold / fx)^2
    uint32_t seed;
    int32_t *m;              // [1] workspace: the number of participants
    float4 *points;          // [n] workspace: participant j's calibrated (x, y) and its landmark's (X, Y)
    float *depth;            // [n] workspace: its landmark's Z
    int32_t *list;           // [n] workspace: its index
    int32_t *counts;         // [hypotheses] workspace or the caller's
    float *models;           // [hypotheses][12] workspace or the caller's
    uint8_t *valid;          // [hypotheses] workspace
    float *totals;           // [tiles][27] workspace
    int32_t *tile_counts;    // [tiles] workspace
    float *state;            // [kPnpStateFloats] workspace
    int32_t *flags;          // [kPnpFlags] workspace
    float *pose;             // [7]
    int32_t *n_inliers, *best, *out_valid;  // [1] each
    int32_t scan_per_thread, select_per_thread;
    int32_t sample;          // the plan's (the launcher sets it): below it the score and select kernels form nothing
    int32_t step;            // the refit step a sums kernel belongs to (the launcher sets it)
};
hipError_t pnp_launch(const PnpPlan &plan, const PnpParams &p, hipStream_t stream);

}  // namespace ftk
