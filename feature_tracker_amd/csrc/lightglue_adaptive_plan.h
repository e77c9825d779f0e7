// lightglue_adaptive_plan.h — the launch plan and workspace layout of LightGlue's adaptive pass (lightglue_adaptive_kernels.hip, DESIGN.md
// 5.26), as transformer_plan.h is the layer's: a pure function of values (no context, no environment, no HIP call;
// tests/test_lightglue_adaptive_args_cpu.py walks it without a device through host/build/lightglue_adaptive_plan_cli).
// ftk_lightglue_adaptive.cpp plans, the launcher carries the plan out: every grid it launches is a field of the plan.
#pragma once

#include "ftk_device.h"
#include "ftk_layout.h"

namespace ftk {

constexpr int kAdaptiveMaxLayers = 64;       // FTK_LIGHTGLUE_MAX_LAYERS: L
constexpr int kAdaptiveConfThreads = 64;     // confidence_kernel: one row per thread
constexpr int kAdaptiveDecideThreads = 256;  // decide_kernel: ONE workgroup; a thread owns ceil(rows / 256) <= 16 consecutive rows of a side
constexpr int kAdaptiveGatherThreads = 64;   // gather_kernel: one wave per destination row
constexpr int kAdaptiveCopyThreads = 256;    // head_select_kernel and remap_kernel
constexpr int kAdaptiveCopyMaxBlocks = 1024;
constexpr int kAdaptiveUnmatched = 2;        // the status of a row without a match (FTK_STATUS_LARGE_RESIDUAL), as ftk_nn_match_scores_device's
// the words of the pass's state, int32 [kAdaptiveStateWords] in device memory
enum AdaptiveState { kStateLive0 = 0, kStateLive1 = 1, kStateStopped = 2, kStateStopLayer = 3, kAdaptiveStateWords = 4 };

struct LightglueAdaptivePlanInput {
    int32_t rows0, rows1;  // M, N
    int32_t dim;           // D
    int32_t heads;         // h
};
enum class LightglueAdaptiveRefusal { None, Layer, Assignment };  // the transformer layer's plan refused, the assignment head's
struct LightglueAdaptivePlan {
    LightglueAdaptiveRefusal refused;  // not None: nothing else is set
    uint32_t conf_blocks;              // kAdaptiveConfThreads rows of the M + N
    uint32_t decide_blocks;            // 1
    uint32_t gather_blocks;            // M + N
    uint32_t select_blocks, remap_blocks;  // grid-stride over the head's (D + 1) D + D + 1 floats and M indices; over M + N rows
    int32_t step_launches;             // 3 per layer in front of the last: confidence, decide, gather
    int32_t finish_launches;           // 2 on top of the head's and the matcher's: head select, remap
    // the workspace (ftk_layout.h), in this order: the layer's workspace and the assignment head's (with weights) as the bytes of their
    // own plans, the selected head [D + 1][D] and [D + 1], the gather maps [M], [N], the matcher's index [M] and status [M]
    ftk_slot16<uint8_t> layer, assign, status;
    ftk_slot16<float> head_w, head_b;
    ftk_slot16<int32_t> src0, src1, match;
    size_t bytes;
};
const char *lightglue_adaptive_refusal_name(LightglueAdaptiveRefusal r);
// confidence_kernel's grid for `rows` rows of both sets: the plan's conf_blocks, and the grid of the confidence entry alone.
uint32_t lightglue_confidence_blocks(int64_t rows);
LightglueAdaptivePlan lightglue_adaptive_plan(const LightglueAdaptivePlanInput &in);

struct ConfidenceParams {
    const float *desc0, *desc1;       // [M][D], [N][D]
    int32_t rows0, rows1, dim;
    const float *token_w, *token_b;   // [D], [1]
    const float *match_w, *match_b;   // [D], [1]
    const int32_t *live0, *live1;     // device words or null: rows at or behind clamp(live, 0, rows) are skipped
    const int32_t *gate;              // device word or null: nothing is done when *gate != 0
    float *conf, *mt;                 // [M + N] each, the second set from M
};
hipError_t confidence_launch(const LightglueAdaptivePlan &plan, const ConfidenceParams &p, hipStream_t stream);

struct AdaptStepParams {
    const float *conf, *mt;           // [M + N]
    int32_t rows0, rows1, dim, head_dim;
    const int32_t *count0, *count1;   // the input counts (P = their clamped sum); device words or null
    int32_t *state;                   // [kAdaptiveStateWords]
    int32_t layer;                    // i
    int32_t depth_on, width_on;
    float threshold, depth, width;    // t_i, (float)depth_confidence, (float)(1 - width_confidence)
    int32_t min_keypoints;
    int32_t *src0, *src1;             // workspace: the source row of each destination row
    const float *desc_in0, *desc_in1, *enc_in0, *enc_in1;
    const int32_t *ind_in0, *ind_in1;
    float *desc_out0, *desc_out1, *enc_out0, *enc_out1;
    int32_t *ind_out0, *ind_out1;
    int32_t *layers0, *layers1;       // [M], [N]
};
hipError_t adapt_step_launch(const LightglueAdaptivePlan &plan, const AdaptStepParams &p, hipStream_t stream);

struct FinishParams {
    int32_t rows0, rows1, dim, n_layers;
    const float *head_w, *head_b;     // [L][D + 1][D], [L][D + 1]
    float *sel_w, *sel_b;             // workspace
    const int32_t *state;
    const int32_t *ind0, *ind1;
    const int32_t *match;             // the matcher's index in compacted space [M]
    const uint8_t *status_in;         // and its status [M]
    int32_t *match_index;             // [M], original indices
    uint8_t *status;                  // [M]
    int32_t *layers0, *layers1;
};
hipError_t head_select_launch(const LightglueAdaptivePlan &plan, const FinishParams &p, hipStream_t stream);
hipError_t remap_launch(const LightglueAdaptivePlan &plan, const FinishParams &p, hipStream_t stream);

}  // namespace ftk
