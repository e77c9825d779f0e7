// ftk_corr_ondemand.cpp — RAFT's on-demand correlation of the C ABI (include/ftk.h): layout, prepare, lookup.  No volume:
// the workspace holds the two feature maps channel-last (fmap1 pooled through the levels) and a lookup computes the correlation values its
// windows read.  The geometry of every launch is raft_corr_ondemand_plan's.
#include <math.h>

#include "ftk_internal.h"
#include "raft_corr_ondemand_plan.h"

namespace {

// the plan's refusal as the entry's error; `what` is the entry's name
int refuse(ftk_context *ctx, const char *what, const ftk::CorrOdPlan &p, int32_t B, int32_t C, int32_t H, int32_t W, int32_t levels, int32_t radius) {
    switch (p.refused) {
    case ftk::CorrOdRefusal::Sizes:
        return ftk_fail(ctx, FTK_E_INVALID_ARGUMENT, "%s: sizes B %d, H %d, W %d must be positive", what, B, H, W);
    case ftk::CorrOdRefusal::Channels:
        return ftk_fail(ctx, FTK_E_INVALID_ARGUMENT, "%s: %d channels", what, C);
    case ftk::CorrOdRefusal::Levels:
        return ftk_fail(ctx, FTK_E_INVALID_ARGUMENT, "%s: %d levels (1 .. %d)", what, levels, FTK_CORR_MAX_LEVELS);
    case ftk::CorrOdRefusal::EmptyLevel:
        return ftk_fail(ctx, FTK_E_INVALID_ARGUMENT,
                        "%s: level %d of %d x %d feature maps would be %d x %d (the reference's avg_pool2d raises): use at most %d levels", what, p.empty_level, H,
                        W, H >> p.empty_level, W >> p.empty_level, p.empty_level);
    case ftk::CorrOdRefusal::Radius:
        return ftk_fail(ctx, FTK_E_INVALID_ARGUMENT, "%s: radius %d (0 .. %d)", what, radius, FTK_CORR_MAX_RADIUS);
    case ftk::CorrOdRefusal::Overflow:
        return ftk_fail(ctx, FTK_E_INVALID_ARGUMENT, "%s: the workspace of B %d, C %d, %d x %d, %d levels does not fit in a byte count", what, B, C, H, W, levels);
    case ftk::CorrOdRefusal::Grid:
        return ftk_fail(ctx, FTK_E_INVALID_ARGUMENT, "%s: B %d, C %d, %d x %d is beyond the launch grid", what, B, C, H, W);
    case ftk::CorrOdRefusal::None:
        break;
    }
    return FTK_OK;
}

ftk::CorrOdPlan plan_of(int32_t B, int32_t C, int32_t H, int32_t W, int32_t levels, int32_t radius, const void *workspace) {
    ftk::CorrOdPlanInput in{};
    in.B = B, in.C = C, in.H = H, in.W = W, in.levels = levels, in.radius = radius;
    in.aligned16 = (reinterpret_cast<uintptr_t>(workspace) & 15) == 0 ? 1 : 0;
    return ftk::raft_corr_ondemand_plan(in);
}

}  // namespace

extern "C" {

int ftk_corr_ondemand_layout(int32_t B, int32_t C, int32_t H, int32_t W, int32_t levels, int64_t *elements, int64_t *level_offsets, int32_t *level_h,
                             int32_t *level_w) {
    if (!elements) {
        return ftk_fail(nullptr, FTK_E_INVALID_ARGUMENT, "corr_ondemand_layout: null output");
    }
    const ftk::CorrOdPlan p = plan_of(B, C, H, W, levels, 0, nullptr);
    if (p.refused != ftk::CorrOdRefusal::None) {
        return refuse(nullptr, "corr_ondemand_layout", p, B, C, H, W, levels, 0);
    }
    for (int32_t l = 0; l < levels; ++l) {
        if (level_offsets) {
            level_offsets[l] = p.level_offset[l];
        }
        if (level_h) {
            level_h[l] = p.level_h[l];
        }
        if (level_w) {
            level_w[l] = p.level_w[l];
        }
    }
    *elements = p.elements;
    return FTK_OK;
}

int ftk_corr_ondemand_prepare_device(ftk_context *ctx, void *stream, const float *d_fmap0, const float *d_fmap1, int32_t B, int32_t C, int32_t H,
                                     int32_t W, int32_t levels, float *d_workspace) {
    if (!ctx) {
        return ftk_fail(nullptr, FTK_E_INVALID_ARGUMENT, "corr_ondemand_prepare_device: null context");
    }
    FTK_LOCK(ctx);
    if (!d_fmap0 || !d_fmap1 || !d_workspace) {
        return ftk_fail(ctx, FTK_E_INVALID_ARGUMENT, "corr_ondemand_prepare_device: null argument");
    }
    const ftk::CorrOdPlan p = plan_of(B, C, H, W, levels, 0, d_workspace);
    if (p.refused != ftk::CorrOdRefusal::None) {
        return refuse(ctx, "corr_ondemand_prepare_device", p, B, C, H, W, levels, 0);
    }
    FTK_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    ftk::CorrOdTransposeParams t{};
    t.f0 = d_fmap0;
    t.f1 = d_fmap1;
    t.out0 = d_workspace;
    t.out1 = d_workspace + p.level_offset[0];
    t.B = B;
    t.C = C;
    t.HW = (int64_t)H * W;
    FTK_HIP(ctx, ftk::corr_od_transpose_launch(t, p.transpose_grid, p.transpose_block, s));
    for (int32_t l = 1; l < levels; ++l) {  // chained: level l from level l - 1
        ftk::CorrOdPoolParams q{};
        q.src = d_workspace + p.level_offset[l - 1];
        q.dst = d_workspace + p.level_offset[l];
        q.B = B;
        q.C = C;
        q.hin = p.level_h[l - 1];
        q.win = p.level_w[l - 1];
        FTK_HIP(ctx, ftk::corr_od_pool_launch(q, p.pool_blocks[l], s));
    }
    return FTK_OK;
}

int ftk_corr_ondemand_lookup_device(ftk_context *ctx, void *stream, const float *d_workspace, int32_t B, int32_t C, int32_t H, int32_t W,
                                    int32_t levels, int32_t radius, const float *d_coords, float *d_out, int32_t per_level) {
    if (!ctx) {
        return ftk_fail(nullptr, FTK_E_INVALID_ARGUMENT, "corr_ondemand_lookup_device: null context");
    }
    FTK_LOCK(ctx);
    if (!d_workspace || !d_coords || !d_out) {
        return ftk_fail(ctx, FTK_E_INVALID_ARGUMENT, "corr_ondemand_lookup_device: null argument");
    }
    const ftk::CorrOdPlan p = plan_of(B, C, H, W, levels, radius, d_workspace);
    if (p.refused != ftk::CorrOdRefusal::None) {
        return refuse(ctx, "corr_ondemand_lookup_device", p, B, C, H, W, levels, radius);
    }
    FTK_HIP(ctx, hipSetDevice(ctx->device));
    ftk::CorrOdLookupParams q{};
    q.workspace = d_workspace;
    q.coords = d_coords;
    q.out = d_out;
    q.B = B;
    q.C = C;
    q.H = H;
    q.W = W;
    q.levels = levels;
    q.radius = radius;
    q.per_level = per_level ? 1 : 0;
    q.lattice_side = p.lattice_side;
    q.vector = p.vector;
    q.divisor = (float)sqrt((double)C);  // the all-pairs build's divisor (ftk_corr.cpp)
    for (int32_t l = 0; l < levels; ++l) {
        q.level_offset[l] = p.level_offset[l];
        q.level_h[l] = p.level_h[l];
        q.level_w[l] = p.level_w[l];
    }
    FTK_HIP(ctx, ftk::corr_od_lookup_launch(q, p.lookup_grid, p.lookup_block, static_cast<hipStream_t>(stream)));
    return FTK_OK;
}

}  // extern "C"
